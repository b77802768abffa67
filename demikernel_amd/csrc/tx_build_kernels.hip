// tx_build_kernels.hip — CDNA4 (gfx950) kernels that build TCP frames from connection state: the emit passes, i.e. the
// device halves of calls whose plan and commit kernels and host entry points are elsewhere:
//   dk_tcp_tx_emit_kernel    dk_tcp_tx_segment (tcp_tx_kernels.hip): pushed buffers copied, summed and cut into frames;
//   dk_tcp_rtx_emit_kernel   dk_tcp_retransmit (tcp_tx_kernels.hip): queue entries resent under fresh headers;
//   dk_tcp_ack_emit_kernel   dk_tcp_ack_emit (tcp_ackemit_kernels.hip) and dk_tcp_ack_timer (tcp_tx_kernels.hip): the
//                            receiver's pure ACKs;
// and their launchers (declared in rx_common.h). They read no frame: payloads are copied by tcp_tx_copy_sum below, and
// the 54 header bytes come from registers through frame_build.h (tx_store_header, the checksum residue arithmetic),
// which dk_tx_serialize_kernel in rx_kernels.hip uses too. That kernel stays there because its payload sums are the
// receive kernels' frame stream (stream_chunk).
#include <hip/hip_runtime.h>

#include "frame_build.h"
#include "rx_common.h"

namespace dk {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// TCP send segmentation, emit pass (dk_tcp_tx_segment, dk_tcp.h). The plan kernels (tcp_tx_kernels.hip) left, per
// pushed buffer, the bytes it may send, the sequence number of its first byte and the exclusive scan of the frame
// counts. Here a wave takes 64-frame chunks round-robin over the persistent grid: each lane finds its frame's buffer
// by a search of that scan (64 searches at once), then the wave copies the chunk's payloads four frames at a time,
// one quarter-wave per frame (a whole wave per frame, two loads per lane in flight and one 64-lane reduction per frame,
// took 1,017 us at 1M x 1460 B where this takes 892): 16-byte granules aligned on the DESTINATION
// (a frame slot: the payload sits at slot + lead + 54, an unrelated residue to the source piece's, which starts at
// off + j * mss), loaded from the source at whatever alignment that leaves (the hardware takes unaligned global loads;
// with both sides aligned the kernel is 3 % faster, so no realignment in registers was built), the up to 15 bytes in
// front of the first and behind the last whole granule as bytes. Every payload byte is read once and written once; the granules are summed
// as they pass (hsum2). Their 16-bit grid is the destination's: when the payload starts at an odd address it is the
// payload's grid shifted by one byte, and the residue is byte-swapped once per lane (x256 mod 0xFFFF). After each four
// frames the lanes that own them build their 54 header bytes from registers, with dk_tx_serialize's arithmetic and
// stores.
// ---------------------------------------------------------------------------------------------------------------------
// A 16-byte global load at any address.
__device__ __forceinline__ uint4 load16_any(const uint8_t* p) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4), aligned(1)));
    const v4u v = *(const __attribute__((address_space(1))) v4u*)(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// Copy L bytes src -> dst with one quarter-wave (`sub` = the lane's index in it, 0..15; the quarters of a wave work on
// four frames at once); returns, in each of its lanes, their LE-half sum on the payload's own grid (byte k weighs
// 2^(8 (k & 1))). Up to kTxGranules 16-byte loads per lane are in flight together: six cover a 1460-byte piece in one
// round (92 granules over 16 lanes).
constexpr int kTxSub = 16, kTxGranules = 6;
__device__ __forceinline__ uint32_t tcp_tx_copy_sum(const uint8_t* src, uint8_t* dst, uint32_t L, uint32_t sub) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const uint32_t dmis = (uint32_t)reinterpret_cast<uintptr_t>(dst) & 15u;
    const uint32_t head = min((16u - dmis) & 15u, L);  // bytes in front of the first aligned granule
    const uint32_t ng = (L - head) >> 4;               // whole granules
    const uint32_t tail0 = head + 16u * ng;            // payload index of the first byte behind them
    uint32_t accb = 0, accg = 0;
    {
        // lane `sub` takes head byte `sub` and tail byte `sub` (at most 15 of each)
        const uint32_t kt = tail0 + sub;
        const bool hon = sub < head, ton = kt < L;
        uint32_t hb = 0, tb = 0;
        if (hon) hb = gptr(src)[sub];
        if (ton) tb = gptr(src)[kt];
        if (hon) gptr(dst)[sub] = (uint8_t)hb;
        if (ton) gptr(dst)[kt] = (uint8_t)tb;
        accb = (hb << ((sub & 1u) * 8)) + (tb << ((kt & 1u) * 8));
    }
    const uint8_t* s = src + head;
    uint8_t* d = dst + head;
    for (uint32_t g0 = sub; g0 < ng; g0 += kTxSub * kTxGranules) {
        uint4 v[kTxGranules];
#pragma unroll
        for (int u = 0; u < kTxGranules; u++) {
            v[u] = make_uint4(0, 0, 0, 0);
            if (g0 + u * kTxSub < ng) v[u] = load16_any(s + 16 * (size_t)(g0 + u * kTxSub));
        }
#pragma unroll
        for (int u = 0; u < kTxGranules; u++) {
            if (g0 + u * kTxSub < ng)
                *gptr(reinterpret_cast<u32x4*>(d + 16 * (size_t)(g0 + u * kTxSub))) = u32x4{v[u].x, v[u].y, v[u].z, v[u].w};
            accg = hsum2(v[u].w, hsum2(v[u].z, hsum2(v[u].y, hsum2(v[u].x, accg))));
        }
    }
    uint32_t r = mod_ffff(accg);
    if (head & 1u) r = bswap16(r);  // the granules' grid is one byte off the payload's
    uint32_t t = accb + r;          // < 2^18 per lane
    for (int o = 1; o < kTxSub; o <<= 1) t += (uint32_t)__shfl_xor((int)t, o);
    return t;
}

__global__ __launch_bounds__(kBlock) void dk_tcp_tx_emit_kernel(TcpTxEmitParams P) {
    const uint64_t total = *P.total;
    if (!tcp_tx_fits(total, P.max_frames, P.stride, P.out_bytes)) return;  // all or nothing, the call's one device-side test
    const uint32_t n = (uint32_t)total;
    const uint32_t lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t nw = gridDim.x * kWaves, gw = blockIdx.x * kWaves + wv;
    const uint32_t nchunks = n / 64 + (n % 64 != 0);
    for (uint32_t ch = gw; ch < nchunks; ch += nw) {
        const uint32_t f0 = ch * 64, f = f0 + lane;
        const bool live = f < n;
        uint32_t bi = 0, plen = 0, seq = 0, ack = 0, win = 0, b13 = 0x10u, conn = 0, slo = 0, shi = 0;
        if (live) {
            uint32_t lo = 0, hi = P.nbufs;  // the last buffer whose first frame is <= f
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (P.first[mid] <= f) lo = mid;
                else hi = mid;
            }
            bi = lo;
            const uint4 r = reinterpret_cast<const uint4*>(P.rec)[bi];
            const uint32_t j = f - (uint32_t)P.first[bi];  // the piece of the buffer
            conn = P.conn[bi];
            const uint32_t mss = P.tx[conn].mss, blen = P.len[bi];
            const uint64_t done = (uint64_t)j * mss;
            plen = r.x ? min(mss, r.x - (uint32_t)done) : 0u;
            // the piece that ends the buffer carries PSH, the end-of-send marker's frame FIN (sender.rs:161-189)
            const bool ends = done + plen >= r.x && r.x == blen;
            b13 = 0x10u | (ends ? (blen ? 0x08u : 0x01u) : 0u);
            const uint64_t so = (uint64_t)P.off[bi] + done;
            slo = (uint32_t)so;
            shi = (uint32_t)(so >> 32);
            seq = r.y + (uint32_t)done;
            ack = r.z;
            win = r.w;
        }
        // the frame's results, and its connection's header fields (the arithmetic of tx_seg_finish for a TCP segment
        // without options, H = 54), loaded before the copy
        const uint32_t foff = (uint32_t)((uint64_t)f * P.stride + P.lead);
        uint32_t src = 0, dst = 0, ports = 0, ipw = 0;
        uint3 Lk = make_uint3(0, 0, 0);
        if (live) {
            __builtin_nontemporal_store(foff, gptr(P.off_out) + f);
            __builtin_nontemporal_store((uint16_t)(54u + plen), gptr(P.len_out) + f);
            if (P.frame_buf) __builtin_nontemporal_store(bi, gptr(P.frame_buf) + f);
            const dk_tcp_tx_conn& T = P.tx[conn];
            src = T.local_ip, dst = T.remote_ip, ports = T.ports, ipw = T.ip_word;
            const uint32_t* lw = reinterpret_cast<const uint32_t*>(P.links + T.link);
            Lk = make_uint3(lw[0], lw[1], lw[2]);
        }
        const uint32_t cnt = min(64u, n - f0);
        const uint32_t sub = lane & (kTxSub - 1), q = lane / kTxSub;
        for (uint32_t t = 0; t < cnt; t += 64 / kTxSub) {  // quarter q copies frame t + q
            const uint32_t fr = t + q;
            const uint64_t so = (uint64_t)(uint32_t)__shfl((int)slo, (int)fr) | (uint64_t)(uint32_t)__shfl((int)shi, (int)fr) << 32;
            const uint32_t lf = (uint32_t)__shfl((int)plen, (int)fr);  // every lane shuffles: a quarter past the chunk's
            const uint32_t L = fr < cnt ? lf : 0u;                     // end still holds frames the others read
            uint8_t* pay = P.out + ((uint64_t)(f0 + fr) * P.stride + P.lead + 54u);
            const uint32_t s = tcp_tx_copy_sum(P.src + so, pay, L, sub);
            // the sum of frame `lane`, from the quarter that copied it
            const uint32_t le = (uint32_t)__shfl((int)s, (int)(((lane - t) & (64 / kTxSub - 1)) * kTxSub));
            // The four lanes that own these frames store their headers now, right behind the payload's first line, which
            // the header shares (against storing all 64 headers after the chunk: 1 % less of the plain copy's time in
            // the same run, DESIGN.md section 4: inside what two runs differ).
            if (!(live && lane >= t && lane < t + 64 / kTxSub)) continue;
            const uint32_t tot = 40u + plen, seg = 20u + plen;
            const uint32_t ident = ipw & 0xFFFFu, ttl = (ipw >> 16) & 0xFFu, tos = ipw >> 24;
            const uint32_t ipsum = (0x4500u | tos) + tot + ident + 0x4000u + ((ttl << 8) | 6u) + ip_be_sum(src) + ip_be_sum(dst);
            const uint32_t ipc = csum_from_residue(mod_ffff(ipsum));
            const uint32_t sport = ports & 0xFFFFu, dport = ports >> 16;
            const uint32_t b12 = 5u << 4;
            uint32_t c = 0;
            if (!(P.flags & DK_TX_OFFLOAD_TCP)) {
                const uint32_t be = ip_be_sum(src) + ip_be_sum(dst) + 6u + seg + sport + dport + be16_sum(seq) +
                                    be16_sum(ack) + ((b12 << 8) | b13) + win;
                c = csum_from_residue(mod_ffff(be_residue(le) + be));
            }
            uint32_t d[14];
            d[0] = Lk.x;
            d[1] = Lk.y;
            d[2] = Lk.z;
            d[3] = 0x0008u | 0x45u << 16 | tos << 24;
            d[4] = bswap16(tot) | bswap16(ident) << 16;
            d[5] = 0x0040u | ttl << 16 | 6u << 24;
            d[6] = bswap16(ipc) | (src & 0xFFFFu) << 16;
            d[7] = (src >> 16) | (dst & 0xFFFFu) << 16;
            d[8] = (dst >> 16) | bswap16(sport) << 16;
            const uint32_t sq = __builtin_bswap32(seq), ak = __builtin_bswap32(ack);
            d[9] = bswap16(dport) | sq << 16;
            d[10] = (sq >> 16) | ak << 16;
            d[11] = (ak >> 16) | b12 << 16 | b13 << 24;
            d[12] = bswap16(win) | bswap16(c) << 16;
            d[13] = 0;
            tx_store_header(P.out + foff, d, true);
        }
    }
}

// Retransmission, emit pass (dk_tcp_retransmit, dk_tcp.h): the kernel above with a connection's front queue entry in
// place of a pushed buffer's piece. It is frame-major: rtx_plan (tcp_tx_kernels.hip) left, per connection, a record of
// the entry and the header fields, and the exclusive scan of the emit flags numbers the frames, so frame f belongs to
// the largest c with first[c] <= f (the connection that emits is the last one holding its scan value). A burst of 200
// in a table of 100k connections costs 200 searches and 200 frames' copies; no wave walks the table. The entry goes out
// whole, whatever the connection's mss is now; PSH or FIN follows from its length.
__global__ __launch_bounds__(kBlock) void dk_tcp_rtx_emit_kernel(TcpRtxEmitParams P) {
    const uint64_t total = *P.total;
    if (!tcp_tx_fits(total, P.max_frames, P.stride, P.out_bytes)) return;  // all or nothing, as rtx_commit tests it
    const uint32_t n = (uint32_t)total;
    const uint32_t lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t nw = gridDim.x * kWaves, gw = blockIdx.x * kWaves + wv;
    // A wave takes `per` frames a round: 64 when every wave of the grid has that many, else the power of two (4 at the
    // least: one per quarter) that spreads the call's frames over the grid, so that a burst of a few hundred frames is
    // not copied by a handful of waves, four frames at a time, while the rest of the chip idles.
    uint32_t per = 64 / kTxSub;
    while (per < 64 && (uint64_t)per * nw < n) per <<= 1;
    const uint32_t nchunks = n / per + (n % per != 0);
    for (uint32_t ch = gw; ch < nchunks; ch += nw) {
        const uint32_t f0 = ch * per, f = f0 + lane;
        const bool live = lane < per && f < n;
        uint32_t plen = 0, seq = 0, ack = 0, win = 0, b13 = 0x10u, conn = 0, so = 0;
        if (live) {
            uint32_t lo = 0, hi = P.nconns;  // the last connection whose frame index is <= f
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (P.first[mid] <= f) lo = mid;
                else hi = mid;
            }
            conn = lo;
            const uint4 r = reinterpret_cast<const uint4*>(P.rec)[conn];
            so = r.x;
            plen = r.y & 0xFFFFu;
            win = r.y >> 16;
            seq = r.z;
            ack = r.w;
            b13 = 0x10u | (plen ? 0x08u : 0x01u);  // retransmit(): PSH on data, FIN for the marker (sender.rs:396-401)
        }
        const uint32_t foff = (uint32_t)((uint64_t)f * P.stride + P.lead);
        uint32_t src = 0, dst = 0, ports = 0, ipw = 0;
        uint3 Lk = make_uint3(0, 0, 0);
        if (live) {
            __builtin_nontemporal_store(foff, gptr(P.off_out) + f);
            __builtin_nontemporal_store((uint16_t)(54u + plen), gptr(P.len_out) + f);
            if (P.frame_conn) __builtin_nontemporal_store(conn, gptr(P.frame_conn) + f);
            const dk_tcp_tx_conn& T = P.tx[conn];
            src = T.local_ip, dst = T.remote_ip, ports = T.ports, ipw = T.ip_word;
            const uint32_t* lw = reinterpret_cast<const uint32_t*>(P.links + T.link);
            Lk = make_uint3(lw[0], lw[1], lw[2]);
        }
        const uint32_t cnt = min(per, n - f0);
        const uint32_t sub = lane & (kTxSub - 1), q = lane / kTxSub;
        for (uint32_t t = 0; t < cnt; t += 64 / kTxSub) {  // quarter q copies frame t + q
            const uint32_t fr = t + q;
            const uint32_t sf = (uint32_t)__shfl((int)so, (int)fr);
            const uint32_t lf = (uint32_t)__shfl((int)plen, (int)fr);  // every lane shuffles, as above
            const uint32_t L = fr < cnt ? lf : 0u;
            uint8_t* pay = P.out + ((uint64_t)(f0 + fr) * P.stride + P.lead + 54u);
            const uint32_t s = tcp_tx_copy_sum(P.src + sf, pay, L, sub);
            const uint32_t le = (uint32_t)__shfl((int)s, (int)(((lane - t) & (64 / kTxSub - 1)) * kTxSub));
            if (!(live && lane >= t && lane < t + 64 / kTxSub)) continue;
            // the header arithmetic of dk_tcp_tx_emit_kernel
            const uint32_t tot = 40u + plen, seg = 20u + plen;
            const uint32_t ident = ipw & 0xFFFFu, ttl = (ipw >> 16) & 0xFFu, tos = ipw >> 24;
            const uint32_t ipsum = (0x4500u | tos) + tot + ident + 0x4000u + ((ttl << 8) | 6u) + ip_be_sum(src) + ip_be_sum(dst);
            const uint32_t ipc = csum_from_residue(mod_ffff(ipsum));
            const uint32_t sport = ports & 0xFFFFu, dport = ports >> 16;
            const uint32_t b12 = 5u << 4;
            uint32_t c = 0;
            if (!(P.flags & DK_TX_OFFLOAD_TCP)) {
                const uint32_t be = ip_be_sum(src) + ip_be_sum(dst) + 6u + seg + sport + dport + be16_sum(seq) +
                                    be16_sum(ack) + ((b12 << 8) | b13) + win;
                c = csum_from_residue(mod_ffff(be_residue(le) + be));
            }
            uint32_t d[14];
            d[0] = Lk.x;
            d[1] = Lk.y;
            d[2] = Lk.z;
            d[3] = 0x0008u | 0x45u << 16 | tos << 24;
            d[4] = bswap16(tot) | bswap16(ident) << 16;
            d[5] = 0x0040u | ttl << 16 | 6u << 24;
            d[6] = bswap16(ipc) | (src & 0xFFFFu) << 16;
            d[7] = (src >> 16) | (dst & 0xFFFFu) << 16;
            d[8] = (dst >> 16) | bswap16(sport) << 16;
            const uint32_t sq = __builtin_bswap32(seq), ak = __builtin_bswap32(ack);
            d[9] = bswap16(dport) | sq << 16;
            d[10] = (sq >> 16) | ak << 16;
            d[11] = (ak >> 16) | b12 << 16 | b13 << 24;
            d[12] = bswap16(win) | bswap16(c) << 16;
            d[13] = 0;
            tx_store_header(P.out + foff, d, true);
        }
    }
}

// Pure ACKs (dk_tcp_ack_emit and dk_tcp_ack_timer, dk_tcp.h): ControlBlock::send_ack's frame, the 54 header bytes of the
// kernels above with no payload behind them. Frame-major, one lane per frame: frame f belongs to the last item (a batch
// frame, or a connection) holding the scan value f, found by binary search as dk_tcp_rtx_emit_kernel finds its
// connection. seq = SND.NXT, flags ACK, ack = RCV.NXT as the item's moment left it, window = hdr_window_size() of that
// RCV.NXT (ctrlblk.rs:699-720, :786-803).
__global__ __launch_bounds__(kBlock) void dk_tcp_ack_emit_kernel(TcpAckEmitParams P) {
    const uint64_t total = *P.total;
    if (!tcp_tx_fits(total, P.max_frames, P.stride, P.out_bytes)) return;  // all or nothing, as the commit tests it
    for (uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x; f < total; f += (uint64_t)gridDim.x * kBlock) {
        uint32_t lo = 0, hi = P.nitems;  // the last item whose frame index is <= f
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (P.first[mid] <= f) lo = mid;
            else hi = mid;
        }
        const uint32_t item = lo, conn = P.item_conn ? P.item_conn[item] : item;
        const dk_tcp_tx_conn& T = P.tx[conn];
        const dk_tcp_conn& R = P.rx[conn];
        const uint32_t ack = P.item_ack ? P.item_ack[item] : R.receive_next;
        const uint32_t seq = T.snd_nxt, b13 = 0x10u;
        const uint32_t win = ((uint32_t)(R.buffer_size - (ack - R.reader_next)) >> (T.rcv_wscale & 31u)) & 0xFFFFu;
        const uint32_t foff = (uint32_t)(f * P.stride + P.lead);
        __builtin_nontemporal_store(foff, gptr(P.off_out) + f);
        __builtin_nontemporal_store((uint16_t)54u, gptr(P.len_out) + f);
        if (P.frame_conn) __builtin_nontemporal_store(conn, gptr(P.frame_conn) + f);
        if (P.frame_seg) __builtin_nontemporal_store(item, gptr(P.frame_seg) + f);
        const uint32_t src = T.local_ip, dst = T.remote_ip, ports = T.ports, ipw = T.ip_word;
        const uint32_t* lw = reinterpret_cast<const uint32_t*>(P.links + T.link);
        // the header arithmetic of dk_tcp_tx_emit_kernel with an empty payload
        const uint32_t tot = 40u, seg = 20u;
        const uint32_t ident = ipw & 0xFFFFu, ttl = (ipw >> 16) & 0xFFu, tos = ipw >> 24;
        const uint32_t ipsum = (0x4500u | tos) + tot + ident + 0x4000u + ((ttl << 8) | 6u) + ip_be_sum(src) + ip_be_sum(dst);
        const uint32_t ipc = csum_from_residue(mod_ffff(ipsum));
        const uint32_t sport = ports & 0xFFFFu, dport = ports >> 16;
        const uint32_t b12 = 5u << 4;
        uint32_t c = 0;
        if (!(P.flags & DK_TX_OFFLOAD_TCP)) {
            const uint32_t be = ip_be_sum(src) + ip_be_sum(dst) + 6u + seg + sport + dport + be16_sum(seq) +
                                be16_sum(ack) + ((b12 << 8) | b13) + win;
            c = csum_from_residue(mod_ffff(be_residue(0u) + be));  // the payload's sum is 0
        }
        uint32_t d[14];
        d[0] = lw[0];
        d[1] = lw[1];
        d[2] = lw[2];
        d[3] = 0x0008u | 0x45u << 16 | tos << 24;
        d[4] = bswap16(tot) | bswap16(ident) << 16;
        d[5] = 0x0040u | ttl << 16 | 6u << 24;
        d[6] = bswap16(ipc) | (src & 0xFFFFu) << 16;
        d[7] = (src >> 16) | (dst & 0xFFFFu) << 16;
        d[8] = (dst >> 16) | bswap16(sport) << 16;
        const uint32_t sq = __builtin_bswap32(seq), ak = __builtin_bswap32(ack);
        d[9] = bswap16(dport) | sq << 16;
        d[10] = (sq >> 16) | ak << 16;
        d[11] = (ak >> 16) | b12 << 16 | b13 << 24;
        d[12] = bswap16(win) | bswap16(c) << 16;
        d[13] = 0;
        tx_store_header(P.out + foff, d, true);
    }
}

}  // namespace
}  // namespace dk

int dk_tcp_tx_emit_resident_blocks() {
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, dk::dk_tcp_tx_emit_kernel, dk::kBlock, 0) != hipSuccess)
        return 0;
    return blocks;
}

int dk_launch_tcp_tx_emit(const dk::TcpTxEmitParams& p, uint32_t grid, void* stream) {
    if (p.nbufs == 0 || grid == 0) return 0;
    hipLaunchKernelGGL(dk::dk_tcp_tx_emit_kernel, dim3(grid), dim3(dk::kBlock), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 5;
}

int dk_launch_tcp_rtx_emit(const dk::TcpRtxEmitParams& p, uint32_t grid, void* stream) {
    if (p.nconns == 0 || grid == 0) return 0;
    hipLaunchKernelGGL(dk::dk_tcp_rtx_emit_kernel, dim3(grid), dim3(dk::kBlock), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 5;
}

int dk_launch_tcp_ack_emit(const dk::TcpAckEmitParams& p, uint32_t grid, void* stream) {
    if (p.nitems == 0 || grid == 0) return 0;
    hipLaunchKernelGGL(dk::dk_tcp_ack_emit_kernel, dim3(grid), dim3(dk::kBlock), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 5;
}
