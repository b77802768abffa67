// tcp_tx_kernels.hip — dk_tcp_tx_segment, dk_tcp_retransmit and dk_tcp_ack_timer (dk_tcp.h): the plan and commit kernels
// and the host entry points. The emit kernels (the payload copy, the checksums and the headers) are dk_tcp_tx_emit_kernel and
// dk_tcp_rtx_emit_kernel in tx_build_kernels.hip; they share their header arithmetic with dk_tx_serialize (frame_build.h).
//
// Sender::send_segment (tcp/established/sender.rs:124-208) cuts one segment at a time, each as large as
// min(send window - in flight, MSS, cwnd - in flight) allows. With no ACK arriving inside a call the windows are fixed,
// so a connection has one budget B = min(snd_wnd, cwnd) - in flight (0 by get_open_window_size_bytes' three tests, or
// when mss == 0), and the loop has a closed form: with C = the sequence space of the connection's earlier buffers
// (their lengths, an end-of-send marker counting 1), a buffer sends take = clamp(B - C, 0, len) bytes in ceil(take / mss)
// frames, a marker one frame iff B - C >= 1, and nothing behind the first marker. Everything is then a scan:
//   1. fill:   per buffer its sequence space, marker flag and range error; segment heads and tails by connection
//      scan:   exclusive sums over the whole push list (conn is non-decreasing, so a connection's C is the difference
//              to the sum at its head: no segmented scan is needed)
//   2. plan:   per buffer the connection checks, B, C, take, its frame count, the header's ack and window
//      scan:   exclusive sum of the frame counts = first_frame, its total = n_frames
//   3. emit    (tx_build_kernels.hip), and
//      commit: results per buffer; snd_nxt and fin_sent by the one buffer per connection that knows the total (the
//              first marker, else the connection's last buffer).
// Emit and commit both start with the same test of the total against max_frames / out_bytes, so a call that does not
// fit writes no frame and no connection, with no host round trip. The scans are three small kernels each (tile sums,
// one workgroup over the tile sums, tile scan): the push list is small next to the payload.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>

#include "../../include/dk_diag.h"
#include "../../include/dk_tcp.h"
#include "rx_common.h"
#include "tcp_order.h"

namespace dk_tcp_tx {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kItems = 4;                 // consecutive items per thread
constexpr uint32_t kTile = kBlock * kItems;    // items per workgroup of a scan
constexpr uint32_t kMaxMss = 65481;            // 54 + mss, the frame, must fit len_out / dk_rx_batch.len (16 bits)
constexpr uint32_t kCommit = 1u, kCommitFin = 2u;

struct Plan {
    const uint8_t* src;
    uint64_t src_bytes, out_bytes;
    const uint32_t* conn;
    const uint32_t* off;
    const uint32_t* len;
    uint32_t nbufs;
    dk_tcp_tx_conn* tx;
    const dk_tcp_conn* rx;
    uint32_t nconns, nlinks;
    uint32_t stride, lead, max_frames;
    uint64_t* seqsp;   // [nbufs] sequence space per buffer, then its exclusive scan
    uint64_t* flags;   // [nbufs] marker | range error << 32, then its exclusive scan
    uint64_t* frames;  // [nbufs] frame counts, then their exclusive scan
    uint64_t* tot;     // [0] sequence space, [1] flags, [2] frames
    uint32_t* head;    // [nconns] first and last buffer of each connection that has any
    uint32_t* tail;
    uint4* rec;        // [nbufs] take, seq of the first byte, ack, window (the emit kernel's)
    uint2* cm;         // [nbufs] kCommit* bits, the connection's new sequence space total
    dk_tcp_tx_results res;
};

__global__ __launch_bounds__(kBlock) void fill_kernel(Plan P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.nbufs) return;
    const uint32_t c = P.conn[i], o = P.off[i], l = P.len[i];
    P.seqsp[i] = l ? l : 1u;
    const uint64_t bad = (uint64_t)o + l > P.src_bytes;
    P.flags[i] = (l == 0 ? 1ull : 0ull) | bad << 32;
    if (c < P.nconns) {
        if (i == 0 || P.conn[i - 1] != c) P.head[c] = i;
        if (i + 1 == P.nbufs || P.conn[i + 1] != c) P.tail[c] = i;
    }
}

// Inclusive scan of one value per thread over the workgroup; `total` = the workgroup's sum.
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t& total) {
    __shared__ uint64_t s_w[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t u = __shfl_up(v, o);
        if (lane >= (uint32_t)o) v += u;
    }
    __syncthreads();  // s_w may still be read from a previous call
    if (lane == 63) s_w[wv] = v;
    __syncthreads();
    uint64_t base = 0;
    total = 0;
    for (uint32_t k = 0; k < kBlock / 64; k++) {
        if (k < wv) base += s_w[k];
        total += s_w[k];
    }
    return v + base;
}

// Sums of each tile of nq arrays a[q * n .. ) -> bsum[q * nb + tile].
__global__ __launch_bounds__(kBlock) void scan_sums_kernel(const uint64_t* a0, const uint64_t* a1, uint32_t n,
                                                           uint64_t* bsum, uint32_t nb) {
    const uint64_t base = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kItems;
    for (uint32_t q = 0; q < 2; q++) {
        const uint64_t* a = q ? a1 : a0;
        if (!a) continue;
        uint64_t v = 0;
        for (uint32_t k = 0; k < kItems; k++)
            if (base + k < n) v += a[base + k];
        uint64_t total;
        block_scan(v, total);
        if (threadIdx.x == 0) bsum[(size_t)q * nb + blockIdx.x] = total;
    }
}

// One workgroup: exclusive scan of the tile sums in place, the grand totals to tot0 / tot1.
__global__ __launch_bounds__(kBlock) void scan_spine_kernel(uint64_t* bsum, uint32_t nb, bool two, uint64_t* tot0,
                                                            uint64_t* tot1) {
    for (uint32_t q = 0; q < (two ? 2u : 1u); q++) {
        uint64_t* b = bsum + (size_t)q * nb;
        uint64_t carry = 0;
        for (uint32_t k0 = 0; k0 < nb; k0 += kBlock) {
            const uint32_t k = k0 + threadIdx.x;
            const uint64_t v = k < nb ? b[k] : 0;
            uint64_t total;
            const uint64_t inc = block_scan(v, total);
            if (k < nb) b[k] = carry + inc - v;
            carry += total;
        }
        if (threadIdx.x == 0) *(q ? tot1 : tot0) = carry;
    }
}

// Exclusive scan of each tile in place, offset by its scanned tile sum.
__global__ __launch_bounds__(kBlock) void scan_tiles_kernel(uint64_t* a0, uint64_t* a1, uint32_t n, const uint64_t* bsum,
                                                            uint32_t nb) {
    const uint64_t base = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kItems;
    for (uint32_t q = 0; q < 2; q++) {
        uint64_t* a = q ? a1 : a0;
        if (!a) continue;
        uint64_t x[kItems], v = 0;
        for (uint32_t k = 0; k < kItems; k++) {
            x[k] = base + k < n ? a[base + k] : 0;
            v += x[k];
        }
        uint64_t total;
        uint64_t run = block_scan(v, total) - v + bsum[(size_t)q * nb + blockIdx.x];
        for (uint32_t k = 0; k < kItems; k++) {
            if (base + k < n) a[base + k] = run;
            run += x[k];
        }
    }
}

__global__ __launch_bounds__(kBlock) void plan_kernel(Plan P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.nbufs) return;
    const uint32_t c = P.conn[i], len = P.len[i];
    uint32_t take = 0, nfr = 0, seq0 = 0, ack = 0, win = 0, st = DK_TCP_TX_E_CONN, commit = 0, newtot = 0;
    if (c < P.nconns) {
        const dk_tcp_tx_conn T = P.tx[c];
        const uint32_t h = P.head[c], t = P.tail[c];
        const uint64_t fh = P.flags[h], fi = P.flags[i];
        const uint64_t fend = t + 1 < P.nbufs ? P.flags[t + 1] : P.tot[1];  // inclusive at the connection's last buffer
        const bool range_bad = (fend >> 32) != (fh >> 32);
        uint64_t w = T.rcv_wnd_hdr;
        ack = T.rcv_nxt;
        if (P.rx) {  // ControlBlock::tcp_header: RCV.NXT and hdr_window_size (ctrlblk.rs:699-709, :786-803)
            const dk_tcp_conn& R = P.rx[c];
            const uint32_t rn = R.receive_next;
            ack = rn;
            const uint32_t ws = T.rcv_wscale;
            w = ws > 31 ? 0u : (uint32_t)(R.buffer_size - (rn - R.reader_next)) >> ws;
        }
        const bool ok = T.state == DK_TCP_ESTABLISHED && w <= 0xFFFFu && T.link < P.nlinks && T.mss <= kMaxMss &&
                        (uint64_t)P.lead + 54u + T.mss <= P.stride && !range_bad;
        if (ok) {
            win = (uint32_t)w;
            const uint32_t inflight = T.snd_nxt - T.snd_una;
            const uint32_t B = (T.snd_wnd == 0 || T.snd_wnd < inflight || T.cwnd < inflight || T.mss == 0)
                                   ? 0u : min(T.snd_wnd, T.cwnd) - inflight;
            const uint64_t C = P.seqsp[i] - P.seqsp[h];
            const uint32_t markers_before = (uint32_t)fi - (uint32_t)fh;
            const bool closed = T.fin_sent || markers_before;
            const uint32_t rem = B > C ? (uint32_t)(B - C) : 0u;
            seq0 = T.snd_nxt + (uint32_t)C;
            if (closed) {
                st = DK_TCP_TX_CLOSED;
            } else if (len == 0) {
                nfr = rem >= 1;
                st = nfr ? DK_TCP_TX_SENT : DK_TCP_TX_UNSENT;
            } else {
                take = min(rem, len);
                nfr = (take + T.mss - 1) / max(T.mss, 1u);  // take > 0 only with mss > 0
                if (take == 0) nfr = 0;
                st = take == len ? DK_TCP_TX_SENT : take ? DK_TCP_TX_PARTIAL : DK_TCP_TX_UNSENT;
            }
            // One buffer commits the connection: the first marker, else the last buffer. The sequence space sent up to
            // and including it is min(B, C + its own).
            const bool any_marker = (uint32_t)fend != (uint32_t)fh;
            if (!T.fin_sent && ((len == 0 && !markers_before) || (i == t && !any_marker))) {
                const uint64_t upto = C + (len ? len : 1u);
                newtot = (uint32_t)(B < upto ? B : upto);
                commit = kCommit | (len == 0 && nfr ? kCommitFin : 0u);
            }
        }
    }
    P.frames[i] = nfr;
    P.rec[i] = make_uint4(take, seq0, ack, win);
    P.cm[i] = make_uint2(commit | st << 8, newtot);
}

__global__ __launch_bounds__(kBlock) void commit_kernel(Plan P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.nbufs) return;
    const uint64_t total = P.tot[2];
    const bool fits = dk::tcp_tx_fits(total, P.max_frames, P.stride, P.out_bytes);
    if (i == 0) *P.res.n_frames = (uint32_t)min(total, (uint64_t)0xFFFFFFFFu);
    const uint64_t first = P.frames[i];
    const uint64_t next = i + 1 < P.nbufs ? P.frames[i + 1] : total;
    const uint32_t count = (uint32_t)min(next - first, (uint64_t)0xFFFFFFFFu);
    const uint2 cm = P.cm[i];
    const uint4 r = P.rec[i];
    uint32_t st = cm.x >> 8;
    uint32_t sent = P.len[i] ? r.x : (count ? 1u : 0u);
    if (!fits) {
        sent = 0;
        if (count) st = DK_TCP_TX_NO_ROOM;
    }
    P.res.sent[i] = sent;
    P.res.first_frame[i] = (uint32_t)min(first, (uint64_t)0xFFFFFFFFu);
    P.res.frame_count[i] = count;
    P.res.status[i] = st;
    if (fits && (cm.x & kCommit)) {
        dk_tcp_tx_conn& T = P.tx[P.conn[i]];
        T.snd_nxt += cm.y;
        if (cm.x & kCommitFin) T.fin_sent = 1;
    }
}

// dk_tcp_retransmit (dk_tcp.h): one lane per connection plans (the checks in the header's order, emit 0/1, the front
// entry and the header fields as a record), the scan above numbers the frames, dk_tcp_rtx_emit_kernel
// (tx_build_kernels.hip) builds them, and one lane per connection commits behind the same capacity test.
struct RtxPlan {
    uint64_t src_bytes, out_bytes, now_ns;
    const uint8_t* fire;
    const dk_tcp_tx_conn* tx;
    dk_tcp_ack_conn* ak;
    const dk_tcp_conn* rx;
    dk_tcp_unacked q;
    uint32_t nconns, nq, nlinks;
    uint32_t stride, lead, max_frames;
    uint64_t* emit;  // [nconns] emit flags, then their exclusive scan
    uint64_t* tot;   // the frames the call needs
    uint4* rec;      // [nconns] the front's off, len | window << 16, seq, ack number (the emit kernel's)
    dk_tcp_rtx_results res;
};

__global__ __launch_bounds__(kBlock) void rtx_plan(RtxPlan P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= P.nconns) return;
    const uint32_t fire = P.fire[c];
    uint32_t st = DK_TCP_RTX_NOT_FIRED;
    uint4 rec = make_uint4(0, 0, 0, 0);
    if (fire > DK_TCP_RTX_FAST) {
        st = DK_TCP_RTX_E_FIRE;
    } else if (fire) {
        const dk_tcp_tx_conn T = P.tx[c];
        const dk_tcp_ack_conn& A = P.ak[c];
        const uint32_t qf = A.q_first, qc = A.q_count;
        uint64_t w = T.rcv_wnd_hdr;
        uint32_t ack = T.rcv_nxt;
        if (P.rx) {  // as plan_kernel: RCV.NXT and hdr_window_size
            const dk_tcp_conn& R = P.rx[c];
            const uint32_t rn = R.receive_next;
            ack = rn;
            const uint32_t ws = T.rcv_wscale;
            w = ws > 31 ? 0u : (uint32_t)(R.buffer_size - (rn - R.reader_next)) >> ws;
        }
        if (T.state != DK_TCP_ESTABLISHED) st = DK_TCP_RTX_E_STATE;
        else if ((uint64_t)qf + qc > P.nq) st = DK_TCP_RTX_E_QUEUE;
        else if (T.link >= P.nlinks) st = DK_TCP_RTX_E_LINK;
        else if (w > 0xFFFFu) st = DK_TCP_RTX_E_WINDOW;
        else if (qc == 0 || (fire == DK_TCP_RTX_TIMEOUT && !A.rtx_armed)) st = DK_TCP_RTX_IDLE;
        else {
            const uint32_t off = P.q.off[qf], len = P.q.len[qf];
            if ((uint64_t)off + len > P.src_bytes) st = DK_TCP_RTX_E_RANGE;
            else if (len > kMaxMss || (uint64_t)P.lead + 54u + len > P.stride) st = DK_TCP_RTX_E_SLOT;
            else {
                st = DK_TCP_RTX_SENT;
                rec = make_uint4(off, len | (uint32_t)w << 16, T.snd_una, ack);
            }
        }
    }
    P.emit[c] = st == DK_TCP_RTX_SENT;
    P.rec[c] = rec;
    P.res.status[c] = st;  // SENT stands unless rtx_commit finds no room
}

__global__ __launch_bounds__(kBlock) void rtx_commit(RtxPlan P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= P.nconns) return;
    const uint64_t total = P.tot[0];
    const bool fits = dk::tcp_tx_fits(total, P.max_frames, P.stride, P.out_bytes);
    if (c == 0) *P.res.n_frames = (uint32_t)total;  // at most nconns
    const uint64_t first = P.emit[c];
    const bool emits = (c + 1 < P.nconns ? P.emit[c + 1] : total) != first;
    P.res.frame[c] = emits && fits ? (uint32_t)first : 0xFFFFFFFFu;
    if (!emits) return;
    if (!fits) {
        P.res.status[c] = DK_TCP_RTX_NO_ROOM;
        return;
    }
    dk_tcp_ack_conn& A = P.ak[c];
    P.q.tx_time[A.q_first] = DK_TCP_TX_TIME_NONE;  // Karn: no sample from a retransmitted entry
    if (P.fire[c] == DK_TCP_RTX_TIMEOUT) {
        double r = A.rto * 2.0;  // RtoCalculator::back_off -> update_rto's clamp
        if (r < 0.1) r = 0.1;
        if (r > 60.0) r = 60.0;
        A.rto = r;
        A.rtx_base_ns = P.now_ns;
        A.rtx_armed = 1;
    }
}

// dk_tcp_ack_timer (dk_tcp.h): the acknowledger's expiry, with dk_tcp_retransmit's shape. One lane per connection
// plans (the checks in the header's order, emit 0/1), the scan numbers the frames, dk_tcp_ack_emit_kernel
// (tx_build_kernels.hip) builds them from the tables as they stand, and one lane per connection commits behind the
// same capacity test.
struct AckTimerPlan {
    uint64_t out_bytes;
    const uint8_t* fire;
    const dk_tcp_tx_conn* tx;
    const dk_tcp_conn* rx;
    dk_tcp_dack_conn* dack;
    uint32_t nconns, nlinks;
    uint32_t stride, lead, max_frames;
    uint64_t* emit;  // [nconns] emit flags, then their exclusive scan
    uint64_t* tot;   // the frames the call needs
    dk_tcp_ackemit_results res;
};

__global__ __launch_bounds__(kBlock) void ack_timer_plan(AckTimerPlan P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= P.nconns) return;
    uint32_t st = DK_TCP_ACKEMIT_NOT_FIRED;
    if (P.fire[c]) {
        st = dk::tcp_ackemit_check(P.tx[c], P.rx[c], P.nlinks, P.stride, P.lead);
        if (st == DK_TCP_ACKEMIT_OK && !P.dack[c].armed) st = DK_TCP_ACKEMIT_IDLE;
    }
    P.emit[c] = st == DK_TCP_ACKEMIT_OK;
    P.res.status[c] = st;  // OK stands unless ack_timer_commit finds no room
}

__global__ __launch_bounds__(kBlock) void ack_timer_commit(AckTimerPlan P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= P.nconns) return;
    const uint64_t total = P.tot[0];
    const bool fits = dk::tcp_tx_fits(total, P.max_frames, P.stride, P.out_bytes);
    if (c == 0) *P.res.n_frames = (uint32_t)total;  // at most nconns
    const uint64_t first = P.emit[c];
    const bool emits = (c + 1 < P.nconns ? P.emit[c + 1] : total) != first;
    P.res.ack_frame[c] = emits && fits ? (uint32_t)first : 0xFFFFFFFFu;
    P.res.n_acks[c] = emits;
    if (!emits) return;
    if (!fits) {
        P.res.status[c] = DK_TCP_ACKEMIT_NO_ROOM;
        return;
    }
    P.dack[c].armed = 0;  // emit() clears the deadline (ctrlblk.rs:761); deadline_ns is left as it is
}

using dk::ctl::DeviceGuard;

std::atomic<int32_t> g_emit_grid{-1};  // dk_diag_tcp_tx_set_grid

// Exclusive scans of a0 (and a1) in place, totals to tot0 (tot1).
int scan(uint64_t* a0, uint64_t* a1, uint32_t n, uint64_t* bsum, uint32_t nb, uint64_t* tot0, uint64_t* tot1,
         hipStream_t s) {
    hipLaunchKernelGGL(scan_sums_kernel, dim3(nb), dim3(kBlock), 0, s, a0, a1, n, bsum, nb);
    hipLaunchKernelGGL(scan_spine_kernel, dim3(1), dim3(kBlock), 0, s, bsum, nb, a1 != nullptr, tot0, tot1);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(nb), dim3(kBlock), 0, s, a0, a1, n, bsum, nb);
    return hipGetLastError() == hipSuccess ? 0 : EIO;
}

}  // namespace
}  // namespace dk_tcp_tx

// One scratch set per context; calls are serialised on it as dk_tcp_ctx's are (a call on another stream than the
// previous one first waits, on the device, for the previous call's work).
struct dk_tcp_tx_ctx {
    int device = 0;
    dk::ctl::CallOrder serial;
    uint32_t cus = 0, occ = 0;
    dk::ctl::Buf<uint64_t> seqsp, flags, frames, bsum, tot;
    dk::ctl::Buf<uint32_t> head, tail;
    dk::ctl::Buf<uint4> rec;
    dk::ctl::Buf<uint2> cm;
    // dk_tcp_retransmit's: the emit flags / their scan and the records per connection (tot[3] is its total)
    dk::ctl::Buf<uint64_t> rtx_emit;
    dk::ctl::Buf<uint4> rtx_rec;
    // dk_tcp_ack_timer's emit flags / their scan per connection (tot[4] is its total)
    dk::ctl::Buf<uint64_t> ackt_emit;
    // dk_tcp_tx_commit's turn after dk_tcp_tx_segment, its form and its scratch (tcp_commit_kernels.hip)
    dk_tcp_commit_state commit;
};

int dk_tcp_tx_ctx_serial(dk_tcp_tx_ctx* t, dk_tcp_tx_serial* o) {
    if (!t || !o) return EINVAL;
    *o = dk_tcp_tx_serial{t->device, &t->serial, t->cus, &t->commit};
    return 0;
}

uint32_t dk_tcp_tx_scan_tiles(uint32_t n) { return (n + dk_tcp_tx::kTile - 1) / dk_tcp_tx::kTile; }

int dk_tcp_tx_scan(uint64_t* a, uint32_t n, uint64_t* bsum, uint64_t* tot, void* stream) {
    return dk_tcp_tx::scan(a, nullptr, n, bsum, dk_tcp_tx_scan_tiles(n), tot, nullptr, (hipStream_t)stream);
}

extern "C" {

int dk_diag_tcp_tx_set_grid(int32_t grid) {
    dk_tcp_tx::g_emit_grid = grid;
    return 0;
}

int dk_tcp_tx_ctx_create(int32_t device, dk_tcp_tx_ctx** out) {
    if (!out) return EINVAL;
    *out = nullptr;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return EINVAL;
    dk_tcp_tx::DeviceGuard g(device);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        return EINVAL;
    dk_tcp_tx_ctx* t = new dk_tcp_tx_ctx();
    t->device = device;
    t->cus = (uint32_t)cus;
    t->occ = (uint32_t)std::max(dk_tcp_tx_emit_resident_blocks(), 1);
    if (hipEventCreateWithFlags(&t->serial.last, hipEventDisableTiming) != hipSuccess) {
        delete t;
        return EINVAL;
    }
    if (t->tot.grow(t->serial, 5)) {
        (void)hipEventDestroy(t->serial.last);
        delete t;
        return ENOMEM;
    }
    *out = t;
    return 0;
}

void dk_tcp_tx_ctx_destroy(dk_tcp_tx_ctx* t) {
    if (!t) return;
    dk_tcp_tx::DeviceGuard g(t->device);
    (void)t->serial.drain();
    dk::ctl::free_all(t->seqsp, t->flags, t->frames, t->bsum, t->tot, t->head, t->tail, t->rec, t->cm, t->rtx_emit,
                      t->rtx_rec, t->ackt_emit, t->commit.scratch);
    (void)hipEventDestroy(t->serial.last);
    delete t;
}

uint64_t dk_tcp_tx_frame_bound(const uint32_t* len, uint32_t nbufs, uint32_t mss) {
    if (!len || mss == 0) return 0;
    uint64_t total = 0;
    for (uint32_t i = 0; i < nbufs; i++) total += std::max<uint64_t>(1, ((uint64_t)len[i] + mss - 1) / mss);
    return total;
}

int dk_tcp_tx_segment(dk_tcp_tx_ctx* t, const uint8_t* src, uint64_t src_bytes, const dk_tcp_tx_push* push,
                      uint32_t nbufs, dk_tcp_tx_conn* tx_conns, uint32_t nconns, const dk_tcp_conn* rx_conns,
                      const dk_tx_link* links, uint32_t nlinks, uint8_t* out, uint64_t out_bytes,
                      const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t flags,
                      const dk_tcp_tx_results* res, void* stream) {
    using namespace dk_tcp_tx;
    if (!t || !push || !layout || !res || !res->n_frames) return EINVAL;
    if (src_bytes > DK_RX_MAX_BLOB || out_bytes > DK_RX_MAX_BLOB) return EINVAL;
    if (reinterpret_cast<uintptr_t>(tx_conns) & 15) return EINVAL;
    if (nbufs && (!push->conn || !push->off || !push->len || !res->sent || !res->first_frame || !res->frame_count ||
                  !res->status || !links || nlinks == 0 || (nconns && !tx_conns) || (src_bytes && !src)))
        return EINVAL;
    if (nbufs && max_frames && (!out || !res->off_out || !res->len_out)) return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    if (t->serial.order(s)) return EIO;
    if (nbufs == 0) {
        if (hipMemsetAsync(res->n_frames, 0, sizeof(uint32_t), s) != hipSuccess) return EIO;
    } else {
        const uint32_t nb = (nbufs + kTile - 1) / kTile;
        dk::ctl::CallOrder& o = t->serial;
        int rc = 0;
        if ((rc = t->seqsp.grow(o, nbufs)) || (rc = t->flags.grow(o, nbufs)) || (rc = t->frames.grow(o, nbufs)) ||
            (rc = t->bsum.grow(o, 2 * (size_t)nb)) || (rc = t->head.grow(o, nconns)) || (rc = t->tail.grow(o, nconns)) ||
            (rc = t->rec.grow(o, nbufs)) || (rc = t->cm.grow(o, nbufs)))
            return rc;
        Plan P{src, src_bytes, out_bytes, push->conn, push->off, push->len, nbufs, tx_conns, rx_conns, nconns, nlinks,
               layout->slot_stride, layout->frame_lead, max_frames, t->seqsp.p, t->flags.p, t->frames.p, t->tot.p,
               t->head.p, t->tail.p, t->rec.p, t->cm.p, *res};
        const dim3 per_buf((nbufs + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(fill_kernel, per_buf, dim3(kBlock), 0, s, P);
        if ((rc = scan(t->seqsp.p, t->flags.p, nbufs, t->bsum.p, nb, t->tot.p + 0, t->tot.p + 1, s))) return rc;
        hipLaunchKernelGGL(plan_kernel, per_buf, dim3(kBlock), 0, s, P);
        if ((rc = scan(t->frames.p, nullptr, nbufs, t->bsum.p, nb, t->tot.p + 2, nullptr, s))) return rc;
        // emit reads the connections the commit updates (never snd_nxt or fin_sent), and runs first
        dk::TcpTxEmitParams E{src, out, out_bytes, push->conn, push->off, push->len, nbufs, tx_conns, links, t->frames.p,
                              t->tot.p + 2, reinterpret_cast<const uint32_t*>(t->rec.p), layout->slot_stride,
                              layout->frame_lead, max_frames, flags, res->off_out, res->len_out, res->frame_buf};
        // the persistent grid is sized from what the host knows: the frames the outputs have room for
        // (a workgroup's four waves take 256 frames a round)
        uint32_t grid = std::min<uint32_t>(max_frames / 256 + 1, std::min(t->occ, 8u) * t->cus);
        const int32_t cap = g_emit_grid;
        if (cap > 0) grid = std::min(grid, (uint32_t)cap);
        if (max_frames && (rc = dk_launch_tcp_tx_emit(E, grid, s))) return EIO;
        hipLaunchKernelGGL(commit_kernel, per_buf, dim3(kBlock), 0, s, P);
    }
    if (t->serial.record(s)) return EIO;
    if (++t->commit.seg_call == 0) t->commit.seg_call = 1;  // dk_tcp_tx_commit's turn; 0 stays "no call yet"
    t->commit.seg_nbufs = nbufs;
    return 0;
}

int dk_tcp_retransmit(dk_tcp_tx_ctx* t, const uint8_t* src, uint64_t src_bytes, const uint8_t* fire,
                      const dk_tcp_tx_conn* tx_conns, dk_tcp_ack_conn* ack_conns, uint32_t nconns,
                      const dk_tcp_conn* rx_conns, const dk_tcp_unacked* q, uint32_t nq, uint64_t now_ns,
                      const dk_tx_link* links, uint32_t nlinks, uint8_t* out, uint64_t out_bytes,
                      const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t flags,
                      const dk_tcp_rtx_results* res, void* stream) {
    using namespace dk_tcp_tx;
    if (!t || !layout || !res || !res->n_frames || !q || !links || nlinks == 0) return EINVAL;
    if (src_bytes > DK_RX_MAX_BLOB || out_bytes > DK_RX_MAX_BLOB) return EINVAL;
    if ((reinterpret_cast<uintptr_t>(tx_conns) | reinterpret_cast<uintptr_t>(ack_conns) |
         reinterpret_cast<uintptr_t>(rx_conns)) & 15)
        return EINVAL;
    if (nconns && (!fire || !tx_conns || !ack_conns || !res->status || !res->frame || (src_bytes && !src) ||
                   (nq && (!q->off || !q->len || !q->tx_time))))
        return EINVAL;
    if (nconns && max_frames && (!out || !res->off_out || !res->len_out)) return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    if (t->serial.order(s)) return EIO;
    if (nconns == 0) {
        if (hipMemsetAsync(res->n_frames, 0, sizeof(uint32_t), s) != hipSuccess) return EIO;
    } else {
        const uint32_t nb = (nconns + kTile - 1) / kTile;
        int rc = 0;
        if ((rc = t->rtx_emit.grow(t->serial, nconns)) || (rc = t->rtx_rec.grow(t->serial, nconns)) ||
            (rc = t->bsum.grow(t->serial, nb)))
            return rc;
        RtxPlan P{src_bytes, out_bytes, now_ns, fire, tx_conns, ack_conns, rx_conns, *q, nconns, nq, nlinks,
                  layout->slot_stride, layout->frame_lead, max_frames, t->rtx_emit.p, t->tot.p + 3, t->rtx_rec.p, *res};
        const dim3 per_conn((nconns + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(rtx_plan, per_conn, dim3(kBlock), 0, s, P);
        if ((rc = scan(t->rtx_emit.p, nullptr, nconns, t->bsum.p, nb, t->tot.p + 3, nullptr, s))) return rc;
        // emit reads the records, never the rows the commit writes, and runs first
        dk::TcpRtxEmitParams E{src, out, out_bytes, tx_conns, links, t->rtx_emit.p, t->tot.p + 3,
                               reinterpret_cast<const uint32_t*>(t->rtx_rec.p), nconns, layout->slot_stride,
                               layout->frame_lead, max_frames, flags, res->off_out, res->len_out, res->frame_conn};
        // sized from what the host knows: a frame per connection at most, and no more than the outputs have room for
        const uint32_t grid = std::min<uint32_t>(std::min(max_frames, nconns) / 256 + 1, std::min(t->occ, 8u) * t->cus);
        if (max_frames && dk_launch_tcp_rtx_emit(E, grid, s)) return EIO;
        hipLaunchKernelGGL(rtx_commit, per_conn, dim3(kBlock), 0, s, P);
    }
    return t->serial.record(s);
}

int dk_tcp_ack_timer(dk_tcp_tx_ctx* t, const uint8_t* fire, const dk_tcp_tx_conn* tx_conns, const dk_tcp_conn* rx_conns,
                     dk_tcp_dack_conn* dack, uint32_t nconns, const dk_tx_link* links, uint32_t nlinks, uint8_t* out,
                     uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t flags,
                     const dk_tcp_ackemit_results* res, void* stream) {
    using namespace dk_tcp_tx;
    if (!t || !layout || !res || !res->n_frames || !links || nlinks == 0) return EINVAL;
    if (out_bytes > DK_RX_MAX_BLOB) return EINVAL;
    if ((reinterpret_cast<uintptr_t>(tx_conns) | reinterpret_cast<uintptr_t>(rx_conns) |
         reinterpret_cast<uintptr_t>(dack)) & 15)
        return EINVAL;
    if (nconns && (!fire || !tx_conns || !rx_conns || !dack || !res->status || !res->n_acks || !res->ack_frame))
        return EINVAL;
    if (nconns && max_frames && (!out || !res->off_out || !res->len_out)) return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    if (t->serial.order(s)) return EIO;
    if (nconns == 0) {
        if (hipMemsetAsync(res->n_frames, 0, sizeof(uint32_t), s) != hipSuccess) return EIO;
    } else {
        const uint32_t nb = (nconns + kTile - 1) / kTile;
        int rc = 0;
        if ((rc = t->ackt_emit.grow(t->serial, nconns)) || (rc = t->bsum.grow(t->serial, nb))) return rc;
        AckTimerPlan P{out_bytes, fire, tx_conns, rx_conns, dack, nconns, nlinks, layout->slot_stride, layout->frame_lead,
                       max_frames, t->ackt_emit.p, t->tot.p + 4, *res};
        const dim3 per_conn((nconns + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(ack_timer_plan, per_conn, dim3(kBlock), 0, s, P);
        if ((rc = scan(t->ackt_emit.p, nullptr, nconns, t->bsum.p, nb, t->tot.p + 4, nullptr, s))) return rc;
        // emit reads the tables, never the rows the commit writes, and runs first
        dk::TcpAckEmitParams E{out, out_bytes, tx_conns, rx_conns, links, t->ackt_emit.p, t->tot.p + 4, nullptr, nullptr,
                               nconns, layout->slot_stride, layout->frame_lead, max_frames, flags, res->off_out,
                               res->len_out, res->frame_conn, nullptr};
        const uint32_t grid = std::min<uint32_t>(std::min(max_frames, nconns) / 256 + 1, 8u * t->cus);
        if (max_frames && dk_launch_tcp_ack_emit(E, grid, s)) return EIO;
        hipLaunchKernelGGL(ack_timer_commit, per_conn, dim3(kBlock), 0, s, P);
    }
    return t->serial.record(s);
}

}  // extern "C"
