// tcp_ackemit_kernels.hip — the receiver's ACKs on the GPU (include/dk_tcp.h, dk_tcp_ack_emit; dk_tcp_ack_timer's
// kernels sit with dk_tcp_retransmit's in tcp_tx_kernels.hip, the frame builder both share is dk_tcp_ack_emit_kernel in
// tx_build_kernels.hip).
//
// ControlBlock::process_packet (ctrlblk.rs:403-440) decides per segment whether an ACK goes out and what becomes of the
// delayed-ACK deadline; send_ack (:712-720) puts RCV.NXT and the window of that moment into it. dk_tcp_rx_process left
// each segment's action and view and, in its context, the batch's order by connection (tcp_order.h); its kernels are
// not touched. What a row of dk_tcp.h's table does to `armed` is one of four maps on a bit (identity, toggle, set,
// clear), and RCV.NXT moves only at DELIVERED / FIN segments, which start exactly at RCV.NXT once trimmed, so RCV.NXT
// after a segment is the trimmed start of the connection's next DELIVERED / FIN segment (the table's receive_next
// behind the last). The pass:
//   1. ackemit_conn_kernel: the connection checks, per-connection outputs zeroed.
//   2. ackemit_merge_kernel: the connection's walked segments and the strays the key kernel classified early sit apart
//      in the order (range[2c] .. range[2c + 1] .. range[2c + 2]), each part in arrival order; every element finds its
//      rank in the other part by binary search, which merges them by frame index.
//   3. the walk over each connection's merged segments, in one of two forms with identical results:
//        ackemit_lane_kernel: one lane per connection, backward for RCV.NXT, forward for `armed`: the table, literally;
//        the scan form: the maps compose and "the next DELIVERED / FIN start" is a first-valid suffix, so both are
//        scans over the whole merged order at once (tile aggregates, one workgroup over the tiles, tile scan). A
//        connection's first element is composed with the constant map of its initial `armed` and its last one closes
//        the suffix with the table's receive_next: constants absorb whatever lies beyond them, so no segmented scan is
//        needed.
//      Either leaves, per batch frame, an emit flag and the ACK's RCV.NXT, per connection n_acks and the new `armed`.
//   4. the exclusive scan of the flags in frame order (tcp_tx_kernels.hip's) numbers the ACKs by the frames that
//      triggered them; dk_tcp_ack_emit_kernel builds them frame-major; ackemit_finish_kernel writes ack_frame and, behind
//      the same capacity test, the dack rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>

#include "../../include/dk_diag.h"
#include "../../include/dk_tcp.h"
#include "ctl_common.h"
#include "tcp_order.h"

namespace dk_tcp_ackemit {
namespace {

constexpr uint32_t kBlock = 256, kWave = 64, kWaves = kBlock / kWave;
constexpr uint32_t kItems = 4, kTile = kBlock * kItems;
constexpr uint32_t kNoConn = 0xFFFFFFFFu;
constexpr uint32_t kScanMinSegs = 8;  // the scan form from this many segments per connection
// what a segment does (dk_tcp.h's table): nothing; ACK if armed, armed toggles; ACK, armed = 1; ACK, armed = 0
constexpr uint32_t kNothing = 0, kToggle = 1, kSet = 2, kClear = 3;
// a map on one bit as f(0) | f(1) << 1
constexpr uint32_t kIdentity = 2;
// pend[c]: the connection's row as the finish kernel commits it
constexpr uint32_t kTouched = 1, kArmedOnce = 2, kArmedLast = 4;

struct Params {
    const uint32_t* svals;
    const uint32_t* range;
    const uint4* rec;
    const uint8_t* action;
    const dk_tcp_view* view;
    const dk_tcp_conn* rx;
    const dk_tcp_tx_conn* tx;
    dk_tcp_dack_conn* dack;
    uint32_t n, nconns, nlinks;
    uint32_t stride, lead, max_frames;
    uint64_t out_bytes, now;
    uint32_t* morder;  // [n] the batch's frames by connection, each connection's in arrival order
    uint32_t* mconn;   // [n] the element's connection, kNoConn behind the last connection's
    uint32_t* ackno;   // [n] by frame: RCV.NXT as the frame's ACK carries it (where flag is set)
    uint64_t* flag;    // [n] by frame: 1 = an ACK, then their exclusive scan
    uint64_t* esum;    // [n] by element: trimmed start | (kind | DELIVERED / FIN << 2) << 32 (the scan form)
    uint32_t* tile_m;  // [tiles] each tile's composed map, then the composition of the tiles before it
    uint64_t* tile_v;  // [tiles] each tile's first DELIVERED / FIN start | 1 << 32, then that of the tiles behind it
    uint32_t* pend;    // [nconns] kTouched | kArmedOnce | kArmedLast
    uint64_t* tot;     // the frames the call needs
    dk_tcp_ackemit_results res;
};

__device__ __forceinline__ uint32_t apply(uint32_t map, uint32_t bit) { return (map >> bit) & 1u; }
// f first, then g
__device__ __forceinline__ uint32_t compose(uint32_t f, uint32_t g) { return apply(g, f & 1u) | apply(g, f >> 1) << 1; }
__device__ __forceinline__ uint32_t map_of(uint32_t kind) {
    return kind == kNothing ? kIdentity : kind == kToggle ? 1u : kind == kSet ? 3u : 0u;
}

struct Elem {
    uint32_t kind;
    bool moves;       // DELIVERED or FIN: RCV.NXT stood at `start` before it
    uint32_t start;
};

// Frame i's row of the table, and where RCV.NXT stood before it if it moved it.
__device__ __forceinline__ Elem load_elem(const Params& P, uint32_t i) {
    const uint32_t act = P.action[i];
    Elem e{kNothing, false, 0u};
    if (act == DK_TCP_SKIP || act == DK_TCP_UNPROCESSED || act == DK_TCP_RST || act == DK_TCP_SYN || act == DK_TCP_NO_ACK)
        return e;
    const uint4 g = P.rec[i];  // {seq, ack, meta, payload}
    const uint32_t flags = (g.z >> 16) & 0xFFu;
    if (act == DK_TCP_DELIVERED || act == DK_TCP_NO_DATA) e.kind = kToggle;
    else if (act == DK_TCP_STORED || act == DK_TCP_STORE_DUP) e.kind = kSet;
    else if (act == DK_TCP_FIN || act == DK_TCP_ACK_UNSENT) e.kind = kClear;
    else if (act == DK_TCP_DUPLICATE || act == DK_TCP_OUT_OF_WINDOW) e.kind = (flags & 0x04u) ? kNothing : kClear;
    if (act == DK_TCP_DELIVERED || act == DK_TCP_FIN) {
        // check_segment_in_window's front trim (ctrlblk.rs:476-493): the view's offset moved by the old bytes, a SYN
        // that survives to here was trimmed with them and took one sequence number
        e.moves = true;
        e.start = g.x + (P.view[i].off - (g.w & 0xFFFFu)) + ((flags >> 1) & 1u);
    }
    return e;
}

__global__ __launch_bounds__(kBlock) void ackemit_conn_kernel(Params P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= P.nconns) return;
    P.res.status[c] = dk::tcp_ackemit_check(P.tx[c], P.rx[c], P.nlinks, P.stride, P.lead);
    P.res.n_acks[c] = 0;
    P.pend[c] = 0;
}

// number of frame indices below x in svals[lo .. hi) (ascending)
__device__ __forceinline__ uint32_t count_below(const uint32_t* svals, uint32_t lo, uint32_t hi, uint32_t x) {
    const uint32_t lo0 = lo;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (svals[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo - lo0;
}

__global__ __launch_bounds__(kBlock) void ackemit_merge_kernel(Params P) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= P.n) return;
    const uint32_t i = P.svals[p];
    uint32_t lo = 0, hi = 2 * P.nconns + 1;  // the last sort key k with range[k] <= p
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (P.range[mid] <= p) lo = mid;
        else hi = mid;
    }
    if (lo == 2 * P.nconns) {  // no connection's
        P.morder[p] = i;
        P.mconn[p] = kNoConn;
        return;
    }
    const uint32_t c = lo / 2, r0 = P.range[2 * c], r1 = P.range[2 * c + 1], r2 = P.range[2 * c + 2];
    const uint32_t q = (lo & 1u) ? r0 + (p - r1) + count_below(P.svals, r0, r1, i)
                                 : p + count_below(P.svals, r1, r2, i);
    P.morder[q] = i;
    P.mconn[q] = c;
}

// The specification form: connection c's merged segments morder[r0 .. r2) by one lane.
__global__ __launch_bounds__(kWave) void ackemit_lane_kernel(Params P) {
    const uint32_t c = blockIdx.x * kWave + threadIdx.x;
    if (c >= P.nconns || P.res.status[c] != DK_TCP_ACKEMIT_OK) return;
    const uint32_t r0 = P.range[2 * c], r2 = P.range[2 * c + 2];
    uint32_t rn = P.rx[c].receive_next;  // RCV.NXT behind the connection's last segment
    for (uint32_t q = r2; q-- > r0;) {
        const uint32_t i = P.morder[q];
        const Elem e = load_elem(P, i);
        P.ackno[i] = rn;
        if (e.moves) rn = e.start;
    }
    uint32_t armed = P.dack[c].armed != 0, bits = 0, acks = 0;
    for (uint32_t q = r0; q < r2; q++) {
        const uint32_t i = P.morder[q];
        const Elem e = load_elem(P, i);
        if (e.kind == kNothing) continue;
        const bool send = e.kind == kToggle ? armed != 0 : true;
        armed = e.kind == kToggle ? armed ^ 1u : e.kind == kSet;
        bits |= kTouched | (armed ? kArmedOnce : 0u);  // whenever a row leaves it armed, that row armed it
        if (send) {
            P.flag[i] = 1;
            acks++;
        }
    }
    P.res.n_acks[c] = acks;
    P.pend[c] = bits | (armed ? kArmedLast : 0u);
}

// ---- the scan form ----
// Per thread: the composition of its items' maps and the first DELIVERED / FIN start among them. Out: mx = the
// composition of the threads before this one in the workgroup, (sv, sval) = the first start among the threads behind
// it, and the workgroup's totals.
__device__ __forceinline__ void block_scan2(uint32_t m, uint32_t v, uint32_t val, uint32_t& mx, uint32_t& sv,
                                            uint32_t& sval, uint32_t& mt, uint32_t& tv, uint32_t& tval) {
    __shared__ uint32_t s_m[kWaves], s_v[kWaves], s_val[kWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    for (uint32_t o = 1; o < kWave; o <<= 1) {
        const uint32_t um = (uint32_t)__shfl_up((int)m, o);
        const uint32_t dv = (uint32_t)__shfl_down((int)v, o), dval = (uint32_t)__shfl_down((int)val, o);
        if (lane >= o) m = compose(um, m);
        if (lane + o < kWave && !v) v = dv, val = dval;
    }
    __syncthreads();  // the arrays may still be read from a previous call
    if (lane == kWave - 1) s_m[wv] = m;
    if (lane == 0) s_v[wv] = v, s_val[wv] = val;
    __syncthreads();
    uint32_t em = (uint32_t)__shfl_up((int)m, 1);
    uint32_t ev = (uint32_t)__shfl_down((int)v, 1), eval = (uint32_t)__shfl_down((int)val, 1);
    if (lane == 0) em = kIdentity;
    if (lane == kWave - 1) ev = 0;
    uint32_t base = kIdentity;
    mt = kIdentity, tv = 0, tval = 0;
    for (uint32_t k = 0; k < kWaves; k++) {
        if (k < wv) base = compose(base, s_m[k]);
        mt = compose(mt, s_m[k]);
        if (k > wv && !ev && s_v[k]) ev = 1, eval = s_val[k];
        if (!tv && s_v[k]) tv = 1, tval = s_val[k];
    }
    mx = compose(base, em);
    sv = ev, sval = eval;
}

// One merged element as the scans see it: its map (a connection's first element composed with the constant of the
// connection's initial armed bit) and what it shows the elements before it (its start if it moves RCV.NXT; a
// connection's last element the table's receive_next otherwise).
struct ScanElem {
    uint32_t c, i, kind, map, v, val;
    bool head, tail, moves;
    uint32_t armed0, start;
};
template <bool kFromSummary>
__device__ __forceinline__ ScanElem scan_elem(const Params& P, uint32_t q) {
    ScanElem s{kNoConn, 0u, kNothing, kIdentity, 0u, 0u, false, false, false, 0u, 0u};
    if (q >= P.n) return s;
    s.c = P.mconn[q];
    if (s.c == kNoConn) return s;
    s.i = P.morder[q];
    if (kFromSummary) {
        const uint64_t u = P.esum[q];
        s.kind = (uint32_t)(u >> 32) & 3u, s.moves = (u >> 34) & 1u, s.start = (uint32_t)u;
    } else {
        const Elem e = load_elem(P, s.i);
        s.kind = e.kind, s.moves = e.moves, s.start = e.start;
        P.esum[q] = (uint64_t)e.start | (uint64_t)(e.kind | (e.moves ? 4u : 0u)) << 32;
    }
    s.head = q == P.range[2 * s.c];
    s.tail = q + 1 == P.range[2 * s.c + 2];
    s.map = map_of(s.kind);
    if (s.head) {
        s.armed0 = P.dack[s.c].armed != 0;
        s.map = apply(s.map, s.armed0) * 3u;
    }
    s.v = s.moves || s.tail;
    s.val = s.moves ? s.start : s.tail ? P.rx[s.c].receive_next : 0u;
    return s;
}

__global__ __launch_bounds__(kBlock) void ackemit_tile_kernel(Params P) {
    const uint32_t q0 = blockIdx.x * kTile + threadIdx.x * kItems;
    uint32_t m = kIdentity, v = 0, val = 0;
#pragma unroll
    for (uint32_t k = 0; k < kItems; k++) {
        const ScanElem s = scan_elem<false>(P, q0 + k);
        m = compose(m, s.map);
        if (!v && s.v) v = 1, val = s.val;
    }
    uint32_t mx, sv, sval, mt, tv, tval;
    block_scan2(m, v, val, mx, sv, sval, mt, tv, tval);
    if (threadIdx.x == 0) {
        P.tile_m[blockIdx.x] = mt;
        P.tile_v[blockIdx.x] = (uint64_t)tval | (uint64_t)tv << 32;
    }
}

// One workgroup: the composition of the tiles before each tile, and the first start of the tiles behind it, in place.
__global__ __launch_bounds__(kBlock) void ackemit_spine_kernel(Params P, uint32_t nb) {
    uint32_t mx, sv, sval, mt, tv, tval;
    uint32_t carry = kIdentity;
    for (uint32_t k0 = 0; k0 < nb; k0 += kBlock) {
        const uint32_t k = k0 + threadIdx.x;
        block_scan2(k < nb ? P.tile_m[k] : kIdentity, 0u, 0u, mx, sv, sval, mt, tv, tval);
        if (k < nb) P.tile_m[k] = compose(carry, mx);
        carry = compose(carry, mt);
    }
    uint32_t cv = 0, cval = 0;
    for (uint32_t k0 = (nb - 1) / kBlock * kBlock;; k0 -= kBlock) {
        const uint32_t k = k0 + threadIdx.x;
        const uint64_t u = k < nb ? P.tile_v[k] : 0ull;
        block_scan2(kIdentity, (uint32_t)(u >> 32), (uint32_t)u, mx, sv, sval, mt, tv, tval);
        if (k < nb) P.tile_v[k] = sv ? (uint64_t)sval | 1ull << 32 : (uint64_t)cval | (uint64_t)cv << 32;
        if (tv) cv = 1, cval = tval;
        if (k0 == 0) break;
    }
}

__global__ __launch_bounds__(kBlock) void ackemit_apply_kernel(Params P) {
    const uint32_t q0 = blockIdx.x * kTile + threadIdx.x * kItems;
    ScanElem s[kItems];
    uint32_t m = kIdentity, v = 0, val = 0;
#pragma unroll
    for (uint32_t k = 0; k < kItems; k++) {
        s[k] = scan_elem<true>(P, q0 + k);
        m = compose(m, s[k].map);
        if (!v && s[k].v) v = 1, val = s[k].val;
    }
    uint32_t mx, sv, sval, mt, tv, tval;
    block_scan2(m, v, val, mx, sv, sval, mt, tv, tval);
    uint32_t before = compose(P.tile_m[blockIdx.x], mx);  // of everything before the thread's first item
    if (!sv) sval = (uint32_t)P.tile_v[blockIdx.x];        // a connection's last element always shows a value
    // what each item sees behind it: the first start among the thread's later items, else the thread's
    uint32_t behind[kItems];
#pragma unroll
    for (int k = (int)kItems - 1; k >= 0; k--) {
        behind[k] = sval;
        if (s[k].v) sval = s[k].val;
    }
    // the connection's counts, gathered over the thread's items of one connection before they go to memory
    uint32_t cur = kNoConn, acks = 0, bits = 0;
    const auto flush = [&]() {
        if (cur == kNoConn) return;
        if (acks) atomicAdd(P.res.n_acks + cur, acks);
        if (bits) atomicOr(P.pend + cur, bits);
    };
#pragma unroll
    for (uint32_t k = 0; k < kItems; k++) {
        const ScanElem& e = s[k];
        const uint32_t armed = e.head ? e.armed0 : before & 1u;  // behind a head the composition is a constant
        before = compose(before, e.map);
        if (e.c == kNoConn || P.res.status[e.c] != DK_TCP_ACKEMIT_OK) continue;
        if (e.c != cur) {
            flush();
            cur = e.c, acks = 0, bits = 0;
        }
        const uint32_t after = e.kind == kNothing ? armed : e.kind == kToggle ? armed ^ 1u : e.kind == kSet;
        if (e.kind != kNothing) bits |= kTouched | (after ? kArmedOnce : 0u);
        if (e.tail && after) bits |= kArmedLast;
        if (e.kind == kToggle ? armed != 0 : e.kind != kNothing) {
            P.flag[e.i] = 1;
            P.ackno[e.i] = e.tail ? P.rx[e.c].receive_next : behind[k];
            acks++;
        }
    }
    // a wave whose items are all one connection's sends one pair of atomics
    const uint32_t first = s[0].c, c0 = (uint32_t)__shfl((int)first, 0);
    const bool mine = cur == first && first == s[kItems - 1].c && first != kNoConn;
    if (__all(mine && first == c0)) {
        for (uint32_t o = kWave / 2; o; o >>= 1) {
            acks += (uint32_t)__shfl_xor((int)acks, (int)o);
            bits |= (uint32_t)__shfl_xor((int)bits, (int)o);
        }
        if ((threadIdx.x & (kWave - 1)) != 0) cur = kNoConn;
    }
    flush();
}

// ack_frame per batch frame, the dack rows and NO_ROOM per connection, n_frames: behind the call's one capacity test.
__global__ __launch_bounds__(kBlock) void ackemit_finish_kernel(Params P) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const uint64_t total = P.tot[0];
    const bool fits = dk::tcp_tx_fits(total, P.max_frames, P.stride, P.out_bytes);
    if (j == 0) *P.res.n_frames = (uint32_t)total;  // at most n
    if (j < P.n) {
        const uint64_t first = P.flag[j];
        const bool emits = (j + 1 < P.n ? P.flag[j + 1] : total) != first;
        P.res.ack_frame[j] = emits && fits ? (uint32_t)first : 0xFFFFFFFFu;
    }
    if (j < P.nconns && P.res.status[j] == DK_TCP_ACKEMIT_OK) {
        if (!fits) {
            if (P.res.n_acks[j]) P.res.status[j] = DK_TCP_ACKEMIT_NO_ROOM;
            return;
        }
        const uint32_t bits = P.pend[j];
        dk_tcp_dack_conn& D = P.dack[j];
        if (bits & kTouched) D.armed = (bits & kArmedLast) != 0;
        if (bits & kArmedOnce) D.deadline_ns = P.now + D.delay_ns;
    }
}

using dk::ctl::DeviceGuard;
using dk::ctl::round16;

}  // namespace
}  // namespace dk_tcp_ackemit

extern "C" {

int dk_diag_tcp_ack_emit_set_form(dk_tcp_ctx* t, int32_t form) {
    dk_tcp_order o;
    if (dk_tcp_ctx_order(t, &o) || form < -1 || form > 1) return EINVAL;
    o.emit->form = form;
    return 0;
}

int dk_diag_tcp_ack_emit_last_form(const dk_tcp_ctx* t) {
    dk_tcp_order o;
    return dk_tcp_ctx_order(const_cast<dk_tcp_ctx*>(t), &o) ? -1 : o.emit->last_form;
}

int dk_tcp_ack_emit(dk_tcp_ctx* t, const dk_rx_results* rx, uint32_t n, const uint8_t* action, const dk_tcp_view* view,
                    const dk_tcp_conn* rx_conns, const dk_tcp_tx_conn* tx_conns, dk_tcp_dack_conn* dack, uint32_t nconns,
                    const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns, uint8_t* out, uint64_t out_bytes,
                    const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t flags,
                    const dk_tcp_ackemit_results* res, void* stream) {
    using namespace dk_tcp_ackemit;
    dk_tcp_order o;
    if (dk_tcp_ctx_order(t, &o) || !rx || !layout || !res || !res->n_frames || !links || nlinks == 0) return EINVAL;
    if (out_bytes > DK_RX_MAX_BLOB) return EINVAL;
    if (n && (!action || !view || !res->ack_frame)) return EINVAL;
    if (nconns && (!rx_conns || !tx_conns || !dack || !res->status || !res->n_acks)) return EINVAL;
    if (n && nconns && (!rx->flow_id || (max_frames && (!out || !res->off_out || !res->len_out)))) return EINVAL;
    if ((reinterpret_cast<uintptr_t>(rx_conns) | reinterpret_cast<uintptr_t>(tx_conns) |
         reinterpret_cast<uintptr_t>(dack)) & 15)
        return EINVAL;
    // in turn: after the dk_tcp_rx_process call of this context whose order it reuses, once
    if (!o.live || o.call == 0 || o.emit->done == o.call || n != o.n || nconns != o.nconns) return EINVAL;
    DeviceGuard g(o.device);
    const hipStream_t s = (hipStream_t)stream;
    // the scratch, before the turn is taken: a call that cannot get it leaves the turn to its retry
    const uint32_t nb = (n + kTile - 1) / kTile, sb = dk_tcp_tx_scan_tiles(n);
    const size_t need = 3 * round16((size_t)n * 4) + 2 * round16((size_t)n * 8) + round16((size_t)sb * 8) +
                        round16((size_t)nb * 4) + round16((size_t)nb * 8) + round16((size_t)nconns * 4) + 16;
    if (int rc = o.emit->scratch.grow(*o.serial, need)) return rc;
    o.emit->done = o.call;
    o.emit->last_form = -1;
    if (o.serial->order(s)) return EIO;
    Params P{};
    P.svals = o.svals, P.range = o.range, P.rec = o.rec;
    P.action = action, P.view = view, P.rx = rx_conns, P.tx = tx_conns, P.dack = dack;
    P.n = n, P.nconns = nconns, P.nlinks = nlinks;
    P.stride = layout->slot_stride, P.lead = layout->frame_lead, P.max_frames = max_frames;
    P.out_bytes = out_bytes, P.now = now_ns;
    dk::ctl::Carver c{o.emit->scratch.p};
    P.flag = c.take<uint64_t>(n);
    P.esum = c.take<uint64_t>(n);
    uint64_t* bsum = c.take<uint64_t>(sb);
    P.tile_v = c.take<uint64_t>(nb);
    P.tot = c.take<uint64_t>(1);
    P.morder = c.take<uint32_t>(n);
    P.mconn = c.take<uint32_t>(n);
    P.ackno = c.take<uint32_t>(n);
    P.tile_m = c.take<uint32_t>(nb);
    P.pend = c.take<uint32_t>(nconns);
    P.res = *res;
    const dim3 per_conn((nconns + kBlock - 1) / kBlock), per_frame((n + kBlock - 1) / kBlock);
    if (nconns) hipLaunchKernelGGL(ackemit_conn_kernel, per_conn, dim3(kBlock), 0, s, P);
    if (n == 0 || nconns == 0) {  // no segment of a connection: no ACK, no row changes
        if (hipMemsetAsync(res->n_frames, 0, sizeof(uint32_t), s) != hipSuccess) return EIO;
        if (n && hipMemsetAsync(res->ack_frame, 0xFF, (size_t)n * sizeof(uint32_t), s) != hipSuccess) return EIO;
    } else {
        const int form = o.emit->form >= 0 ? o.emit->form : (uint64_t)n >= (uint64_t)kScanMinSegs * nconns ? 1 : 0;
        o.emit->last_form = form;
        if (hipMemsetAsync(P.flag, 0, (size_t)n * 8, s) != hipSuccess) return EIO;
        hipLaunchKernelGGL(ackemit_merge_kernel, per_frame, dim3(kBlock), 0, s, P);
        if (form == 1) {
            hipLaunchKernelGGL(ackemit_tile_kernel, dim3(nb), dim3(kBlock), 0, s, P);
            hipLaunchKernelGGL(ackemit_spine_kernel, dim3(1), dim3(kBlock), 0, s, P, nb);
            hipLaunchKernelGGL(ackemit_apply_kernel, dim3(nb), dim3(kBlock), 0, s, P);
        } else {
            hipLaunchKernelGGL(ackemit_lane_kernel, dim3((nconns + kWave - 1) / kWave), dim3(kWave), 0, s, P);
        }
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag, n, bsum, P.tot, s)) return EIO;
        // the builder reads the tables and the scratch, never the rows the finish kernel writes, and runs first
        dk::TcpAckEmitParams E{out, out_bytes, tx_conns, rx_conns, links, P.flag, P.tot, rx->flow_id, P.ackno, n,
                               layout->slot_stride, layout->frame_lead, max_frames, flags, res->off_out, res->len_out,
                               res->frame_conn, res->frame_seg};
        const uint32_t grid = std::min<uint32_t>(std::min(max_frames, n) / kBlock + 1, 2048u);
        if (max_frames && dk_launch_tcp_ack_emit(E, grid, s)) return EIO;
        hipLaunchKernelGGL(ackemit_finish_kernel, dim3((std::max(n, nconns) + kBlock - 1) / kBlock), dim3(kBlock), 0, s, P);
    }
    return o.serial->record(s);
}

}  // extern "C"
