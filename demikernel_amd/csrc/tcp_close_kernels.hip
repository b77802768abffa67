// tcp_close_kernels.hip — closing a connection on the GPU (include/dk_tcp.h, the dk_tcp_close_* section): close() up to
// its first await for a batch of connections, the close coroutine's loop (local_close, remote_already_closed) over a
// whole receive batch, and TIME-WAIT's end.
//
// A row's loop in dk_tcp_close_process ends after at most two transitions (FIN_WAIT_1 -> FIN_WAIT_2 | CLOSING -> a final
// state; every other live state goes straight to a final one), and what a frame does depends on the row's state and on
// three bits of the frame alone (A, U, F: snd_nxt does not move in a call). Each transition is "the first frame after
// index t that triggers one from state s", so no sort and no per-row walk is needed:
//   1. cls_check_kernel     per row: status, and the snapshot (state, RCV.NXT) the later passes read.
//   2. cls_classify_kernel  per frame: its row and bits; a 32-bit atomicMin finds T1, the first frame that moves the row
//                           out of its state.
//   3. cls_second_kernel    the rows whose state after T1 is not final: a second atomicMin over the frames behind T1
//                           finds T2. Both minima are exact for any number of frames per row.
//   4. cls_decide_kernel    every frame's state-before by comparing its index with T1 and T2; its action, its replies
//                           (0, 1 or 2) and whether it makes a done record. Two scans number the replies and the records.
//   5. cls_build_kernel     the frames, the records and the per-frame results, behind the call's one capacity test,
//                           made on the device; cls_finish_kernel the rows (one thread is a row's only writer), the two
//                           words and NO_ROOM.
// dk_tcp_close_start is a prefix maximum (one workgroup), flag, scan, build over close[] entries; dk_tcp_close_timers is
// flag, scan, build over rows. No loop depends on another workgroup's progress. Atomics are agent-scope integer
// __hip_atomic_* on global memory; everything else is plain vector stores. The frame builder is ctl_common.h's.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <mutex>

#include "../../include/dk_tcp.h"
#include "ctl_common.h"

namespace dk_tcp_close {
namespace {
using namespace dk::ctl;

constexpr uint32_t kNone = DK_TCP_CLS_NONE;

// bits[i]: what the classify pass leaves per frame
constexpr uint32_t kA = 1, kU = 2, kF = 4, kLive = 8;

struct Params {
    dk_rx_results rx;
    uint32_t n;
    dk_tcp_closer* rows;
    dk_tcp_conn* rxc;
    const dk_tcp_tx_conn* txc;
    dk_tcp_tx_conn* txw;  // dk_tcp_close_timers: the table it may write
    dk_tcp_dack_conn* dack;
    uint32_t nconns;
    const uint8_t* action_in;
    const dk_tx_link* links;
    uint32_t nlinks;
    uint64_t now;
    uint8_t* out;
    uint64_t out_bytes;
    uint32_t stride, lead, max_frames, max_done, flags;
    dk_tcp_cls_results res;
    // dk_tcp_close_start
    const uint32_t* close;
    uint32_t nclose;
    uint32_t *st_status, *push_conn, *push_off, *push_len, *n_markers;
    uint64_t* pmax;  // [nclose]: 1 + the maximum of close[0 .. k), 0 for k == 0
    // scratch
    uint32_t *t1, *t2;            // [nconns]: the row's first and second transition frames
    uint32_t *s0, *rn0, *work, *sent;  // [nconns]: the live state (0: none) and RCV.NXT before the call; had frames; sent an ACK
    uint8_t *bits, *act, *sa;     // [n]
    uint64_t *flag_r, *flag_y, *tot;  // [items] x 2, [2]: replies, records
};

__device__ __forceinline__ bool fits(const Params& P) {
    return dk::tcp_tx_fits(P.tot[0], P.max_frames, P.stride, P.out_bytes) && P.tot[1] <= P.max_done;
}

// ---- the state table (dk_tcp.h) -----------------------------------------------------------------------------------------
__device__ __forceinline__ bool live(uint32_t s) {
    return s == DK_TCP_CLS_FIN_WAIT_1 || s == DK_TCP_CLS_FIN_WAIT_2 || s == DK_TCP_CLS_CLOSING || s == DK_TCP_CLS_LAST_ACK;
}
__device__ __forceinline__ bool final_state(uint32_t s) {
    return s == DK_TCP_CLS_TIME_WAIT || s == DK_TCP_CLS_CLOSED || s == DK_TCP_CLS_FAULT;
}
// Whether a frame with bits b moves a row out of state s.
__device__ __forceinline__ bool triggers(uint32_t s, uint32_t b) {
    if (s == DK_TCP_CLS_FIN_WAIT_2) return (b & kF) != 0;
    if (s == DK_TCP_CLS_LAST_ACK) return (b & kA) != 0;
    return (b & (kA | kF)) != 0;  // FIN_WAIT_1, CLOSING
}
// The state after a frame with bits b that triggers(s, b).
__device__ __forceinline__ uint32_t next_state(uint32_t s, uint32_t b) {
    if (s == DK_TCP_CLS_FIN_WAIT_1)
        return (b & kA) ? ((b & kF) ? DK_TCP_CLS_TIME_WAIT : DK_TCP_CLS_FIN_WAIT_2) : DK_TCP_CLS_CLOSING;
    if (s == DK_TCP_CLS_FIN_WAIT_2) return DK_TCP_CLS_TIME_WAIT;
    if (s == DK_TCP_CLS_CLOSING) return (b & kF) ? DK_TCP_CLS_FAULT : DK_TCP_CLS_TIME_WAIT;
    return DK_TCP_CLS_CLOSED;  // LAST_ACK
}
// process_remote_close consumes the FIN in the local_close loop only, and CLOSING + F applies nothing.
__device__ __forceinline__ bool consumes_fin(uint32_t s, uint32_t b) {
    return (b & kF) && (s == DK_TCP_CLS_FIN_WAIT_1 || s == DK_TCP_CLS_FIN_WAIT_2);
}

// Row c after the call, from its snapshot and its two minima.
struct RowEnd {
    uint32_t state, last, fin;  // the final state, the frame that made it (kNone: the row did not move), the FIN's frame
};
__device__ __forceinline__ RowEnd row_end(const Params& P, uint32_t c) {
    const uint32_t s0 = P.s0[c], T1 = P.t1[c];
    RowEnd e{s0, kNone, kNone};
    if (s0 == 0 || T1 == kNone) return e;
    const uint32_t b1 = P.bits[T1], s1 = next_state(s0, b1);
    e.state = s1, e.last = T1;
    if (consumes_fin(s0, b1)) e.fin = T1;
    const uint32_t T2 = P.t2[c];
    if (final_state(s1) || T2 == kNone) return e;
    const uint32_t b2 = P.bits[T2];
    e.state = next_state(s1, b2), e.last = T2;
    if (consumes_fin(s1, b2)) e.fin = T2;
    return e;
}

// Ethernet2 + IPv4 + TCP, flags ACK, no options, no payload: the bytes dk_tcp_ack_emit writes for the connection.
__device__ void build_ack(uint8_t* a, const dk_tx_link* lk, const dk_tcp_tx_conn& T, uint32_t ack, uint32_t win,
                          bool offload) {
    tcp_frame(a, lk, T.ip_word, T.local_ip, T.remote_ip, T.ports & 0xFFFFu, T.ports >> 16, T.snd_nxt, ack, 0x10u, win, false,
              0u, 0u, offload);
}

// Reply f of the call: an ACK of connection c carrying RCV.NXT = ack, triggered by batch frame seg.
__device__ void emit_ack(const Params& P, uint64_t f, uint32_t seg, uint32_t c, uint32_t ack) {
    const dk_tcp_tx_conn& T = P.txc[c];
    const dk_tcp_conn& R = P.rxc[c];
    const uint32_t win = ((uint32_t)(R.buffer_size - (ack - R.reader_next)) >> (T.rcv_wscale & 31u)) & 0xFFFFu;
    const uint32_t foff = (uint32_t)(f * P.stride + P.lead);
    P.res.off_out[f] = foff;
    P.res.len_out[f] = (uint16_t)DK_TCP_CLS_ACK_BYTES;
    if (P.res.frame_seg) P.res.frame_seg[f] = seg;
    build_ack(P.out + foff, P.links + T.link, T, ack, win, (P.flags & DK_TX_OFFLOAD_TCP) != 0);
}

// The row checks of dk_tcp_close_process, in dk_tcp.h's order.
__device__ __forceinline__ uint32_t row_check(const Params& P, uint32_t c) {
    const dk_tcp_conn& R = P.rxc[c];
    const dk_tcp_tx_conn& T = P.txc[c];
    if (R.state != DK_TCP_CLOSED) return DK_TCP_CLS_E_RX_STATE;
    if (T.state != DK_TCP_ESTABLISHED) return DK_TCP_CLS_E_STATE;
    if (T.link >= P.nlinks) return DK_TCP_CLS_E_LINK;
    if (T.rcv_wscale > 14) return DK_TCP_CLS_E_WSCALE;
    if ((R.buffer_size >> T.rcv_wscale) > 0xFFFFu) return DK_TCP_CLS_E_WINDOW;
    if ((uint64_t)P.lead + DK_TCP_CLS_ACK_BYTES > P.stride) return DK_TCP_CLS_E_SLOT;
    return DK_TCP_CLS_OK;
}

// ---- dk_tcp_close_process -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cls_check_kernel(Params P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= P.nconns) return;
    const uint32_t s = P.rows[c].state;
    const uint32_t st = live(s) ? row_check(P, c) : (uint32_t)DK_TCP_CLS_OK;
    P.res.status[c] = st;
    P.s0[c] = live(s) && st == DK_TCP_CLS_OK ? s : 0u;
    P.rn0[c] = P.rxc[c].receive_next;
}

// Frame i's row if it belongs to a live row that passed its checks, else kNone.
__device__ __forceinline__ uint32_t live_row(const Params& P, uint32_t i) {
    const uint32_t f = P.rx.flow_id[i];
    return (P.rx.meta[i] & 0xFFu) == DK_V_OK_TCP && f < P.nconns && P.s0[f] != 0 ? f : kNone;
}

__global__ __launch_bounds__(kBlock) void cls_classify_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    uint32_t b = 0;
    const uint32_t c = live_row(P, i);
    if (c != kNone) {
        const uint32_t fl = P.rx.meta[i] >> 16;  // byte 13: FIN 1, ACK 16
        b = kLive | ((fl & 1u) ? kF : 0u);
        if (fl & 16u) b |= (int32_t)(P.rx.tcp_ack[i] - P.txc[c].snd_nxt) <= 0 ? kA : kU;
        P.work[c] = 1;
        if (triggers(P.s0[c], b)) min32(P.t1 + c, i);
    }
    P.bits[i] = (uint8_t)b;
}

__global__ __launch_bounds__(kBlock) void cls_second_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t b = P.bits[i];
    if (!(b & kLive)) return;
    const uint32_t c = P.rx.flow_id[i], T1 = P.t1[c];
    if (T1 == kNone || i <= T1) return;
    const uint32_t s1 = next_state(P.s0[c], P.bits[T1]);
    if (!final_state(s1) && triggers(s1, b)) min32(P.t2 + c, i);
}

__global__ __launch_bounds__(kBlock) void cls_decide_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t b = P.bits[i];
    uint32_t act = 0, sa = 0, replies = 0;
    bool done = false;
    if (b & kLive) {
        const uint32_t c = P.rx.flow_id[i], s0 = P.s0[c], T1 = P.t1[c];
        uint32_t sb = s0;  // the state the frame meets; 0: never popped
        if (T1 != kNone && i > T1) {
            const uint32_t s1 = next_state(s0, P.bits[T1]), T2 = P.t2[c];
            sb = s1;
            if (final_state(s1)) sb = 0, sa = s1;
            else if (T2 != kNone && i > T2) sb = 0, sa = next_state(s1, P.bits[T2]);
        }
        if (sb == 0) {
            act = DK_TCP_CLS_UNPROCESSED;
        } else {
            sa = triggers(sb, b) ? next_state(sb, b) : sb;
            done = final_state(sa);
            if (sa == DK_TCP_CLS_FAULT) {
                act = DK_TCP_CLS_FAULT_BIT;
            } else {
                const bool fin = consumes_fin(sb, b);
                act = DK_TCP_CLS_POPPED | ((b & kA) ? DK_TCP_CLS_ACK_OK : 0u) | ((b & kU) ? DK_TCP_CLS_ACK_UNSENT : 0u) |
                      (fin ? DK_TCP_CLS_FIN : 0u);
                replies = ((b & kU) ? 1u : 0u) + (fin ? 1u : 0u);
                if (replies) P.sent[c] = 1;
            }
        }
    }
    P.act[i] = (uint8_t)act;
    P.sa[i] = (uint8_t)sa;
    P.flag_r[i] = replies;
    P.flag_y[i] = done;
}

// Behind the capacity test. Nothing a row's frames read here is written before cls_finish_kernel.
__global__ __launch_bounds__(kBlock) void cls_build_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n || !fits(P)) return;
    const uint32_t act = P.act[i], b = P.bits[i];
    uint32_t rf = kNone, aa = P.action_in ? P.action_in[i] : (uint32_t)DK_TCP_SKIP;
    if (b & kLive) {
        const uint32_t c = P.rx.flow_id[i];
        aa = !(act & DK_TCP_CLS_POPPED) ? DK_TCP_UNPROCESSED
             : (b & kA)                  ? DK_TCP_NO_DATA
             : (b & kU)                  ? DK_TCP_ACK_UNSENT
                                         : DK_TCP_NO_ACK;
        if (act & (DK_TCP_CLS_ACK_UNSENT | DK_TCP_CLS_FIN)) {
            const RowEnd e = row_end(P, c);
            uint64_t f = P.flag_r[i];
            rf = (uint32_t)f;
            const uint32_t rn = P.rn0[c] + (e.fin != kNone && e.fin < i ? 1u : 0u);  // RCV.NXT as the frame met it
            if (act & DK_TCP_CLS_ACK_UNSENT) emit_ack(P, f++, i, c, rn);
            if (act & DK_TCP_CLS_FIN) emit_ack(P, f, i, c, rn + 1u);
        }
        if (P.flag_y[i] != (i + 1 < P.n ? P.flag_y[i + 1] : P.tot[1])) {  // this frame ended its row's loop
            const RowEnd e = row_end(P, c);
            const dk_tcp_closer& R = P.rows[c];
            dk_tcp_cls_done* Y = P.res.done + P.flag_y[i];
            Y->row = c;
            Y->state = (uint16_t)e.state;
            Y->err = (uint16_t)(e.state == DK_TCP_CLS_FAULT ? EPROTO : R.err);
            Y->frame = i;
            Y->fin_frame = e.fin;
            Y->deadline_ns = e.state == DK_TCP_CLS_TIME_WAIT ? P.now + R.linger_ns : R.deadline_ns;
            Y->reserved = 0;
        }
    }
    P.res.action[i] = (uint8_t)act;
    P.res.state_after[i] = P.sa[i];
    P.res.ack_action[i] = (uint8_t)aa;
    P.res.reply_frame[i] = rf;
}

// The rows, the two words and NO_ROOM.
__global__ __launch_bounds__(kBlock) void cls_finish_kernel(Params P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    const bool ok = fits(P);
    if (c == 0) {
        *P.res.n_frames = (uint32_t)P.tot[0];
        *P.res.n_done = (uint32_t)P.tot[1];
    }
    if (c >= P.nconns) return;
    if (!ok) {
        if (P.res.status[c] == DK_TCP_CLS_OK && P.work[c]) P.res.status[c] = DK_TCP_CLS_NO_ROOM;
        return;
    }
    uint32_t fin = kNone;
    if (P.n && P.s0[c] != 0) {
        const RowEnd e = row_end(P, c);
        fin = e.fin;
        dk_tcp_closer& R = P.rows[c];
        if (e.last != kNone) {
            R.state = (uint16_t)e.state;
            if (e.state == DK_TCP_CLS_FAULT) R.err = EPROTO;
            if (e.state == DK_TCP_CLS_TIME_WAIT) R.deadline_ns = P.now + R.linger_ns;
        }
        if (fin != kNone) P.rxc[c].receive_next = P.rn0[c] + 1u;
        if (P.dack && P.sent[c]) P.dack[c].armed = 0;  // emit() clears the deadline (ctrlblk.rs:761)
    }
    P.res.fin_frame[c] = fin;
}

// ---- dk_tcp_close_timers ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cls_sweep_kernel(Params P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= P.nconns) return;
    const dk_tcp_closer& R = P.rows[c];
    const bool due = R.state == DK_TCP_CLS_TIME_WAIT && R.deadline_ns <= P.now;
    const bool rec = (due || R.state == DK_TCP_CLS_CLOSED) && !(R.flags & DK_TCP_CLS_RETIRED);
    P.st_status[c] = DK_TCP_CLS_OK;
    P.work[c] = (due ? 1u : 0u) | (rec ? 2u : 0u);
    P.flag_y[c] = rec;
}

__global__ __launch_bounds__(kBlock) void cls_expire_kernel(Params P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    const bool ok = P.tot[1] <= P.max_done;
    if (c == 0) *P.res.n_done = (uint32_t)P.tot[1];
    if (c >= P.nconns) return;
    const uint32_t w = P.work[c];
    if (!w) return;
    if (!ok) {
        P.st_status[c] = DK_TCP_CLS_NO_ROOM;
        return;
    }
    dk_tcp_closer& R = P.rows[c];
    if (w & 1u) R.state = DK_TCP_CLS_CLOSED;
    if (w & 2u) {
        R.flags |= DK_TCP_CLS_RETIRED;
        if (P.txw) P.txw[c].state = DK_TCP_CLOSED;
        dk_tcp_cls_done* Y = P.res.done + P.flag_y[c];
        Y->row = c;
        Y->state = DK_TCP_CLS_CLOSED;
        Y->err = R.err;
        Y->frame = kNone;
        Y->fin_frame = kNone;
        Y->deadline_ns = R.deadline_ns;
        Y->reserved = 0;
    }
}

// ---- dk_tcp_close_start -------------------------------------------------------------------------------------------------
// One workgroup: pmax[k] = 1 + max(close[0 .. k)), 0 for k == 0, 256 entries a step with the running maximum carried.
__global__ __launch_bounds__(kBlock) void cls_pmax_kernel(Params P) {
    __shared__ uint64_t s_w[kBlock / kWave];
    const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < P.nclose; base += kBlock) {  // uniform
        const uint32_t k = base + threadIdx.x;
        const uint64_t own = k < P.nclose ? (uint64_t)P.close[k] + 1u : 0u;
        uint64_t v = own;  // inclusive maximum within the wave
        for (uint32_t o = 1; o < kWave; o <<= 1) {
            const uint64_t u = __shfl_up(v, o);
            if (lane >= o) v = u > v ? u : v;
        }
        __syncthreads();  // s_w of the step before has been read
        if (lane == kWave - 1) s_w[wv] = v;
        __syncthreads();
        uint64_t ex = __shfl_up(v, 1);  // exclusive
        if (lane == 0) ex = 0;
        uint64_t all = carry;
        for (uint32_t w = 0; w < kBlock / kWave; w++) {
            if (w < wv) ex = s_w[w] > ex ? s_w[w] : ex;
            all = s_w[w] > all ? s_w[w] : all;
        }
        if (k < P.nclose) P.pmax[k] = ex > carry ? ex : carry;
        carry = all;
    }
}

__global__ __launch_bounds__(kBlock) void cls_admit_kernel(Params P) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= P.nclose) return;
    const uint32_t c = P.close[k];
    uint32_t st = DK_TCP_CLS_OK;
    if (c >= P.nconns) st = DK_TCP_CLS_E_ROW;
    else if ((uint64_t)c + 1u <= P.pmax[k]) st = DK_TCP_CLS_E_ORDER;
    else if (P.txc[c].state != DK_TCP_ESTABLISHED) st = DK_TCP_CLS_E_STATE;
    else if (P.rows[c].state != DK_TCP_CLS_IDLE || P.rxc[c].state == DK_TCP_NONE) st = DK_TCP_CLS_E_BADF;
    P.st_status[k] = st;
    P.flag_r[k] = st == DK_TCP_CLS_OK;
}

// An accepted connection appears once in close[] (the list ascends), so its thread is the row's only writer.
__global__ __launch_bounds__(kBlock) void cls_open_kernel(Params P) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k == 0) *P.n_markers = (uint32_t)P.tot[0];
    if (k >= P.nclose) return;
    P.push_off[k] = 0;
    P.push_len[k] = 0;
    if (k >= P.tot[0]) P.push_conn[k] = 0xFFFFFFFFu;
    if (P.st_status[k] != DK_TCP_CLS_OK) return;
    const uint32_t c = P.close[k];
    dk_tcp_closer& R = P.rows[c];
    if (P.rxc[c].state == DK_TCP_ESTABLISHED) {
        R.state = DK_TCP_CLS_FIN_WAIT_1;
        P.rxc[c].state = DK_TCP_CLOSED;  // poll() has returned
    } else {
        R.state = DK_TCP_CLS_LAST_ACK;
    }
    R.err = 0, R.flags = 0, R.deadline_ns = 0;
    P.push_conn[P.flag_r[k]] = c;
}

// ---- the host side ------------------------------------------------------------------------------------------------------
CallScratch g_pool[kMaxDevices];  // one per device: the calls' scratch, and the event that serialises them on it
std::mutex g_mutex;

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace
}  // namespace dk_tcp_close

extern "C" {

int dk_tcp_close_start(dk_tcp_closer* rows, dk_tcp_conn* rx_conns, const dk_tcp_tx_conn* tx_conns, uint32_t nconns,
                       const uint32_t* close, uint32_t nclose, uint32_t* status, uint32_t* push_conn, uint32_t* push_off,
                       uint32_t* push_len, uint32_t* n_markers, void* stream) {
    using namespace dk_tcp_close;
    if (!n_markers || nclose > 0x7FFFFFFFu) return EINVAL;
    if (nconns && (!rows || !rx_conns || !tx_conns)) return EINVAL;
    if (misaligned(rows) || misaligned(rx_conns) || misaligned(tx_conns)) return EINVAL;
    if (nclose && (!close || !status || !push_conn || !push_off || !push_len)) return EINVAL;
    std::lock_guard<std::mutex> lock(g_mutex);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t sb = dk_tcp_tx_scan_tiles(nclose);
    const size_t need = round16(2 * 8) + 2 * round16((size_t)nclose * 8) + round16((size_t)sb * 8) + 16;
    CallScratch* pool = nullptr;
    if (int rc = enter_pool(g_pool, need, s, &pool)) return rc;
    Params P{};
    P.rows = rows, P.rxc = rx_conns, P.txc = tx_conns, P.nconns = nconns;
    P.close = close, P.nclose = nclose, P.st_status = status;
    P.push_conn = push_conn, P.push_off = push_off, P.push_len = push_len, P.n_markers = n_markers;
    Carver c{pool->scratch.p};
    P.tot = c.take<uint64_t>(2);
    P.flag_r = c.take<uint64_t>(nclose);
    P.pmax = c.take<uint64_t>(nclose);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if (hipMemsetAsync(P.tot, 0, 16, s) != hipSuccess) return EIO;
    if (nclose) {
        hipLaunchKernelGGL(cls_pmax_kernel, dim3(1), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(cls_admit_kernel, grid_for(nclose), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, nclose, bsum, P.tot, s)) return EIO;
    }
    hipLaunchKernelGGL(cls_open_kernel, grid_for(nclose), dim3(kBlock), 0, s, P);
    return pool->record(s);
}

int dk_tcp_close_process(const dk_rx_results* rx, uint32_t n, dk_tcp_closer* rows, dk_tcp_conn* rx_conns,
                         const dk_tcp_tx_conn* tx_conns, dk_tcp_dack_conn* dack, uint32_t nconns,
                         const uint8_t* action_in, const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns,
                         uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames,
                         uint32_t max_done, uint32_t flags, const dk_tcp_cls_results* res, void* stream) {
    using namespace dk_tcp_close;
    if (!rx || !layout || !res || !res->n_frames || !res->n_done || !links || nlinks == 0) return EINVAL;
    if (out_bytes > DK_RX_MAX_BLOB || n > 0x7FFFFFFFu) return EINVAL;
    if (nconns && (!rows || !rx_conns || !tx_conns || !res->status || !res->fin_frame)) return EINVAL;
    if (misaligned(rows) || misaligned(rx_conns) || misaligned(tx_conns) || misaligned(dack)) return EINVAL;
    if (n && (!rx->meta || !rx->flow_id || !rx->tcp_seq || !rx->tcp_ack || !res->action || !res->state_after ||
              !res->ack_action || !res->reply_frame))
        return EINVAL;
    if (n && nconns && ((max_frames && (!out || !res->off_out || !res->len_out)) || (max_done && !res->done))) return EINVAL;
    std::lock_guard<std::mutex> lock(g_mutex);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t sb = dk_tcp_tx_scan_tiles(n);
    const size_t ff_bytes = 2 * round16((size_t)nconns * 4);
    const size_t zero_bytes = 2 * round16((size_t)nconns * 4) + round16(2 * 8);
    const size_t need = ff_bytes + zero_bytes + 2 * round16((size_t)nconns * 4) + 3 * round16(n) +
                        2 * round16((size_t)n * 8) + round16((size_t)sb * 8) + 16;
    CallScratch* pool = nullptr;
    if (int rc = enter_pool(g_pool, need, s, &pool)) return rc;
    Params P{};
    P.rx = *rx, P.n = n, P.rows = rows, P.rxc = rx_conns, P.txc = tx_conns, P.dack = dack, P.nconns = nconns;
    P.action_in = action_in, P.links = links, P.nlinks = nlinks, P.now = now_ns;
    P.out = out, P.out_bytes = out_bytes, P.stride = layout->slot_stride, P.lead = layout->frame_lead;
    P.max_frames = max_frames, P.max_done = max_done, P.flags = flags, P.res = *res;
    Carver c{pool->scratch.p};
    P.t1 = c.take<uint32_t>(nconns);
    P.t2 = c.take<uint32_t>(nconns);
    uint8_t* zz = c.b;
    P.work = c.take<uint32_t>(nconns);
    P.sent = c.take<uint32_t>(nconns);
    P.tot = c.take<uint64_t>(2);
    P.s0 = c.take<uint32_t>(nconns);
    P.rn0 = c.take<uint32_t>(nconns);
    P.bits = c.take<uint8_t>(n);
    P.act = c.take<uint8_t>(n);
    P.sa = c.take<uint8_t>(n);
    P.flag_r = c.take<uint64_t>(n);
    P.flag_y = c.take<uint64_t>(n);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if ((ff_bytes && hipMemsetAsync(P.t1, 0xFF, ff_bytes, s) != hipSuccess) ||
        hipMemsetAsync(zz, 0, zero_bytes, s) != hipSuccess)
        return EIO;
    if (nconns) hipLaunchKernelGGL(cls_check_kernel, grid_for(nconns), dim3(kBlock), 0, s, P);
    if (n) {
        hipLaunchKernelGGL(cls_classify_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(cls_second_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(cls_decide_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, n, bsum, P.tot, s) || dk_tcp_tx_scan(P.flag_y, n, bsum, P.tot + 1, s)) return EIO;
        hipLaunchKernelGGL(cls_build_kernel, grid_for(n), dim3(kBlock), 0, s, P);
    }
    hipLaunchKernelGGL(cls_finish_kernel, grid_for(nconns), dim3(kBlock), 0, s, P);
    return pool->record(s);
}

int dk_tcp_close_timers(dk_tcp_closer* rows, dk_tcp_tx_conn* tx_conns, uint32_t nconns, uint64_t now_ns,
                        dk_tcp_cls_done* done, uint32_t max_done, uint32_t* n_done, uint32_t* status, void* stream) {
    using namespace dk_tcp_close;
    if (!n_done || (nconns && (!rows || !status || (max_done && !done)))) return EINVAL;
    if (misaligned(rows) || misaligned(tx_conns)) return EINVAL;
    std::lock_guard<std::mutex> lock(g_mutex);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t sb = dk_tcp_tx_scan_tiles(nconns);
    const size_t need = round16(2 * 8) + round16((size_t)nconns * 4) + round16((size_t)nconns * 8) +
                        round16((size_t)sb * 8) + 16;
    CallScratch* pool = nullptr;
    if (int rc = enter_pool(g_pool, need, s, &pool)) return rc;
    Params P{};
    P.rows = rows, P.txw = tx_conns, P.nconns = nconns, P.now = now_ns, P.max_done = max_done;
    P.res.done = done, P.res.n_done = n_done, P.st_status = status;
    Carver c{pool->scratch.p};
    P.tot = c.take<uint64_t>(2);
    P.work = c.take<uint32_t>(nconns);
    P.flag_y = c.take<uint64_t>(nconns);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if (hipMemsetAsync(P.tot, 0, 16, s) != hipSuccess) return EIO;
    if (nconns) {
        hipLaunchKernelGGL(cls_sweep_kernel, grid_for(nconns), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_y, nconns, bsum, P.tot + 1, s)) return EIO;
    }
    hipLaunchKernelGGL(cls_expire_kernel, grid_for(nconns), dim3(kBlock), 0, s, P);
    return pool->record(s);
}

}  // extern "C"
