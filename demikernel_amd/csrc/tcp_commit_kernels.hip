// tcp_commit_kernels.hip — dk_tcp_tx_commit and dk_tcp_rtx_piggyback (dk_tcp.h): the send side's bookkeeping after a
// dk_tcp_tx_segment / dk_tcp_retransmit call. Calls on a dk_tcp_tx_ctx, reached through dk_tcp_tx_ctx_serial
// (tcp_order.h).
//
// The commit is a per-connection decision (status, placement, the move of the live entries to the region's start)
// followed by one independent store per frame. The decision is always one wave per connection: the wave finds its
// buffers by binary search in the non-decreasing push.conn, sums frame_count over those that sent, tests the row and
// moves the live entries if the new ones do not fit behind them. The move overlaps with dest < src: it goes ascending
// in chunks of 64 entries, each chunk read whole (the stores wait for the wave's loads: their data) before it is
// written, so a chunk's stores never reach a later chunk's source.
//   conn form: the same wave then writes its k entries 64 at a time, and the row.
//   chip form: the wave leaves the connection's base (q_first' + q_count - its first frame) in the context's scratch;
//              a second kernel runs one lane per frame, bounded by the device's n_frames. The kernel boundary orders
//              the move's reads before the new entries, which may land on old source slots.
// An entry needs no running sum: every frame of a buffer but its last carries the same payload (mss bytes: a
// window-limited short frame closes the window, so nothing follows it), so the bytes of b's frames before f are
// (f - first_frame[b]) * (len_out[first_frame[b]] - 54). All stores are plain vector stores; no atomics, no fences.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>

#include "../../include/dk_diag.h"
#include "../../include/dk_tcp.h"
#include "tcp_order.h"

namespace dk_tcp_commit {
namespace {

constexpr int kBlock = 256;  // four waves: four connections (decide), 256 frames (entries)
constexpr uint32_t kWaves = kBlock / 64;
constexpr uint32_t kHeaders = 54;  // Ethernet + IPv4 + TCP without options: what dk_tcp_tx_segment puts in front
// The engine's rule ("dk_tcp_tx_commit"): the chip form from this many frame slots per connection on.
constexpr uint64_t kChipSlotsPerConn = 1024;

struct Params {
    dk_tcp_tx_push push;
    dk_tcp_tx_results res;
    uint32_t nbufs, max_frames;
    dk_tcp_ack_conn* ak;
    uint32_t nconns;
    dk_tcp_unacked q;
    uint32_t q_cap;
    dk_tcp_dack_conn* dack;
    uint64_t now;
    dk_tcp_commit_out out;
    uint2* base;  // [nconns] chip form: {pool index of frame 0 (wrapping), 1 iff the connection appends}
};

__device__ __forceinline__ bool sent_status(uint32_t st) { return st == DK_TCP_TX_SENT || st == DK_TCP_TX_PARTIAL; }

// Entry pool[pos] for frame f. f < max_frames and frame_buf[f] < nbufs hold for a frame a fitting call wrote; they are
// tested all the same, so that results that are not that call's cannot make the kernel read out of bounds.
__device__ __forceinline__ void write_entry(const Params& P, uint32_t f, uint32_t pos) {
    uint32_t off = 0, len = 0;
    if (f < P.max_frames) {
        const uint32_t b = P.res.frame_buf[f];
        len = (uint32_t)P.res.len_out[f] - kHeaders;
        if (b < P.nbufs) {
            const uint32_t ff = min(P.res.first_frame[b], f);
            off = P.push.off[b] + (f - ff) * ((uint32_t)P.res.len_out[ff] - kHeaders);
        }
    }
    P.q.off[pos] = off;
    P.q.len[pos] = len;
    P.q.tx_time[pos] = P.now;
}

template <bool kEntries>
__global__ __launch_bounds__(kBlock) void dk_tcp_commit_conn_kernel(Params P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * kWaves + (threadIdx.x >> 6);  // wave-uniform
    if (c >= P.nconns) return;
    // the connection's buffers start at the first index with push.conn >= c
    uint32_t lo = 0, hi = P.nbufs;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (P.push.conn[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    uint64_t k64 = 0;
    uint32_t f0 = 0xFFFFFFFFu;  // the connection's first frame: its frames are consecutive
    for (uint32_t b0 = lo; b0 < P.nbufs; b0 += 64) {
        const uint32_t b = b0 + lane;
        const bool mine = b < P.nbufs && P.push.conn[b] == c;
        if (mine && sent_status(P.res.status[b])) {
            k64 += P.res.frame_count[b];
            f0 = min(f0, P.res.first_frame[b]);
        }
        if (__ballot(mine) != ~0ull) break;
    }
    for (int o = 32; o; o >>= 1) {
        k64 += __shfl_xor(k64, o);
        f0 = min(f0, __shfl_xor(f0, o));
    }
    uint32_t status = DK_TCP_COMMIT_OK, appended = 0;
    uint2 base = make_uint2(0, 0);
    if (k64) {
        dk_tcp_ack_conn& A = P.ak[c];
        const uint64_t qf = A.q_first, qc = A.q_count, armed = A.rtx_armed;
        const uint64_t r0 = (uint64_t)c * P.q_cap, r1 = r0 + P.q_cap;  // the region; nconns * q_cap <= nq fits 32 bits
        if (qc > P.q_cap || (qc && (qf < r0 || qf + qc > r1))) status = DK_TCP_COMMIT_E_QUEUE;
        else if (qc + k64 > P.q_cap) status = DK_TCP_COMMIT_E_FULL;
        else {
            const uint32_t k = (uint32_t)k64, n = (uint32_t)qc;
            uint32_t first = (uint32_t)qf;
            if (n == 0) first = (uint32_t)r0;
            else if (qf + qc + k64 > r1) {
                const uint32_t src = first, dst = (uint32_t)r0;
                for (uint32_t i0 = 0; i0 < n; i0 += 64) {
                    const uint32_t i = i0 + lane;
                    uint32_t off = 0, len = 0;
                    uint64_t tt = 0;
                    if (i < n) off = P.q.off[src + i], len = P.q.len[src + i], tt = P.q.tx_time[src + i];
                    if (i < n) P.q.off[dst + i] = off, P.q.len[dst + i] = len, P.q.tx_time[dst + i] = tt;
                }
                first = dst;
            }
            const uint32_t at = first + n;  // the first new entry
            if (kEntries) {
                for (uint32_t j0 = 0; j0 < k; j0 += 64)
                    if (j0 + lane < k) write_entry(P, f0 + j0 + lane, at + j0 + lane);
            }
            base = make_uint2(at - f0, 1);
            appended = k;
            if (lane == 0) {
                A.q_first = first;
                A.q_count = n + k;
                if (!armed) {
                    A.rtx_armed = 1;
                    A.rtx_base_ns = P.now;
                }
            }
        }
        if (lane == 0 && P.dack) P.dack[c].armed = 0;  // the frames left and carried the ACK, whatever the status
    }
    if (lane == 0) {
        P.out.status[c] = status;
        P.out.appended[c] = appended;
        if (!kEntries) P.base[c] = base;
    }
}

// Chip form, second kernel: one lane per frame of the call.
__global__ __launch_bounds__(kBlock) void dk_tcp_commit_frames_kernel(Params P) {
    const uint32_t n = min(*P.res.n_frames, P.max_frames);
    for (uint32_t f = blockIdx.x * kBlock + threadIdx.x; f < n; f += gridDim.x * kBlock) {
        const uint32_t b = P.res.frame_buf[f];
        if (b >= P.nbufs || !sent_status(P.res.status[b])) continue;  // a call without room wrote no frame_buf
        const uint32_t ff = P.res.first_frame[b], c = P.push.conn[b];
        if (f < ff || f - ff >= P.res.frame_count[b] || c >= P.nconns) continue;
        const uint2 base = P.base[c];
        const uint32_t pos = base.x + f;
        if (!base.y || pos / P.q_cap != c) continue;  // a failed connection; the second test never fires on a call's own results
        write_entry(P, f, pos);
    }
}

__global__ __launch_bounds__(kBlock) void dk_tcp_rtx_piggyback_kernel(const uint32_t* status, dk_tcp_dack_conn* dack,
                                                                      uint32_t nconns) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c < nconns && status[c] == DK_TCP_RTX_SENT) dack[c].armed = 0;
}

using dk::ctl::DeviceGuard;

bool misaligned(const void* a, const void* b) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) != 0;
}

}  // namespace
}  // namespace dk_tcp_commit

extern "C" {

int dk_diag_tcp_commit_set_form(dk_tcp_tx_ctx* t, int32_t form) {
    dk_tcp_tx_serial o;
    if (dk_tcp_tx_ctx_serial(t, &o) || form < -1 || form > 1) return EINVAL;
    o.commit->form = form;
    return 0;
}

int dk_diag_tcp_commit_last_form(const dk_tcp_tx_ctx* t) {
    dk_tcp_tx_serial o;
    return dk_tcp_tx_ctx_serial(const_cast<dk_tcp_tx_ctx*>(t), &o) ? -1 : o.commit->last_form;
}

int dk_tcp_tx_commit(dk_tcp_tx_ctx* t, const dk_tcp_tx_push* push, uint32_t nbufs, const dk_tcp_tx_results* res,
                     uint32_t max_frames, dk_tcp_ack_conn* ack_conns, uint32_t nconns, const dk_tcp_unacked* q,
                     uint32_t nq, uint32_t q_cap, dk_tcp_dack_conn* dack, uint64_t now_ns, const dk_tcp_commit_out* out,
                     void* stream) {
    using namespace dk_tcp_commit;
    dk_tcp_tx_serial o;
    if (dk_tcp_tx_ctx_serial(t, &o) || !push || !res || !q || !out) return EINVAL;
    if (now_ns == DK_TCP_TX_TIME_NONE || (uint64_t)nconns * q_cap > nq) return EINVAL;
    if (misaligned(ack_conns, dack)) return EINVAL;
    if (nbufs && (!push->conn || !push->off || !res->first_frame || !res->frame_count || !res->status || !res->n_frames))
        return EINVAL;
    if (nbufs && max_frames && (!res->len_out || !res->frame_buf)) return EINVAL;
    if (nconns && (!ack_conns || !out->status || !out->appended)) return EINVAL;
    if (nconns && q_cap && (!q->off || !q->len || !q->tx_time)) return EINVAL;
    // in turn: once after a dk_tcp_tx_segment call of this context, with its nbufs
    dk_tcp_commit_state& st = *o.commit;
    if (st.seg_call == 0 || st.done == st.seg_call || nbufs != st.seg_nbufs) return EINVAL;
    st.last_form = -1;
    int form = st.form;
    if (form < 0) form = (uint64_t)max_frames >= kChipSlotsPerConn * std::max(nconns, 1u) ? 1 : 0;
    if (nbufs == 0 || max_frames == 0) form = 0;  // no frame to write
    if (nconns == 0) {
        st.done = st.seg_call;
        return 0;
    }
    DeviceGuard g(o.device);
    const hipStream_t s = (hipStream_t)stream;
    if (form == 1)
        if (int rc = st.scratch.grow(*o.serial, nconns)) return rc;
    st.done = st.seg_call;
    if (o.serial->order(s)) return EIO;
    Params P{{}, {}, nbufs, max_frames, ack_conns, nconns, *q, q_cap, dack, now_ns, *out, st.scratch.p};
    if (nbufs) P.push = *push, P.res = *res;
    const dim3 per_conn((nconns + kWaves - 1) / kWaves);
    if (form == 1) {
        hipLaunchKernelGGL(dk_tcp_commit_conn_kernel<false>, per_conn, dim3(kBlock), 0, s, P);
        const uint32_t grid = std::min<uint32_t>((max_frames + kBlock - 1) / kBlock, 8u * std::max(o.cus, 1u));
        hipLaunchKernelGGL(dk_tcp_commit_frames_kernel, dim3(grid), dim3(kBlock), 0, s, P);
    } else {
        hipLaunchKernelGGL(dk_tcp_commit_conn_kernel<true>, per_conn, dim3(kBlock), 0, s, P);
    }
    if (hipGetLastError() != hipSuccess) return EIO;
    st.last_form = form;
    return o.serial->record(s);
}

int dk_tcp_rtx_piggyback(dk_tcp_tx_ctx* t, const dk_tcp_rtx_results* res, dk_tcp_dack_conn* dack, uint32_t nconns,
                         void* stream) {
    using namespace dk_tcp_commit;
    dk_tcp_tx_serial o;
    if (dk_tcp_tx_ctx_serial(t, &o) || !res) return EINVAL;
    if (nconns && (!res->status || !dack)) return EINVAL;
    if (misaligned(dack, nullptr)) return EINVAL;
    if (nconns == 0) return 0;
    DeviceGuard g(o.device);
    const hipStream_t s = (hipStream_t)stream;
    if (o.serial->order(s)) return EIO;
    hipLaunchKernelGGL(dk_tcp_rtx_piggyback_kernel, dim3((nconns + kBlock - 1) / kBlock), dim3(kBlock), 0, s, res->status,
                       dack, nconns);
    return o.serial->record(s);
}

}  // extern "C"
