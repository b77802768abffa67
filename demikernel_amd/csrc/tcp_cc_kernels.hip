// tcp_cc_kernels.hip — CUBIC congestion control and timer expiry on the GPU (include/dk_tcp.h: dk_tcp_cc_ack,
// dk_tcp_timers, dk_tcp_cc_send).
//
// established/congestion_control/cubic.rs restated, one lane per connection, with the connection's Cubic in
// registers: the literal on_ack_received loop over the connection's segments in the order dk_tcp_rx_process left in
// its context (tcp_order.h), on_rto / on_fast_retransmit behind the sweep of the retransmit deadlines, and the two
// send hooks around dk_tcp_tx_segment. The lane form is the specification in code; a parallel form of dk_tcp_cc_ack
// is future work (a connection's segments are a chain through cwnd, but long runs of slow start and of duplicates
// beyond the fourth are sums). The arithmetic rules (wrapping u32, Rust's casts, f32 rounded once per operation, the
// exact Duration conversion, the correctly rounded cube root) are tcp_cc_math.h's.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

#include "../../include/dk_diag.h"
#include "../../include/dk_tcp.h"
#include "tcp_cc_math.h"
#include "tcp_order.h"

static_assert(sizeof(dk_tcp_cc_conn) == 64 && offsetof(dk_tcp_cc_conn, ca_start_ns) == 40, "dk_tcp_cc_conn layout");

namespace dk_tcp_cc {
namespace {

constexpr uint32_t kBlock = 64;
constexpr float kBeta = 0.7f, kC = 0.4f;  // BETA_CUBIC, C (cubic.rs:108-110)
constexpr uint32_t kDupThreshold = 3;     // DUP_ACK_THRESHOLD (cubic.rs:111)

__device__ __forceinline__ bool seq_gt(uint32_t a, uint32_t b) { return (int32_t)(a - b) > 0; }

// The connection's Cubic (cubic.rs:37-59) in registers; mss from the TX table.
struct Cubic {
    uint32_t flags, cwnd, ssthresh, w_max, initial_cwnd, ltci, dup_acks, rpif, recover, prev_ack;
    uint64_t ca_start, last_send, rtt_at_last_send;
    uint32_t mss;

    __device__ __forceinline__ bool has(uint32_t f) const { return (flags & f) != 0; }
    __device__ __forceinline__ void set(uint32_t f, bool on) { flags = on ? flags | f : flags & ~f; }

    __device__ __forceinline__ void load(const dk_tcp_cc_conn& r, uint32_t mss_) {
        flags = r.flags, cwnd = r.cwnd, ssthresh = r.ssthresh, w_max = r.w_max, initial_cwnd = r.initial_cwnd;
        ltci = r.ltci, dup_acks = r.dup_acks, rpif = r.rpif, recover = r.recover, prev_ack = r.prev_ack;
        ca_start = r.ca_start_ns, last_send = r.last_send_ns, rtt_at_last_send = r.rtt_at_last_send_ns;
        mss = mss_;
    }
    __device__ __forceinline__ void store(dk_tcp_cc_conn& r) const {
        r.flags = flags, r.cwnd = cwnd, r.ssthresh = ssthresh, r.w_max = w_max, r.initial_cwnd = initial_cwnd;
        r.ltci = ltci, r.dup_acks = dup_acks, r.rpif = rpif, r.recover = recover, r.prev_ack = prev_ack;
        r.ca_start_ns = ca_start, r.last_send_ns = last_send, r.rtt_at_last_send_ns = rtt_at_last_send;
    }

    // cubic.rs:113-123
    __device__ __forceinline__ void fast_convergence() {
        if (cwnd / mss < w_max / mss) {
            const float f = (float)cwnd * (1.0f + kBeta);
            w_max = dk_cc::f32_as_u32(f / 2.0f);
        } else {
            w_max = cwnd;
        }
    }

    // cubic.rs:125-165
    __device__ __forceinline__ void on_dup_ack(uint32_t snd_nxt, uint32_t ack) {
        dup_acks += 1;
        if (dup_acks < kDupThreshold) ltci += mss;
        const uint32_t diff = ack - prev_ack;
        const bool covers = seq_gt(ack - 1u, recover);
        const bool dropped = cwnd > mss && diff <= 4u * mss;
        if (dup_acks == kDupThreshold && (covers || dropped)) {
            set(DK_TCP_CC_IN_RECOVERY, true);
            recover = snd_nxt;
            const uint32_t reduced = dk_cc::f32_as_u32((float)cwnd * kBeta);
            if (has(DK_TCP_CC_FAST_CONVERGENCE)) fast_convergence();
            else w_max = cwnd;
            ssthresh = max(reduced, 2u * mss);
            cwnd = reduced;
            set(DK_TCP_CC_RETRANSMIT_NOW, true);
        } else if (dup_acks > kDupThreshold || has(DK_TCP_CC_IN_RECOVERY)) {
            cwnd += mss;
        }
    }

    // cubic.rs:167-192
    __device__ __forceinline__ void on_ack_fast_recovery(uint32_t una, uint32_t snd_nxt, uint32_t ack, uint64_t now) {
        const uint32_t outstanding = snd_nxt - una, acked = ack - una;
        if (seq_gt(ack, recover)) {  // full acknowledgement
            cwnd = min(ssthresh, max(outstanding, mss) + mss);
            ca_start = now;
            set(DK_TCP_CC_LAST_WAS_RTO, false);
            set(DK_TCP_CC_IN_RECOVERY, false);
        } else {  // partial
            set(DK_TCP_CC_RETRANSMIT_NOW, true);
            if (acked >= mss) cwnd = cwnd - acked + mss;
            else cwnd = cwnd - acked;
        }
    }

    // cubic.rs:194-215
    __device__ __forceinline__ float k_of(float w) const {
        if (has(DK_TCP_CC_LAST_WAS_RTO)) return 0.0f;
        const float a = w * (1.0f - kBeta);
        return dk_cc::cbrt_f32(a / kC);
    }
    __device__ __forceinline__ static float w_cubic(float w, float t, float k) {
        const float d = t - k, d2 = d * d, d3 = d2 * d;  // powi(3)
        const float c = kC * d3;
        return c + w;
    }
    __device__ __forceinline__ static float w_est(float w, float t, float rtt) {
        const float num = 3.0f * (1.0f - kBeta), den = 1.0f + kBeta, coef = num / den;  // folded in f32
        const float a = w * kBeta, b = coef * t, q = b / rtt;
        return a + q;
    }

    // cubic.rs:217-246
    __device__ __forceinline__ void on_ack_ss_ca(float rtt, uint32_t una, uint32_t ack, uint64_t now) {
        const uint32_t acked = ack - una;
        if (cwnd < ssthresh) {
            cwnd += min(acked, mss);
            return;
        }
        const float t = dk_cc::as_secs_f32(now > ca_start ? now - ca_start : 0ull);
        const float mss_f = (float)mss, w = (float)w_max / mss_f;
        const float k = k_of(w), est = w_est(w, t, rtt);
        if (w_cubic(w, t, k) < est) {
            cwnd = dk_cc::f32_as_u32(est * mss_f);
        } else {
            const float ncwnd = (float)cwnd / mss_f;
            const float target = w_cubic(w, t + rtt, k);
            const float over = target - ncwnd, rel = over / ncwnd;
            cwnd += dk_cc::f32_as_u32(rel * mss_f);
        }
    }

    // cubic.rs:307-328
    __device__ __forceinline__ void on_ack_received(float rtt, uint32_t una, uint32_t snd_nxt, uint32_t ack, uint64_t now) {
        if (ack - una == 0) {
            on_dup_ack(snd_nxt, ack);
            rpif = rpif ? rpif - 1 : 0;
        } else {
            dup_acks = 0;
            if (has(DK_TCP_CC_IN_RECOVERY)) on_ack_fast_recovery(una, snd_nxt, ack, now);
            else on_ack_ss_ca(rtt, una, ack, now);
            prev_ack = ack;
        }
    }

    // cubic.rs:248-278, :330-334
    __device__ __forceinline__ void on_rto(uint32_t una) {
        const uint32_t old = cwnd;
        if (has(DK_TCP_CC_FAST_CONVERGENCE)) fast_convergence();
        else w_max = old;
        cwnd = mss;
        if (rpif == 0) ssthresh = max(dk_cc::f32_as_u32((float)old * kBeta), 2u * mss);
        rpif += 1;
        set(DK_TCP_CC_LAST_WAS_RTO, true);
        recover = una;
        set(DK_TCP_CC_IN_RECOVERY, false);
    }
};

__device__ __forceinline__ bool visited(uint32_t a) {
    return a == DK_TCP_DELIVERED || a == DK_TCP_STORED || a == DK_TCP_STORE_DUP || a == DK_TCP_NO_DATA ||
           a == DK_TCP_FIN || a == DK_TCP_ACK_UNSENT;
}

struct AckParams {
    const uint32_t* svals;
    const uint32_t* range;
    const uint4* rec;
    const uint8_t* action;
    const dk_tcp_conn* rx;
    dk_tcp_tx_conn* tx;
    const dk_tcp_ack_conn* ak;
    dk_tcp_cc_conn* cc;
    uint32_t nconns;
    uint64_t now;
    dk_tcp_cc_ack_out out;
};

__global__ __launch_bounds__(kBlock) void dk_tcp_cc_ack_kernel(AckParams P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= P.nconns) return;
    const dk_tcp_tx_conn& t = P.tx[c];
    const uint32_t snd_nxt = t.snd_nxt, mss = t.mss, flags = P.cc[c].flags;
    const double rto = P.ak[c].rto;
    uint32_t st = DK_TCP_CC_OK;
    if (t.state != DK_TCP_ESTABLISHED) st = DK_TCP_CC_E_STATE;
    else if (P.rx[c].send_next != snd_nxt) st = DK_TCP_CC_E_SND_NXT;
    else if (!(flags & DK_TCP_CC_CUBIC)) st = DK_TCP_CC_OK;
    else if (mss == 0) st = DK_TCP_CC_E_MSS;
    else if (!dk_cc::rto_valid(rto)) st = DK_TCP_CC_E_RTO;
    P.out.status[c] = st;
    uint32_t new_acks = 0, dups = 0;
    if (st == DK_TCP_CC_OK && (flags & DK_TCP_CC_CUBIC)) {
        Cubic k;
        k.load(P.cc[c], mss);
        const float rtt = dk_cc::as_secs_f32(dk_cc::rto_ns(rto));
        uint32_t una = t.snd_una;
        const uint32_t r0 = P.range[2 * c], r1 = P.range[2 * c + 1];
        for (uint32_t p = r0; p < r1; p++) {
            const uint32_t i = P.svals[p], act = P.action[i];
            if (!visited(act)) continue;
            const uint32_t ack = P.rec[i].y;
            if (ack == una) dups++;
            else new_acks++;
            k.on_ack_received(rtt, una, snd_nxt, ack, P.now);
            if (P.out.cwnd_after) P.out.cwnd_after[i] = k.cwnd;
            // Sender::process_ack moves SND.UNA (sender.rs:406-474); an ACK of unsent data never reaches it
            if (act != DK_TCP_ACK_UNSENT && ack - una - 1u < 0x7FFFFFFFu) una = ack;
        }
        k.store(P.cc[c]);
        P.tx[c].cwnd = k.cwnd + k.ltci;
    }
    P.out.new_acks[c] = new_acks;
    P.out.dup_acks[c] = dups;
}

struct TimerParams {
    dk_tcp_tx_conn* tx;
    const dk_tcp_ack_conn* ak;
    dk_tcp_cc_conn* cc;
    const dk_tcp_dack_conn* dack;
    uint32_t nconns;
    uint64_t now;
    uint8_t* rtx_fire;
    uint8_t* ack_fire;
    dk_tcp_timers_out out;
};

// the wave's count of lanes with `on`, added once
__device__ __forceinline__ void count(bool on, uint32_t* word) {
    const unsigned long long m = __ballot(on);
    if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(word, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(kBlock) void dk_tcp_timers_kernel(TimerParams P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    const bool live = c < P.nconns;
    uint32_t fire = DK_TCP_RTX_NONE;
    bool afire = false;
    if (live) {
        const dk_tcp_tx_conn& t = P.tx[c];
        const dk_tcp_ack_conn& a = P.ak[c];
        const uint32_t flags = P.cc[c].flags, mss = t.mss;
        const bool cubic = (flags & DK_TCP_CC_CUBIC) != 0;
        const double rto = a.rto;
        uint32_t st = DK_TCP_CC_OK;
        if (t.state != DK_TCP_ESTABLISHED) st = DK_TCP_CC_E_STATE;
        else if (cubic && mss == 0) st = DK_TCP_CC_E_MSS;
        else if (!dk_cc::rto_valid(rto)) st = DK_TCP_CC_E_RTO;
        P.out.status[c] = st;
        if (st == DK_TCP_CC_OK) {
            const uint64_t d = dk_cc::rto_ns(rto), base = a.rtx_base_ns;
            const uint64_t deadline = base + d < base ? ~0ull : base + d;
            if (cubic && (flags & DK_TCP_CC_RETRANSMIT_NOW)) fire = DK_TCP_RTX_FAST;
            else if (a.rtx_armed && P.now >= deadline) fire = DK_TCP_RTX_TIMEOUT;
            if (cubic) {
                Cubic k;
                k.load(P.cc[c], mss);
                if (fire == DK_TCP_RTX_FAST) k.set(DK_TCP_CC_RETRANSMIT_NOW, false);  // on_fast_retransmit
                else if (fire == DK_TCP_RTX_TIMEOUT) k.on_rto(t.snd_una);
                if (fire != DK_TCP_RTX_NONE) k.store(P.cc[c]);
                P.tx[c].cwnd = k.cwnd + k.ltci;
            }
        }
        P.rtx_fire[c] = (uint8_t)fire;
        if (P.ack_fire) {
            afire = P.dack[c].armed != 0 && P.now >= P.dack[c].deadline_ns;
            P.ack_fire[c] = afire ? 1 : 0;
        }
    }
    count(fire == DK_TCP_RTX_FAST, P.out.n_fast);
    count(fire == DK_TCP_RTX_TIMEOUT, P.out.n_timeout);
    count(afire, P.out.n_ack);
}

struct SendParams {
    dk_tcp_tx_conn* tx;
    const dk_tcp_ack_conn* ak;
    dk_tcp_cc_conn* cc;
    uint32_t nconns, nbufs, phase;
    uint64_t now;
    dk_tcp_tx_push push;
    dk_tcp_tx_results res;
    uint32_t* status;
};

__global__ __launch_bounds__(kBlock) void dk_tcp_cc_send_kernel(SendParams P) {
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= P.nconns) return;
    dk_tcp_cc_conn& row = P.cc[c];
    const dk_tcp_tx_conn& t = P.tx[c];
    const bool cubic = (row.flags & DK_TCP_CC_CUBIC) != 0;
    if (t.state != DK_TCP_ESTABLISHED) {
        P.status[c] = DK_TCP_CC_E_STATE;
        return;
    }
    P.status[c] = DK_TCP_CC_OK;
    if (!cubic) return;
    if (P.phase == DK_TCP_CC_BEFORE_SEND) {  // cubic.rs:290-298
        const uint64_t last = row.last_send_ns, idle = P.now > last ? P.now - last : 0ull;
        uint32_t cwnd = row.cwnd, ltci = row.ltci;
        if (idle > row.rtt_at_last_send_ns) {
            cwnd = min(row.initial_cwnd, cwnd), ltci = 0;
            row.cwnd = cwnd, row.ltci = 0;
        }
        P.tx[c].cwnd = cwnd + ltci;
        return;
    }
    // the connection's buffers push.conn[b0 .. b1): conn is non-decreasing
    uint32_t lo = 0, hi = P.nbufs;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (P.push.conn[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t b0 = lo;
    uint32_t consumed = 0, frames = 0, b1 = b0;
    for (; b1 < P.nbufs && P.push.conn[b1] == c; b1++) {
        const uint32_t s = P.res.status[b1];
        if ((s == DK_TCP_TX_SENT || s == DK_TCP_TX_PARTIAL) && P.res.sent[b1]) {
            consumed += P.res.sent[b1];
            frames += P.res.frame_count[b1];
        }
    }
    if (!frames) return;
    const double rto = P.ak[c].rto;
    if (!dk_cc::rto_valid(rto)) {
        P.status[c] = DK_TCP_CC_E_RTO;
        return;
    }
    // on_send per frame (cubic.rs:300-305), given SND.NXT - SND.UNA as it stands before the frame (sender.rs:177)
    uint32_t ltci = row.ltci;
    uint32_t flight = (t.snd_nxt - consumed) - t.snd_una;
    const uint32_t nf = *P.res.n_frames;  // a call that sent anything fitted: its frames are [0, n_frames)
    for (uint32_t b = b0; b < b1 && ltci; b++) {
        const uint32_t s = P.res.status[b];
        if (!((s == DK_TCP_TX_SENT || s == DK_TCP_TX_PARTIAL) && P.res.sent[b])) continue;
        const uint32_t f0 = P.res.first_frame[b], f1 = min(f0 + P.res.frame_count[b], nf);
        for (uint32_t f = f0; f < f1 && ltci; f++) {
            ltci = ltci > flight ? ltci - flight : 0u;
            const uint32_t bytes = (uint32_t)P.res.len_out[f] - 54u;
            flight += bytes ? bytes : 1u;  // the end-of-send marker's FIN takes one number
        }
    }
    row.last_send_ns = P.now;
    row.rtt_at_last_send_ns = dk_cc::rto_ns(rto);
    row.ltci = ltci;
    P.tx[c].cwnd = row.cwnd + ltci;
}

__global__ __launch_bounds__(256) void dk_tcp_cc_cbrt_kernel(const float* in, float* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = dk_cc::cbrt_f32(in[i]);
}

using dk::ctl::DeviceGuard;

bool misaligned(const void* a, const void* b, const void* c, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) != 0;
}

}  // namespace
}  // namespace dk_tcp_cc

extern "C" {

uint64_t dk_tcp_rto_ns(double rto) { return dk_cc::rto_ns(rto); }

int dk_diag_tcp_cc_cbrt(const float* in, float* out, uint32_t n, void* stream) {
    if (n && (!in || !out)) return EINVAL;
    if (n) hipLaunchKernelGGL(dk_tcp_cc::dk_tcp_cc_cbrt_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, in, out, n);
    return !n || hipGetLastError() == hipSuccess ? 0 : EIO;
}

int dk_tcp_cc_ack(dk_tcp_ctx* t, const dk_rx_results* rx, uint32_t n, const uint8_t* action, const dk_tcp_conn* rx_conns,
                  dk_tcp_tx_conn* tx_conns, const dk_tcp_ack_conn* ack_conns, dk_tcp_cc_conn* cc, uint32_t nconns,
                  uint64_t now_ns, const dk_tcp_cc_ack_out* out, void* stream) {
    using namespace dk_tcp_cc;
    dk_tcp_order o;
    if (dk_tcp_ctx_order(t, &o) || !rx || !out) return EINVAL;
    if (n && !action) return EINVAL;
    if (nconns && (!rx_conns || !tx_conns || !ack_conns || !cc || !out->status || !out->new_acks || !out->dup_acks))
        return EINVAL;
    if (misaligned(tx_conns, ack_conns, cc, rx_conns)) return EINVAL;
    // in turn: after the dk_tcp_rx_process call of this context whose order it reuses, once, and before that batch's
    // dk_tcp_ack_process moves snd_una and rto
    if (!o.live || o.call == 0 || o.cc->done == o.call || o.ack->done == o.call || n != o.n || nconns != o.nconns)
        return EINVAL;
    o.cc->done = o.call;
    if (n == 0 && nconns == 0) return 0;
    DeviceGuard g(o.device);
    const hipStream_t s = (hipStream_t)stream;
    if (o.serial->order(s)) return EIO;
    if (n && out->cwnd_after && hipMemsetAsync(out->cwnd_after, 0, (size_t)n * sizeof(uint32_t), s) != hipSuccess)
        return EIO;
    if (nconns) {
        AckParams P{o.svals, o.range, o.rec, action, rx_conns, tx_conns, ack_conns, cc, nconns, now_ns, *out};
        hipLaunchKernelGGL(dk_tcp_cc_ack_kernel, dim3((nconns + kBlock - 1) / kBlock), dim3(kBlock), 0, s, P);
    }
    return o.serial->record(s);
}

int dk_tcp_timers(dk_tcp_tx_ctx* t, dk_tcp_tx_conn* tx_conns, const dk_tcp_ack_conn* ack_conns, dk_tcp_cc_conn* cc,
                  const dk_tcp_dack_conn* dack, uint32_t nconns, uint64_t now_ns, uint8_t* rtx_fire, uint8_t* ack_fire,
                  const dk_tcp_timers_out* out, void* stream) {
    using namespace dk_tcp_cc;
    dk_tcp_tx_serial o;
    if (dk_tcp_tx_ctx_serial(t, &o) || !out || !out->n_fast || !out->n_timeout || !out->n_ack) return EINVAL;
    if (nconns && (dack != nullptr) != (ack_fire != nullptr)) return EINVAL;
    if (nconns && (!tx_conns || !ack_conns || !cc || !rtx_fire || !out->status)) return EINVAL;
    if (misaligned(tx_conns, ack_conns, cc, dack)) return EINVAL;
    DeviceGuard g(o.device);
    const hipStream_t s = (hipStream_t)stream;
    if (o.serial->order(s)) return EIO;
    if (hipMemsetAsync(out->n_fast, 0, sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(out->n_timeout, 0, sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(out->n_ack, 0, sizeof(uint32_t), s) != hipSuccess)
        return EIO;
    if (nconns) {
        TimerParams P{tx_conns, ack_conns, cc, dack, nconns, now_ns, rtx_fire, ack_fire, *out};
        hipLaunchKernelGGL(dk_tcp_timers_kernel, dim3((nconns + kBlock - 1) / kBlock), dim3(kBlock), 0, s, P);
    }
    return o.serial->record(s);
}

int dk_tcp_cc_send(dk_tcp_tx_ctx* t, uint32_t phase, dk_tcp_tx_conn* tx_conns, const dk_tcp_ack_conn* ack_conns,
                   dk_tcp_cc_conn* cc, uint32_t nconns, const dk_tcp_tx_push* push, uint32_t nbufs,
                   const dk_tcp_tx_results* res, uint64_t now_ns, uint32_t* status, void* stream) {
    using namespace dk_tcp_cc;
    dk_tcp_tx_serial o;
    if (dk_tcp_tx_ctx_serial(t, &o) || phase > DK_TCP_CC_AFTER_SEND) return EINVAL;
    if (nconns && (!tx_conns || !ack_conns || !cc || !status)) return EINVAL;
    if (misaligned(tx_conns, ack_conns, cc)) return EINVAL;
    const bool after = phase == DK_TCP_CC_AFTER_SEND;
    if (after && nbufs &&
        (!push || !res || !push->conn || !res->sent || !res->first_frame || !res->frame_count || !res->status ||
         !res->len_out || !res->n_frames))
        return EINVAL;
    DeviceGuard g(o.device);
    const hipStream_t s = (hipStream_t)stream;
    if (o.serial->order(s)) return EIO;
    if (nconns) {
        SendParams P{tx_conns, ack_conns, cc, nconns, after ? nbufs : 0u, phase, now_ns, {}, {}, status};
        if (after && nbufs) P.push = *push, P.res = *res;
        hipLaunchKernelGGL(dk_tcp_cc_send_kernel, dim3((nconns + kBlock - 1) / kBlock), dim3(kBlock), 0, s, P);
    }
    return o.serial->record(s);
}

}  // extern "C"
