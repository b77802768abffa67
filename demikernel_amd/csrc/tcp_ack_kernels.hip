// tcp_ack_kernels.hip — the sender's reaction to ACKs on the GPU (include/dk_tcp.h, dk_tcp_ack_process).
//
// ControlBlock::process_ack (ctrlblk.rs:607-650) -> Sender::process_ack (sender.rs:406-474), per connection over the
// segments of a batch that dk_tcp_rx_process let through (DELIVERED, STORED, STORE_DUP, NO_DATA, FIN), in the arrival
// order that call's sort left in its context (tcp_order.h). Connections are independent; within one, SND.UNA, the
// window-update pair and the unacknowledged queue are sequential state.
//   dk_tcp_ack_lane_kernel: one lane per connection, the literal loop over segments and queue entries (serial_conn):
//      the specification in code, and the form for many connections with few segments each.
//   dk_tcp_ack_wave_kernel: one wave per connection, 64 segments a step. With o(x) = (int32)(x - SND.NXT), every
//      accepted ack has o in [-2^31, 0] and SND.UNA only moves up in that order, so "new ACK" is "above the running
//      maximum before me": one max-scan. Among new ACKs wl2 <= ack always holds (wl2 <= SND.UNA in the same order,
//      checked), so update_send_window's rule is wl1 <= seq, a running maximum of seq from wl1, and the segment whose
//      window is kept is the last new ACK that attains the maximum: a reduction. The queue is popped once by the total
//      advance: 64 entries a step, a prefix sum of their lengths, their RTT samples converted in parallel and folded
//      in queue order (the EWMA and its fabs do not reassociate bit-exactly). Nothing is committed before the queue is
//      known to cover the advance. Where an assumption fails on the device — wl2 outside (SND.NXT - 2^31, SND.NXT], a
//      sequence number outside (wl1 - 2^29, wl1 + 3 * 2^29), a marker that is not exactly the last byte of the pop, a dry queue —
//      lane 0 redoes the connection with serial_conn.
// f64 arithmetic is the reference's operation by operation: contraction is off for this file.
#include <hip/hip_runtime.h>
#include <rocprim/warp/warp_scan.hpp>

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdint>

#include "../../include/dk_diag.h"
#include "../../include/dk_tcp.h"
#include "tcp_order.h"

#pragma clang fp contract(off)

namespace dk_tcp_ack {
namespace {

constexpr uint32_t kWave = 64;
constexpr uint64_t kNone = DK_TCP_TX_TIME_NONE;
// the walks' own thresholds: one wave per connection from 8 segments per connection (tcp_kernels.hip kWaveWalkMinSegs);
// the chip form where the scan walk runs, from 1,024 segments per connection up to 256 connections (kScanMinSegs,
// DK_TCP_SCAN_MAX_CONNS)
constexpr uint32_t kWaveMinSegs = 8, kChipMinSegs = 1024, kChipMaxConns = 256;

struct Params {
    const uint32_t* svals;
    const uint32_t* range;
    const uint4* rec;
    const uint32_t* win;
    const uint8_t* action;
    const dk_tcp_conn* rx_conns;
    dk_tcp_tx_conn* tx;
    dk_tcp_ack_conn* ak;
    uint32_t nconns;
    dk_tcp_unacked q;
    uint32_t nq;
    uint64_t now;
    dk_tcp_ack_out out;
    // the chip form's scratch: window v of connection c at slot range[2c] / 64 + c + v (disjoint per connection)
    uint4* wpart;   // [slots] {max of seq - wl1 over the window's new ACKs, seq, ack, win of the last that attains it}
    uint2* wcnt;    // [slots] {new ACKs, duplicate ACKs} (before the scan: {a sequence number out of bounds, -})
    int* wmax;      // [slots] the window's maximum of o(ack) over its processed segments
    int* wcarry;    // [slots] o(SND.UNA) as the window finds it
    int2* cstate;   // [nconns] {o(SND.UNA) after the last window, a sequence number out of bounds}
};

__device__ __forceinline__ bool lt(uint32_t a, uint32_t b) { return (int32_t)(a - b) < 0; }
__device__ __forceinline__ bool le(uint32_t a, uint32_t b) { return (int32_t)(a - b) <= 0; }
__device__ __forceinline__ bool processed(uint32_t action) { return action - DK_TCP_DELIVERED <= DK_TCP_FIN - DK_TCP_DELIVERED; }

struct Conn {
    uint32_t una, nxt, wnd;
    uint32_t wl1, wl2, wscale, got, qf, qn;
    double srtt, rttvar, rto;
};

// Duration::as_secs_f64 of now - tx (saturating)
__device__ __forceinline__ double rtt_secs(uint64_t now, uint64_t tx) {
    const uint64_t d = now > tx ? now - tx : 0;
    return (double)(d / 1000000000ull) + (double)(d % 1000000000ull) / 1e9;
}

// RtoCalculator::add_sample (rto.rs:40-66) without its last step: rto is a function of (srtt, rttvar) alone, so a call
// that takes several samples computes it once, after the last (update_rto below). eighth = 0.125 * rtt, the one
// product of a sample that does not depend on the state (the wave form computes it for 64 samples at once).
__device__ __forceinline__ void add_sample(Conn& k, double rtt, double eighth) {
    if (!k.got) {
        k.srtt = rtt;
        k.rttvar = rtt / 2.0;
        k.got = 1;
    } else {
        k.rttvar = 0.75 * k.rttvar + 0.25 * fabs(k.srtt - rtt);
        k.srtt = 0.875 * k.srtt + eighth;
    }
}

// The new RTO of add_sample and update_rto (rto.rs:61-79)
__device__ __forceinline__ void update_rto(Conn& k) {
    const double v = k.srtt + fmax(0.001, 4.0 * k.rttvar);
    k.rto = v < 0.1 ? 0.1 : v > 60.0 ? 60.0 : v;
}

// The connection's state and its connection-level checks: DK_TCP_ACK_OK or the failure.
__device__ __forceinline__ uint32_t load_conn(const Params& P, uint32_t c, Conn& k) {
    const dk_tcp_tx_conn& t = P.tx[c];
    const dk_tcp_ack_conn& a = P.ak[c];
    k.una = t.snd_una, k.nxt = t.snd_nxt, k.wnd = t.snd_wnd;
    k.wl1 = a.wl1, k.wl2 = a.wl2, k.wscale = a.snd_wscale, k.got = a.received_sample, k.qf = a.q_first, k.qn = a.q_count;
    k.srtt = a.srtt, k.rttvar = a.rttvar, k.rto = a.rto;
    if (t.state != DK_TCP_ESTABLISHED) return DK_TCP_ACK_E_STATE;
    if (P.rx_conns[c].send_next != k.nxt) return DK_TCP_ACK_E_SND_NXT;
    if (k.nxt - k.una >= 0x80000000u) return DK_TCP_ACK_E_FLIGHT;
    if (k.wscale > 14) return DK_TCP_ACK_E_WSCALE;
    if ((int32_t)(k.wl2 - k.una) > 0) return DK_TCP_ACK_E_WL2;
    if ((uint64_t)k.qf + k.qn > P.nq) return DK_TCP_ACK_E_QUEUE;
    return DK_TCP_ACK_OK;
}

__device__ __forceinline__ void write_failure(const Params& P, uint32_t c, uint32_t status) {
    P.out.status[c] = status;
    P.out.new_acks[c] = P.out.dup_acks[c] = P.out.bytes_acked[c] = P.out.samples[c] = 0;
}

// One thread writes the connection's new state: k against k0 (its state at the call's start). trimmed: the entry at
// the queue's front was cut to (fo, fl) and lost its transmit time.
__device__ __forceinline__ void commit(const Params& P, uint32_t c, const Conn& k0, const Conn& k, uint32_t new_acks,
                                       uint32_t dup_acks, uint32_t samples, bool trimmed, uint32_t fo, uint32_t fl) {
    P.out.status[c] = DK_TCP_ACK_OK;
    P.out.new_acks[c] = new_acks;
    P.out.dup_acks[c] = dup_acks;
    P.out.bytes_acked[c] = k.una - k0.una;
    P.out.samples[c] = samples;
    if (!new_acks) return;  // duplicate and old ACKs change nothing
    P.tx[c].snd_una = k.una;
    P.tx[c].snd_wnd = k.wnd;
    dk_tcp_ack_conn& a = P.ak[c];
    a.wl1 = k.wl1, a.wl2 = k.wl2;
    a.received_sample = k.got;
    a.q_first = k.qf, a.q_count = k.qn;
    a.srtt = k.srtt, a.rttvar = k.rttvar, a.rto = k.rto;
    uint64_t base = 0;  // update_retransmit_deadline (sender.rs:476-488)
    if (k.qn) {
        uint64_t t = kNone;
        if (trimmed) {
            P.q.off[k.qf] = fo;
            P.q.len[k.qf] = fl;
            P.q.tx_time[k.qf] = kNone;
        } else {
            t = P.q.tx_time[k.qf];
        }
        base = t != kNone ? t : P.now;
    }
    a.rtx_armed = k.qn != 0;
    a.rtx_base_ns = base;
}

// The literal loop (sender.rs:406-474) over connection c's walked segments svals[r0 .. r1), by one thread.
__device__ void serial_conn(const Params& P, uint32_t c, const Conn& k0, uint32_t r0, uint32_t r1) {
    Conn k = k0;
    uint32_t new_acks = 0, dup_acks = 0, samples = 0;
    bool have = false, trimmed = false, dry = false;  // the front entry, once read: (fo, fl, ft)
    uint32_t fo = 0, fl = 0;
    uint64_t ft = 0;
    for (uint32_t p = r0; p < r1 && !dry; p++) {
        const uint32_t i = P.svals[p];
        if (!processed(P.action[i])) continue;
        const uint4 g = P.rec[i];
        const uint32_t seq = g.x, ack = g.y, win = P.win[i] & 0xFFFFu;
        P.out.acked[i] = ack - k.una;
        if (ack == k.una) dup_acks++;
        // una <seq ack, as offsets from SND.NXT (a total order; dk_tcp.h's one deviation)
        if ((int32_t)(ack - k.nxt) <= (int32_t)(k.una - k.nxt)) continue;
        new_acks++;
        uint32_t r = ack - k.una;
        while (r != 0) {
            if (k.qn == 0) {
                dry = true;
                break;
            }
            if (!have) {
                fo = P.q.off[k.qf], fl = P.q.len[k.qf], ft = P.q.tx_time[k.qf];
                have = true, trimmed = false;
            }
            if (ft != kNone) {
                const double rtt = rtt_secs(P.now, ft);
                add_sample(k, rtt, 0.125 * rtt);
                samples++;
            }
            if (fl > r) {
                fo += r, fl -= r, ft = kNone;
                trimmed = true;
                break;
            }
            r = fl == 0 ? 0 : r - fl;  // the marker swallows the remainder
            k.qf++, k.qn--;
            have = false, trimmed = false;
        }
        if (dry) break;
        k.una = ack;
        if (lt(k.wl1, seq) || (k.wl1 == seq && le(k.wl2, ack))) {
            k.wnd = win << k.wscale;
            k.wl1 = seq, k.wl2 = ack;
        }
    }
    if (dry) {
        for (uint32_t p = r0; p < r1; p++) {
            const uint32_t i = P.svals[p];
            if (processed(P.action[i])) P.out.acked[i] = 0;
        }
        write_failure(P, c, DK_TCP_ACK_E_DRY);
        return;
    }
    if (samples) update_rto(k);
    commit(P, c, k0, k, new_acks, dup_acks, samples, have && trimmed, fo, fl);
}

constexpr uint32_t kLaneBlock = 64;
__global__ __launch_bounds__(kLaneBlock) void dk_tcp_ack_lane_kernel(Params P) {
    const uint32_t c = blockIdx.x * kLaneBlock + threadIdx.x;
    if (c >= P.nconns) return;
    Conn k0;
    const uint32_t st = load_conn(P, c, k0);
    if (st != DK_TCP_ACK_OK) {
        write_failure(P, c, st);
        return;
    }
    serial_conn(P, c, k0, P.range[2 * c], P.range[2 * c + 1]);
}

using ScanI = rocprim::warp_scan<int, kWave>;
using ScanL = rocprim::warp_scan<unsigned long long, kWave>;

// lane l's value, l wave-uniform
__device__ __forceinline__ double readlane_f64(double v, uint32_t l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)l);
    return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}

// One window's segments as the lanes hold them: frame index (kNoFrame past the range's end) and what the ACK pass
// reads of the frame.
constexpr uint32_t kNoFrame = 0xFFFFFFFFu;
struct Seg {
    uint4 g;
    uint32_t win, act;
};
__device__ __forceinline__ uint32_t load_index(const Params& P, uint32_t p, uint32_t r1) {
    return p < r1 ? P.svals[p] : kNoFrame;
}
__device__ __forceinline__ Seg load_seg(const Params& P, uint32_t i) {
    Seg s{make_uint4(0, 0, 0, 0), 0u, DK_TCP_SKIP};
    if (i != kNoFrame) s.g = P.rec[i], s.win = P.win[i] & 0xFFFFu, s.act = P.action[i];
    return s;
}

// The second half of a connection's pass, by its wave: the queue popped once by the total advance SND.UNA made over the
// segments (run = o(SND.UNA) after them), then the commit — or, where an assumption failed, the serial redo by lane 0.
__device__ void finish_wave(const Params& P, uint32_t c, const Conn& k0, uint32_t r0, uint32_t r1, bool serial, int run,
                            bool upd, uint32_t useq, uint32_t uack, uint32_t uwin, uint32_t new_acks, uint32_t dup_acks,
                            ScanL::storage_type& scan_l) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    // ---- the queue: one pop of the total advance ----
    Conn k = k0;
    k.una = k0.nxt + (uint32_t)run;
    const uint32_t A = k.una - k0.una;
    uint32_t samples = 0, fo = 0, fl = 0;
    bool trimmed = false;
    unsigned long long carry = 0;  // sequence space of the entries before this step
    bool done = A == 0;
    const auto entry = [&](uint32_t e, uint32_t& len, uint64_t& tx) {
        len = 0u, tx = kNone;
        if (!done && e < k0.qn) len = P.q.len[k0.qf + e], tx = P.q.tx_time[k0.qf + e];
    };
    uint32_t len_next;
    uint64_t tx_next;
    entry(lane, len_next, tx_next);
    for (uint32_t e0 = 0; !done && !serial; e0 += kWave) {
        if (e0 >= k0.qn) {  // dry: serial_conn reports it
            serial = true;
            break;
        }
        const bool valid = e0 + lane < k0.qn;
        const uint32_t len = len_next;
        const uint64_t tx = tx_next;
        entry(e0 + kWave + lane, len_next, tx_next);  // the next step's entries load under this step's fold
        unsigned long long incl;
        ScanL().inclusive_scan((unsigned long long)len, incl, scan_l);
        const unsigned long long excl = incl - len;
        const bool reach = valid && carry + excl < A;  // the pop gets to this entry with bytes left
        uint64_t touched = __ballot(reach);
        const uint64_t marks = __ballot(valid && len == 0) & touched;
        if (marks) {
            // a touched marker: every entry before it is consumed whole. It must be the pop's last byte and the
            // queue's last entry, else which ACK swallowed what depends on the ACKs' boundaries.
            const uint32_t m = (uint32_t)__builtin_ctzll(marks);
            const unsigned long long em = carry + (unsigned long long)__shfl((long long)excl, (int)m);
            if (A - em != 1 || e0 + m != k0.qn - 1) {
                serial = true;
                break;
            }
            touched &= (2ull << m) - 1;
            k.qf = k0.qf + e0 + m + 1, k.qn = 0;
            done = true;
        } else {
            const uint32_t whole = (uint32_t)__popcll(__ballot(reach && carry + incl <= A));  // a prefix of the lanes
            k.qf = k0.qf + e0 + whole, k.qn = k0.qn - e0 - whole;
            if (whole < kWave && ((touched >> whole) & 1)) {  // the entry the advance ends inside
                const uint32_t by = A - (uint32_t)(carry + (unsigned long long)__shfl((long long)excl, (int)whole));
                trimmed = true;
                fo = P.q.off[k.qf] + by;
                fl = (uint32_t)__shfl((int)len, (int)whole) - by;
                done = true;
            } else if (__ballot(valid && carry + incl == A) != 0) {
                done = true;
            }
            carry += (unsigned long long)__shfl((long long)incl, (int)kWave - 1);
        }
        // RTT samples of the touched entries: converted in parallel (the division, the state-free product), folded in
        // queue order with wave-uniform values
        const double rtt = rtt_secs(P.now, tx), eighth = 0.125 * rtt;
        const uint64_t sb = touched & __ballot(tx != kNone);
        samples += (uint32_t)__popcll(sb);
#pragma unroll
        for (uint32_t l = 0; l < kWave; l++)
            if ((sb >> l) & 1) add_sample(k, readlane_f64(rtt, l), readlane_f64(eighth, l));
    }
    if (samples) update_rto(k);
    if (serial) {
        __syncthreads();  // this wave's acked[] stores land before lane 0 rewrites them
        if (lane == 0) serial_conn(P, c, k0, r0, r1);
        return;
    }
    if (upd) {
        k.wnd = uwin << k0.wscale;
        k.wl1 = useq, k.wl2 = uack;
    }
    if (lane == 0) commit(P, c, k0, k, new_acks, dup_acks, samples, trimmed, fo, fl);
}

__global__ __launch_bounds__(kWave) void dk_tcp_ack_wave_kernel(Params P) {
    __shared__ ScanI::storage_type scan_i;
    __shared__ ScanL::storage_type scan_l;
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    Conn k0;
    const uint32_t st = load_conn(P, c, k0);  // wave-uniform
    if (st != DK_TCP_ACK_OK) {
        if (lane == 0) write_failure(P, c, st);
        return;
    }
    const uint32_t r0 = P.range[2 * c], r1 = P.range[2 * c + 1];
    // wl2 in (SND.NXT - 2^31, SND.NXT]: with wl2 <= SND.UNA (load_conn), wl2 <=seq ack for every new ACK
    bool serial = k0.nxt - k0.wl2 >= 0x80000000u;

    // ---- the segments: SND.UNA's running maximum, acked[], the window update ----
    int run = (int)(k0.una - k0.nxt);  // o(SND.UNA)
    int smax = 0;                      // the running maximum of seq - wl1 over the new ACKs, from wl1 itself
    bool upd = false;
    uint32_t useq = 0, uack = 0, uwin = 0, new_acks = 0, dup_acks = 0;
    // loads run ahead of their use: a window's frame indices two windows ahead, its records one window ahead
    uint32_t i_next = load_index(P, r0 + lane, r1);
    Seg s_next = load_seg(P, i_next);
    uint32_t i_after = load_index(P, r0 + kWave + lane, r1);
    for (uint32_t base = r0; base < r1 && !serial; base += kWave) {
        const uint32_t i = i_next;
        const Seg cur = s_next;
        i_next = i_after;
        s_next = load_seg(P, i_next);
        i_after = load_index(P, base + 2 * kWave + lane, r1);
        const bool proc = processed(cur.act);
        const uint4 g = cur.g;
        const uint32_t win = cur.win;
        const int o = proc ? (int)(g.y - k0.nxt) : INT_MIN;
        const int s = (int)(g.x - k0.wl1);
        // every seq in (wl1 - 2^29, wl1 + 3 * 2^29): they and wl1 span less than 2^31, so the wrapping comparisons
        // among them are a total order (forward is where sequence numbers go; behind wl1 is reordering only)
        if (__ballot(proc && (s >= (3 << 29) || s <= -(1 << 29))) != 0) {
            serial = true;
            break;
        }
        int inc;
        ScanI().inclusive_scan(o, inc, scan_i, rocprim::maximum<int>());
        const int up = __shfl_up(inc, 1);
        const int before = max(run, lane ? up : INT_MIN);  // o(SND.UNA) as this segment finds it
        const bool isnew = proc && o > before;
        if (proc) P.out.acked[i] = g.y - (k0.nxt + (uint32_t)before);
        new_acks += (uint32_t)__popcll(__ballot(isnew));
        dup_acks += (uint32_t)__popcll(__ballot(proc && o == before));
        run = max(run, __shfl(inc, (int)kWave - 1));
        int sm;
        ScanI().inclusive_scan(isnew ? s : INT_MIN, sm, scan_i, rocprim::maximum<int>());
        const int wm = __shfl(sm, (int)kWave - 1);
        if (wm >= smax) {  // wave-uniform: the last new ACK that attains the maximum passes, none after it does
            const uint32_t l = 63u - (uint32_t)__builtin_clzll(__ballot(isnew && s == wm));
            smax = wm;
            upd = true;
            useq = (uint32_t)__shfl((int)g.x, (int)l), uack = (uint32_t)__shfl((int)g.y, (int)l);
            uwin = (uint32_t)__shfl((int)win, (int)l);
        }
    }

    finish_wave(P, c, k0, r0, r1, serial, run, upd, useq, uack, uwin, new_acks, dup_acks, scan_l);
}

// ---- The chip form: few connections with many segments each (the scan walk's shape) ----
// Everything the segment half computes is associative: (1) dk_tcp_ack_pre_kernel, across the chip: each window's maximum
// of o(ack); (2) dk_tcp_ack_scan_kernel, one wave per connection: the running maximum over the windows, 64 windows a
// step, gives every window the SND.UNA it starts from; (3) dk_tcp_ack_post_kernel, across the chip: acked[], the new and
// duplicate counts and the window-update candidate of every window; (4) dk_tcp_ack_finish_kernel, one wave per
// connection: the windows' counts summed and the last candidate that attains the maximum taken, 64 windows a step, then
// the queue and the commit as in the wave form.
constexpr uint32_t kChipBlock = 256, kChipWaves = kChipBlock / kWave;
__device__ __forceinline__ uint32_t slot0(uint32_t r0, uint32_t c) { return r0 / kWave + c; }
__device__ __forceinline__ bool seq_out_of_bounds(int s) { return s >= (3 << 29) || s <= -(1 << 29); }

template <bool kPost>
__global__ __launch_bounds__(kChipBlock) void dk_tcp_ack_window_kernel(Params P) {
    __shared__ ScanI::storage_type scan_i[kChipWaves];
    const uint32_t c = blockIdx.y, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    Conn k0;
    if (load_conn(P, c, k0) != DK_TCP_ACK_OK) return;
    const uint32_t r0 = P.range[2 * c], r1 = P.range[2 * c + 1], nwin = (r1 - r0 + kWave - 1) / kWave;
    for (uint32_t v = blockIdx.x * kChipWaves + wave; v < nwin; v += gridDim.x * kChipWaves) {
        const uint32_t ws = slot0(r0, c) + v;
        const uint32_t i = load_index(P, r0 + v * kWave + lane, r1);
        const Seg cur = load_seg(P, i);
        const bool proc = processed(cur.act);
        const int o = proc ? (int)(cur.g.y - k0.nxt) : INT_MIN;
        const int s = (int)(cur.g.x - k0.wl1);
        int inc;
        ScanI().inclusive_scan(o, inc, scan_i[wave], rocprim::maximum<int>());
        if (!kPost) {
            const bool far = __ballot(proc && seq_out_of_bounds(s)) != 0;
            if (lane == kWave - 1) P.wmax[ws] = inc, P.wcnt[ws] = make_uint2(far, 0u);
            continue;
        }
        const int up = __shfl_up(inc, 1);
        const int before = max(P.wcarry[ws], lane ? up : INT_MIN);
        const bool isnew = proc && o > before;
        if (proc) P.out.acked[i] = cur.g.y - (k0.nxt + (uint32_t)before);
        const uint32_t nnew = (uint32_t)__popcll(__ballot(isnew)), ndup = (uint32_t)__popcll(__ballot(proc && o == before));
        int sm;
        ScanI().inclusive_scan(isnew ? s : INT_MIN, sm, scan_i[wave], rocprim::maximum<int>());
        const int wm = __shfl(sm, (int)kWave - 1);
        const uint64_t at = __ballot(isnew && s == wm);
        const uint32_t l = at ? 63u - (uint32_t)__builtin_clzll(at) : 0u;
        if (lane == l) P.wpart[ws] = make_uint4((uint32_t)(nnew ? wm : INT_MIN), cur.g.x, cur.g.y, cur.win);
        if (lane == 0) P.wcnt[ws] = make_uint2(nnew, ndup);
    }
}

__global__ __launch_bounds__(kWave) void dk_tcp_ack_scan_kernel(Params P) {
    __shared__ ScanI::storage_type scan_i;
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    Conn k0;
    if (load_conn(P, c, k0) != DK_TCP_ACK_OK) return;
    const uint32_t r0 = P.range[2 * c], r1 = P.range[2 * c + 1], nwin = (r1 - r0 + kWave - 1) / kWave;
    int run = (int)(k0.una - k0.nxt);
    bool far = false;
    for (uint32_t v0 = 0; v0 < nwin; v0 += kWave) {
        const uint32_t v = v0 + lane, ws = slot0(r0, c) + v;
        const int m = v < nwin ? P.wmax[ws] : INT_MIN;
        far |= __ballot(v < nwin && P.wcnt[ws].x != 0) != 0;
        int inc;
        ScanI().inclusive_scan(m, inc, scan_i, rocprim::maximum<int>());
        const int up = __shfl_up(inc, 1);
        if (v < nwin) P.wcarry[ws] = max(run, lane ? up : INT_MIN);
        run = max(run, __shfl(inc, (int)kWave - 1));
    }
    if (lane == 0) P.cstate[c] = make_int2(run, far);
}

__global__ __launch_bounds__(kWave) void dk_tcp_ack_finish_kernel(Params P) {
    __shared__ ScanI::storage_type scan_i;
    __shared__ ScanL::storage_type scan_l;
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    Conn k0;
    const uint32_t st = load_conn(P, c, k0);
    if (st != DK_TCP_ACK_OK) {
        if (lane == 0) write_failure(P, c, st);
        return;
    }
    const uint32_t r0 = P.range[2 * c], r1 = P.range[2 * c + 1], nwin = (r1 - r0 + kWave - 1) / kWave;
    const int2 cs = P.cstate[c];
    const bool serial = k0.nxt - k0.wl2 >= 0x80000000u || cs.y != 0;
    int smax = 0;
    bool upd = false;
    uint32_t useq = 0, uack = 0, uwin = 0, new_acks = 0, dup_acks = 0;
    for (uint32_t v0 = 0; v0 < nwin && !serial; v0 += kWave) {
        const uint32_t v = v0 + lane, ws = slot0(r0, c) + v;
        const uint4 part = v < nwin ? P.wpart[ws] : make_uint4((uint32_t)INT_MIN, 0, 0, 0);
        const uint2 cnt = v < nwin ? P.wcnt[ws] : make_uint2(0, 0);
        int sums;
        ScanI().inclusive_scan((int)cnt.x, sums, scan_i);
        new_acks += (uint32_t)__shfl(sums, (int)kWave - 1);
        ScanI().inclusive_scan((int)cnt.y, sums, scan_i);
        dup_acks += (uint32_t)__shfl(sums, (int)kWave - 1);
        int sm;
        ScanI().inclusive_scan((int)part.x, sm, scan_i, rocprim::maximum<int>());
        const int wm = __shfl(sm, (int)kWave - 1);
        if (wm >= smax) {  // as in the wave form, a window at a time: its last new ACK that attains the maximum
            const uint32_t l = 63u - (uint32_t)__builtin_clzll(__ballot((int)part.x == wm));
            smax = wm;
            upd = true;
            useq = (uint32_t)__shfl((int)part.y, (int)l), uack = (uint32_t)__shfl((int)part.z, (int)l);
            uwin = (uint32_t)__shfl((int)part.w, (int)l);
        }
    }
    finish_wave(P, c, k0, r0, r1, serial, cs.x, upd, useq, uack, uwin, new_acks, dup_acks, scan_l);
}

using dk::ctl::DeviceGuard;

}  // namespace
}  // namespace dk_tcp_ack

extern "C" {

int dk_diag_tcp_ack_set_form(dk_tcp_ctx* t, int32_t form) {
    dk_tcp_order o;
    if (dk_tcp_ctx_order(t, &o) || form < -1 || form > 2) return EINVAL;
    o.ack->form = form;
    return 0;
}

int dk_diag_tcp_ack_last_form(const dk_tcp_ctx* t) {
    dk_tcp_order o;
    return dk_tcp_ctx_order(const_cast<dk_tcp_ctx*>(t), &o) ? -1 : o.ack->last_form;
}

int dk_tcp_ack_process(dk_tcp_ctx* t, const dk_rx_results* rx, uint32_t n, const uint8_t* action,
                       const dk_tcp_conn* rx_conns, dk_tcp_tx_conn* tx_conns, dk_tcp_ack_conn* ack_conns,
                       uint32_t nconns, const dk_tcp_unacked* q, uint32_t nq, uint64_t now_ns,
                       const dk_tcp_ack_out* out, void* stream) {
    using namespace dk_tcp_ack;
    dk_tcp_order o;
    if (dk_tcp_ctx_order(t, &o) || !rx || !q || !out) return EINVAL;
    if (n && (!rx->tcp_win || !action || !out->acked)) return EINVAL;
    if (nconns && (!rx_conns || !tx_conns || !ack_conns || !out->status || !out->new_acks || !out->dup_acks ||
                   !out->bytes_acked || !out->samples))
        return EINVAL;
    if (nq && (!q->off || !q->len || !q->tx_time)) return EINVAL;
    if ((reinterpret_cast<uintptr_t>(tx_conns) | reinterpret_cast<uintptr_t>(ack_conns)) & 15) return EINVAL;
    // in turn: right after the dk_tcp_rx_process call of this context whose order it reuses, once
    if (!o.live || o.call == 0 || o.ack->done == o.call || n != o.n || nconns != o.nconns) return EINVAL;
    o.ack->done = o.call;
    o.ack->last_form = -1;
    if (n == 0 && nconns == 0) return 0;
    DeviceGuard g(o.device);
    const hipStream_t s = (hipStream_t)stream;
    if (o.serial->order(s)) return EINVAL;
    if (n && hipMemsetAsync(out->acked, 0, (size_t)n * sizeof(uint32_t), s) != hipSuccess) return EINVAL;
    if (nconns) {
        Params P{};
        P.svals = o.svals;
        P.range = o.range;
        P.rec = o.rec;
        P.win = rx->tcp_win;
        P.action = action;
        P.rx_conns = rx_conns;
        P.tx = tx_conns;
        P.ak = ack_conns;
        P.nconns = nconns;
        P.q = *q;
        P.nq = nq;
        P.now = now_ns;
        P.out = *out;
        int form = o.ack->form >= 0 ? o.ack->form
                   : (uint64_t)n >= (uint64_t)kChipMinSegs * nconns && nconns <= kChipMaxConns ? 2
                   : (uint64_t)n >= (uint64_t)kWaveMinSegs * nconns                            ? 1
                                                                                               : 0;
        if (form == 2 && nconns > 65535) form = 1;  // the window kernels' grids have one row per connection
        if (form == 2) {
            const size_t slots = (size_t)n / kWave + nconns + 1;
            const size_t need = slots * (sizeof(uint4) + sizeof(uint2) + 2 * sizeof(int)) + (size_t)nconns * sizeof(int2);
            if (int rc = o.ack->scratch.grow(*o.serial, need)) return rc == EIO ? EINVAL : rc;
            uint8_t* b = o.ack->scratch.p;
            P.wpart = reinterpret_cast<uint4*>(b), b += slots * sizeof(uint4);
            P.wcnt = reinterpret_cast<uint2*>(b), b += slots * sizeof(uint2);
            P.cstate = reinterpret_cast<int2*>(b), b += (size_t)nconns * sizeof(int2);
            P.wmax = reinterpret_cast<int*>(b), b += slots * sizeof(int);
            P.wcarry = reinterpret_cast<int*>(b);
        }
        o.ack->last_form = form;
        if (form == 2) {
            const uint32_t per = (uint32_t)(((uint64_t)n / kWave / nconns + kChipWaves) / kChipWaves);
            const dim3 gw(std::min<uint32_t>(std::max<uint32_t>(per, 1u), 65535u), nconns);
            hipLaunchKernelGGL(dk_tcp_ack_window_kernel<false>, gw, dim3(kChipBlock), 0, s, P);
            hipLaunchKernelGGL(dk_tcp_ack_scan_kernel, dim3(nconns), dim3(kWave), 0, s, P);
            hipLaunchKernelGGL(dk_tcp_ack_window_kernel<true>, gw, dim3(kChipBlock), 0, s, P);
            hipLaunchKernelGGL(dk_tcp_ack_finish_kernel, dim3(nconns), dim3(kWave), 0, s, P);
        } else if (form == 1)
            hipLaunchKernelGGL(dk_tcp_ack_wave_kernel, dim3(nconns), dim3(kWave), 0, s, P);
        else
            hipLaunchKernelGGL(dk_tcp_ack_lane_kernel, dim3((nconns + kLaneBlock - 1) / kLaneBlock), dim3(kLaneBlock), 0,
                               s, P);
    }
    return o.serial->record(s) ? EINVAL : 0;
}

}  // extern "C"
