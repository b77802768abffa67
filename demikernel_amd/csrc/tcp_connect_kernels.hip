// tcp_connect_kernels.hip — the active open on the GPU (include/dk_tcp.h, the dk_tcp_connect_* section): the ISN and
// the first SYN of a batch of connect() calls, SharedActiveOpenSocket's process_ack and retry loop over a whole
// receive batch, and the handshake timeout.
//
// A row's outcome in dk_tcp_connect_process depends on three things: the index T of its first refused / accepted frame,
// the arrival rank e of its EAGAIN frames before T, and syns_left = S. An EAGAIN of rank e < S resends the SYN, the one
// of rank S exhausts the row; T takes effect iff its own rank is <= S; everything behind the deciding frame is FORWARD
// or ORPHANED. So:
//   1. con_check_kernel      per row: status.
//   2. con_classify_kernel   per frame: its row and process_ack's verdict; one add per CONNECTING frame counts the row's
//                            frames, a 32-bit atomicMin finds T.
//   3. con_multi_kernel      the frames that need a rank are those of rows with two or more frames, up to T. Nearly
//                            every row has one frame a batch, whose rank is 0. A second count and a second atomicMin
//                            over those frames settle the rows that have two of them: the first has rank 0, the other
//                            rank 1. con_flag_kernel flags the frames of the rows that have three or more;
//                            dk_tcp_tx_scan compacts them in frame order (con_gather_kernel).
//   4. con_rank_kernel       one wave per 64 frames of the compacted list: the lanes group themselves by row in
//                            registers; a frame's rank within its group is a popcount, and the first lane of each
//                            group pushes the group (its place in the list, its count) onto the row's chain with one
//                            atomic exchange. con_base_kernel: each group's first lane walks its row's chain and adds
//                            up the counts of the groups that lie before its own in the list. A frame's rank, base +
//                            popcount, is exact for any number of frames per row; the memory is a word per row and
//                            four per frame, not tiles x rows; a walk is as long as the row has groups.
//   5. con_decide_kernel     every frame's action, and which frame of a row writes the row; two scans number the
//                            replies and the ready records.
//   6. con_build_kernel      the frames, the records, the per-frame results and the rows, behind the call's one capacity
//                            test, made on the device; con_finish_kernel the two words and NO_ROOM.
// dk_tcp_connect_start and dk_tcp_connect_timers are the same three stages (flag, scan, build) over start[] entries and
// rows. No loop depends on another workgroup's progress. Atomics are agent-scope integer __hip_atomic_* on global
// memory; everything else is plain vector stores. The ISN's CRC and the frame builder are ctl_common.h's.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <mutex>

#include "../../include/dk_tcp.h"
#include "ctl_common.h"

namespace dk_tcp_connect {
namespace {
using namespace dk::ctl;

constexpr uint32_t kNone = DK_TCP_CON_NONE;

// What the classify pass leaves per frame: kind | process_ack's verdict << 4.
enum Kind : uint32_t { kSkip = 0, kForward = 1, kOrphaned = 2, kConn = 3 };
enum Verdict : uint32_t { kEagain = 0, kRefused = 1, kAccepted = 2 };
constexpr uint32_t kDecides = 0x80u;  // act[]: this frame writes its row

struct Params {
    dk_rx_results rx;
    uint32_t n;
    dk_tcp_connector* rows;
    uint32_t nrows;
    const uint32_t* conn_of_flow;
    uint32_t nflows;
    const uint32_t* link;
    const dk_tx_link* links;
    uint32_t nlinks;
    const uint32_t* start;
    uint32_t nstart;
    dk_tcp_isn_gen* gen;
    uint64_t now;
    uint8_t* out;
    uint64_t out_bytes;
    uint32_t stride, lead, max_frames, max_ready, flags;
    dk_tcp_con_results res;
    // scratch
    uint32_t *cnt, *term, *head, *work;  // [nrows]: frames, T, the row's chain of groups, the row had work
    uint32_t *cnt2, *first;              // [nrows]: of the frames up to T in rows of two or more, the count and the first
    uint32_t *frow, *rank, *mlist;       // [n]: a frame's row and rank within its group; the compacted list
    uint32_t *gid, *gnext, *gcnt, *gsum;  // [n]: a frame's group; per group (by its place in the list) the chain link,
                                          // the count, the frames of the row in the groups before it
    uint8_t *kind, *act;                 // [n]
    uint64_t *flag_r, *flag_y, *flag_m, *tot;  // [items] x 3, [3]: frames, records, ranked frames
};

__device__ __forceinline__ bool fits(const Params& P) {
    return dk::tcp_tx_fits(P.tot[0], P.max_frames, P.stride, P.out_bytes) && P.tot[1] <= P.max_ready;
}

// The row checks that every call makes, in dk_tcp.h's order.
__device__ __forceinline__ uint32_t row_check(const Params& P, const dk_tcp_connector& R) {
    if (R.window_scale > 14) return DK_TCP_CON_E_WSCALE;
    if (R.link >= P.nlinks) return DK_TCP_CON_E_LINK;
    if ((uint64_t)P.lead + DK_TCP_CON_SYN_BYTES > P.stride) return DK_TCP_CON_E_SLOT;
    return DK_TCP_CON_OK;
}

// Frame f of the call: its place in out, and the SYN (syn) or the handshake ACK of row R.
__device__ void emit_frame(const Params& P, uint64_t f, uint32_t seg, const dk_tcp_connector& R, uint32_t lk, bool syn,
                           uint32_t ack) {
    const uint32_t foff = (uint32_t)(f * P.stride + P.lead);
    P.res.off_out[f] = foff;
    P.res.len_out[f] = (uint16_t)(syn ? DK_TCP_CON_SYN_BYTES : DK_TCP_CON_ACK_BYTES);
    if (P.res.frame_seg) P.res.frame_seg[f] = seg;
    tcp_frame(P.out + foff, P.links + lk, R.ip_word, R.local_ip, R.remote_ip, R.local_port, R.remote_port,
              syn ? R.local_isn : R.local_isn + 1u, ack, syn ? 0x02u : 0x10u, R.receive_window_size, syn, R.advertised_mss,
              R.window_scale, (P.flags & DK_TX_OFFLOAD_TCP) != 0);
}

__device__ void error_record(dk_tcp_con_ready* Y, uint32_t r, uint32_t cause, uint32_t frame, uint32_t local_isn) {
    Y->row = r;
    Y->err = ECONNREFUSED;
    Y->cause = (uint16_t)cause;
    Y->frame = frame;
    Y->rcv_nxt = 0;
    Y->snd_nxt = local_isn + 1u;
    Y->local_window = 0, Y->remote_window = 0, Y->mss = 0;
    Y->local_wscale = 0, Y->remote_wscale = 0, Y->reserved0 = 0, Y->reserved1 = 0, Y->reserved2 = 0;
}

// ---- dk_tcp_connect_process ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void con_check_kernel(Params P) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= P.nrows) return;
    const dk_tcp_connector& R = P.rows[r];
    P.res.status[r] = R.state == DK_TCP_CON_CONNECTING ? row_check(P, R) : (uint32_t)DK_TCP_CON_OK;
}

__global__ __launch_bounds__(kBlock) void con_classify_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    uint32_t kind = kSkip, r = kNone;
    const uint32_t meta = P.rx.meta[i], f = P.rx.flow_id[i];
    if ((meta & 0xFFu) == DK_V_OK_TCP && f < P.nflows) {
        r = P.conn_of_flow[f];
        if (r < P.nrows) {
            const dk_tcp_connector& R = P.rows[r];
            const uint32_t st = R.state;
            if (st == DK_TCP_CON_ESTAB) kind = kForward;
            else if (st == DK_TCP_CON_FAILED) kind = kOrphaned;
            else if (st == DK_TCP_CON_CONNECTING && row_check(P, R) == DK_TCP_CON_OK) {
                const uint32_t fl = meta >> 16;  // byte 13: FIN 1, SYN 2, RST 4, ACK 16
                uint32_t v = kEagain;
                if ((fl & 16u) && P.rx.tcp_ack[i] == R.local_isn + 1u) v = (fl & 4u) ? kRefused : (fl & 2u) ? kAccepted : kEagain;
                kind = kConn | v << 4;
                add32(P.cnt + r, 1u);
                if (v != kEagain) min32(P.term + r, i);
            }
            if (kind != kSkip) P.work[r] = 1;
        }
    }
    P.kind[i] = (uint8_t)kind;
    P.frow[i] = r;
}

// Whether frame i of row r needs a rank other than 0.
__device__ __forceinline__ bool needs_rank(const Params& P, uint32_t i, uint32_t r) {
    return P.cnt[r] >= 2 && i <= P.term[r];
}

__global__ __launch_bounds__(kBlock) void con_multi_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n || (P.kind[i] & 0xFu) != kConn) return;
    const uint32_t r = P.frow[i];
    if (!needs_rank(P, i, r)) return;
    add32(P.cnt2 + r, 1u);
    min32(P.first + r, i);
}

__global__ __launch_bounds__(kBlock) void con_flag_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    bool m = false;
    if ((P.kind[i] & 0xFu) == kConn) {
        const uint32_t r = P.frow[i];
        m = needs_rank(P, i, r) && P.cnt2[r] >= 3;
    }
    P.flag_m[i] = m;
}

// The frames of i's row before i (i <= T): 0 for a row's only frame, by the first-frame minimum for a row with two
// ranked frames, else what the walk left.
__device__ __forceinline__ uint32_t rank_of(const Params& P, uint32_t i, uint32_t r) {
    if (P.cnt[r] < 2) return 0u;
    if (P.cnt2[r] <= 2) return i != P.first[r];
    return P.rank[i] + P.gsum[P.gid[i]];
}

__global__ __launch_bounds__(kBlock) void con_gather_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint64_t at = P.flag_m[i];
    if ((i + 1 < P.n ? P.flag_m[i + 1] : P.tot[2]) != at) P.mlist[at] = i;
}

// One wave per 64 frames of the compacted list: rank[i] = the frames of i's row before i within the 64, gid[i] = the
// group's place in the list (its first frame's), where its count and its link in the row's chain are kept.
__global__ __launch_bounds__(kBlock) void con_rank_kernel(Params P) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t m = P.tot[2];
    const uint64_t base = ((uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * kWave;
    if (base >= m) return;  // whole waves leave
    const bool on = base + lane < m;
    const uint32_t i = on ? P.mlist[base + lane] : 0u;
    const uint32_t r = on ? P.frow[i] : 0u;
    uint64_t todo = __ballot(on), mine = 0;
    while (todo) {  // uniform: one round per distinct row among the wave's frames, registers only
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t rr = (uint32_t)__shfl((int)r, leader);
        const uint64_t g = __ballot(on && r == rr);
        if (on && r == rr) mine = g;
        todo &= ~g;
    }
    if (!on) return;
    const uint32_t lead = (uint32_t)(__ffsll((long long)mine) - 1), place = (uint32_t)base + lead;
    P.rank[i] = (uint32_t)__popcll(mine & ((1ull << lane) - 1));
    P.gid[i] = place;
    if (lane == lead) {
        P.gcnt[place] = (uint32_t)__popcll(mine);  // the group's count
        P.gnext[place] = __hip_atomic_exchange(P.head + r, place, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Per group (its first frame's lane): the frames of its row in the groups before it. The chain is in push order, not
// list order, so the whole chain is walked; it ends at kNone.
__global__ __launch_bounds__(kBlock) void con_base_kernel(Params P) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= P.tot[2]) return;
    const uint32_t i = P.mlist[p];
    if (P.gid[i] != (uint32_t)p) return;  // not a group's first frame
    uint32_t before = 0;
    for (uint32_t q = P.head[P.frow[i]]; q != kNone; q = P.gnext[q])
        if (q < (uint32_t)p) before += P.gcnt[q];
    P.gsum[p] = before;
}

__global__ __launch_bounds__(kBlock) void con_decide_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t kd = P.kind[i], k = kd & 0xFu, v = kd >> 4;
    uint32_t act = DK_TCP_CON_SKIP;
    bool reply = false, ready = false, decides = false;
    if (k == kForward) act = DK_TCP_CON_FORWARD;
    else if (k == kOrphaned) act = DK_TCP_CON_ORPHANED;
    else if (k == kConn) {
        const uint32_t r = P.frow[i], S = P.rows[r].syns_left, c = P.cnt[r], T = P.term[r];
        if (i <= T) {
            const uint32_t e = rank_of(P, i, r);
            if (i == T) {
                if (e <= S) {
                    act = v == kAccepted ? DK_TCP_CON_ESTABLISHED : DK_TCP_CON_REFUSED;
                    reply = v == kAccepted, ready = true, decides = true;
                } else {
                    act = DK_TCP_CON_ORPHANED;  // the row ran out of SYNs before it
                }
            } else if (e < S) {
                act = DK_TCP_CON_RETRY_SYN;
                reply = true;
                decides = T == kNone && e == c - 1;  // the row's last frame, and nothing ended the handshake
            } else if (e == S) {
                act = DK_TCP_CON_EXHAUSTED;
                ready = true, decides = true;
            } else {
                act = DK_TCP_CON_ORPHANED;
            }
        } else {  // behind T: two frames at least, so T has a rank
            const bool took = rank_of(P, T, r) <= S;
            act = took && (P.kind[T] >> 4) == kAccepted ? DK_TCP_CON_FORWARD : DK_TCP_CON_ORPHANED;
        }
    }
    P.act[i] = (uint8_t)(act | (decides ? kDecides : 0u));
    P.flag_r[i] = reply;
    P.flag_y[i] = ready;
}

// Behind the capacity test. Of a row's frames only the deciding one reads or writes the fields that move.
__global__ __launch_bounds__(kBlock) void con_build_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n || !fits(P)) return;
    const uint32_t a8 = P.act[i], act = a8 & 0x7Fu, r = P.frow[i];
    uint32_t rf = kNone;
    if (act == DK_TCP_CON_RETRY_SYN || act == DK_TCP_CON_ESTABLISHED) {
        const dk_tcp_connector& R = P.rows[r];
        uint32_t lk = R.link;
        if (P.link && P.link[i] < P.nlinks) lk = P.link[i];
        rf = (uint32_t)P.flag_r[i];
        emit_frame(P, P.flag_r[i], i, R, lk, act == DK_TCP_CON_RETRY_SYN, act == DK_TCP_CON_RETRY_SYN ? 0u : P.rx.tcp_seq[i] + 1u);
    }
    if (act == DK_TCP_CON_ESTABLISHED) {
        const dk_tcp_connector& R = P.rows[r];
        uint32_t mss = DK_TCP_CON_FALLBACK_MSS, rws = 0, lws = 0;
        if ((P.rx.meta[i] >> 28) > 5) {  // the record is written for option-bearing segments only
            const dk_tcp_opts& o = P.rx.tcp_opts[i];
            const uint32_t num = o.num < 5 ? o.num : 5;
            for (uint32_t k = 0; k < num; k++) {
                if (o.opt[k].kind == DK_TCPOPT_MSS) mss = o.opt[k].u16;
                else if (o.opt[k].kind == DK_TCPOPT_WS) rws = o.opt[k].u8 < 14 ? o.opt[k].u8 : 14u, lws = R.window_scale;
            }
        }
        dk_tcp_con_ready* Y = P.res.ready + P.flag_y[i];
        Y->row = r;
        Y->err = 0, Y->cause = DK_TCP_CON_CAUSE_NONE;
        Y->frame = i;
        Y->rcv_nxt = P.rx.tcp_seq[i] + 1u;
        Y->snd_nxt = R.local_isn + 1u;
        Y->local_window = (uint32_t)R.receive_window_size << lws;
        Y->remote_window = (P.rx.tcp_win[i] & 0xFFFFu) << rws;
        Y->mss = mss;
        Y->local_wscale = (uint8_t)lws, Y->remote_wscale = (uint8_t)rws;
        Y->reserved0 = 0, Y->reserved1 = 0, Y->reserved2 = 0;
    } else if (act == DK_TCP_CON_REFUSED || act == DK_TCP_CON_EXHAUSTED) {
        error_record(P.res.ready + P.flag_y[i], r, act == DK_TCP_CON_REFUSED ? DK_TCP_CON_CAUSE_RST : DK_TCP_CON_CAUSE_EXHAUSTED,
                     i, P.rows[r].local_isn);
    }
    if (a8 & kDecides) {
        dk_tcp_connector& R = P.rows[r];
        const uint32_t S = R.syns_left, e = rank_of(P, i, r);
        const uint32_t sent = act == DK_TCP_CON_RETRY_SYN ? e + 1u : act == DK_TCP_CON_EXHAUSTED ? S : e;  // SYNs resent
        R.syns_left = S - sent;
        if (sent) R.deadline_ns = P.now + R.handshake_timeout_ns;
        if (act == DK_TCP_CON_ESTABLISHED) R.state = DK_TCP_CON_ESTAB;
        else if (act != DK_TCP_CON_RETRY_SYN) R.state = DK_TCP_CON_FAILED, R.err = ECONNREFUSED;
    }
    P.res.action[i] = (uint8_t)act;
    P.res.row[i] = act == DK_TCP_CON_SKIP ? kNone : r;
    P.res.reply_frame[i] = rf;
}

// The two words, and NO_ROOM for the items (rows; start[] entries) that had work.
__global__ __launch_bounds__(kBlock) void con_finish_kernel(Params P, uint32_t items) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const bool ok = fits(P);
    if (j == 0) {
        *P.res.n_frames = (uint32_t)P.tot[0];
        *P.res.n_ready = (uint32_t)P.tot[1];
        if (ok && P.gen) P.gen->counter = (uint16_t)(P.gen->counter + P.nstart);
    }
    if (j >= items || ok) return;
    if (P.res.status[j] == DK_TCP_CON_OK && (!P.work || P.work[j])) P.res.status[j] = DK_TCP_CON_NO_ROOM;
}

// ---- dk_tcp_connect_timers ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void con_sweep_kernel(Params P) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= P.nrows) return;
    const dk_tcp_connector& R = P.rows[r];
    uint32_t st = DK_TCP_CON_OK;
    bool due = false;
    if (R.state == DK_TCP_CON_CONNECTING) {
        st = row_check(P, R);
        due = st == DK_TCP_CON_OK && R.deadline_ns <= P.now;
    }
    P.res.status[r] = st;
    P.work[r] = due;
    P.flag_r[r] = due && R.syns_left > 0;
    P.flag_y[r] = due && R.syns_left == 0;
}

__global__ __launch_bounds__(kBlock) void con_expire_kernel(Params P) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= P.nrows || !fits(P) || !P.work[r]) return;
    dk_tcp_connector& R = P.rows[r];
    if (R.syns_left > 0) {
        R.syns_left -= 1;
        R.deadline_ns = P.now + R.handshake_timeout_ns;
        emit_frame(P, P.flag_r[r], r, R, R.link, true, 0u);
    } else {
        R.state = DK_TCP_CON_FAILED, R.err = ECONNREFUSED;
        error_record(P.res.ready + P.flag_y[r], r, DK_TCP_CON_CAUSE_EXHAUSTED, kNone, R.local_isn);
    }
}

// ---- dk_tcp_connect_start -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void con_claim_kernel(Params P) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= P.nstart) return;
    const uint32_t r = P.start[k];
    if (r < P.nrows) min32(P.term + r, k);  // the first entry that names the row
}

__global__ __launch_bounds__(kBlock) void con_admit_kernel(Params P) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= P.nstart) return;
    const uint32_t r = P.start[k];
    uint32_t st = DK_TCP_CON_E_ROW, retries = 0;
    if (r < P.nrows) {
        const dk_tcp_connector& R = P.rows[r];
        st = R.state != DK_TCP_CON_IDLE || P.term[r] != k ? (uint32_t)DK_TCP_CON_E_STATE : row_check(P, R);
        retries = R.handshake_retries;
    }
    P.res.status[k] = st;
    P.flag_r[k] = st == DK_TCP_CON_OK && retries > 0;
    P.flag_y[k] = st == DK_TCP_CON_OK && retries == 0;
}

__global__ __launch_bounds__(kBlock) void con_open_kernel(Params P) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= P.nstart || !fits(P) || P.res.status[k] != DK_TCP_CON_OK) return;
    const uint32_t r = P.start[k];
    dk_tcp_connector& R = P.rows[r];
    R.local_isn = isn_crc(R.remote_ip, R.remote_port, R.local_ip, R.local_port, P.gen->nonce) +
                  (uint32_t)(uint16_t)(P.gen->counter + k);
    if (R.handshake_retries > 0) {
        R.state = DK_TCP_CON_CONNECTING, R.err = 0;
        R.syns_left = R.handshake_retries - 1;
        R.deadline_ns = P.now + R.handshake_timeout_ns;
        emit_frame(P, P.flag_r[k], k, R, R.link, true, 0u);
    } else {
        R.state = DK_TCP_CON_FAILED, R.err = ECONNREFUSED;
        R.syns_left = 0;
        error_record(P.res.ready + P.flag_y[k], r, DK_TCP_CON_CAUSE_EXHAUSTED, k, R.local_isn);
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------
CallScratch g_pool[kMaxDevices];  // one per device: the calls' scratch, and the event that serialises them on it
std::mutex g_mutex;

// What every call checks before any GPU work.
bool bad_common(const void* rows, uint32_t nrows, const dk_tx_link* links, uint32_t nlinks, uint64_t out_bytes,
                const dk_tcp_tx_layout* layout, const dk_tcp_con_results* res) {
    if (!layout || !res || !res->n_frames || !res->n_ready || !links || nlinks == 0) return true;
    if (out_bytes > DK_RX_MAX_BLOB) return true;
    if (nrows && !rows) return true;
    return (reinterpret_cast<uintptr_t>(rows) & 15) != 0;
}
bool bad_outputs(const uint8_t* out, uint32_t max_frames, uint32_t max_ready, const dk_tcp_con_results* res) {
    return !res->status || (max_frames && (!out || !res->off_out || !res->len_out)) || (max_ready && !res->ready);
}

void fill_common(Params& P, dk_tcp_connector* rows, uint32_t nrows, const dk_tx_link* links, uint32_t nlinks,
                 uint64_t now_ns, uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames,
                 uint32_t max_ready, uint32_t flags, const dk_tcp_con_results* res) {
    P.rows = rows, P.nrows = nrows, P.links = links, P.nlinks = nlinks, P.now = now_ns;
    P.out = out, P.out_bytes = out_bytes, P.stride = layout->slot_stride, P.lead = layout->frame_lead;
    P.max_frames = max_frames, P.max_ready = max_ready, P.flags = flags, P.res = *res;
}

}  // namespace
}  // namespace dk_tcp_connect

extern "C" {

int dk_tcp_connect_start(dk_tcp_connector* rows, uint32_t nrows, const uint32_t* start, uint32_t nstart,
                         dk_tcp_isn_gen* isn_gen, const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns, uint8_t* out,
                         uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready,
                         uint32_t flags, const dk_tcp_con_results* res, void* stream) {
    using namespace dk_tcp_connect;
    if (bad_common(rows, nrows, links, nlinks, out_bytes, layout, res)) return EINVAL;
    if (!isn_gen || (reinterpret_cast<uintptr_t>(isn_gen) & 7) || nstart > 0x7FFFFFFFu) return EINVAL;
    if (nstart && (!start || bad_outputs(out, max_frames, max_ready, res))) return EINVAL;
    std::lock_guard<std::mutex> lock(g_mutex);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t sb = dk_tcp_tx_scan_tiles(nstart);
    const size_t ff_bytes = round16((size_t)nrows * 4), zero_bytes = round16(3 * 8);
    const size_t need = ff_bytes + zero_bytes + 2 * round16((size_t)nstart * 8) + round16((size_t)sb * 8) + 16;
    CallScratch* pool = nullptr;
    if (int rc = enter_pool(g_pool, need, s, &pool)) return rc;
    Params P{};
    fill_common(P, rows, nrows, links, nlinks, now_ns, out, out_bytes, layout, max_frames, max_ready, flags, res);
    P.start = start, P.nstart = nstart, P.gen = isn_gen;
    Carver c{pool->scratch.p};
    P.term = c.take<uint32_t>(nrows);
    P.tot = c.take<uint64_t>(3);
    P.flag_r = c.take<uint64_t>(nstart);
    P.flag_y = c.take<uint64_t>(nstart);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if ((ff_bytes && hipMemsetAsync(P.term, 0xFF, ff_bytes, s) != hipSuccess) ||
        hipMemsetAsync(P.tot, 0, zero_bytes, s) != hipSuccess)
        return EIO;
    if (nstart) {
        hipLaunchKernelGGL(con_claim_kernel, grid_for(nstart), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(con_admit_kernel, grid_for(nstart), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, nstart, bsum, P.tot, s) || dk_tcp_tx_scan(P.flag_y, nstart, bsum, P.tot + 1, s))
            return EIO;
        hipLaunchKernelGGL(con_open_kernel, grid_for(nstart), dim3(kBlock), 0, s, P);
    }
    hipLaunchKernelGGL(con_finish_kernel, grid_for(nstart), dim3(kBlock), 0, s, P, nstart);
    return pool->record(s);
}

int dk_tcp_connect_process(const dk_rx_results* rx, uint32_t n, dk_tcp_connector* rows, uint32_t nrows,
                           const uint32_t* conn_of_flow, uint32_t nflows, const uint32_t* link, const dk_tx_link* links,
                           uint32_t nlinks, uint64_t now_ns, uint8_t* out, uint64_t out_bytes,
                           const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready, uint32_t flags,
                           const dk_tcp_con_results* res, void* stream) {
    using namespace dk_tcp_connect;
    if (!rx || bad_common(rows, nrows, links, nlinks, out_bytes, layout, res) || n > 0x7FFFFFFFu) return EINVAL;
    if (nrows && !res->status) return EINVAL;
    if (n && (!rx->meta || !rx->flow_id || !rx->tcp_seq || !rx->tcp_ack || !rx->tcp_win || !rx->tcp_opts || !res->action ||
              !res->row || !res->reply_frame))
        return EINVAL;
    if (n && nrows && ((nflows && !conn_of_flow) || bad_outputs(out, max_frames, max_ready, res))) return EINVAL;
    std::lock_guard<std::mutex> lock(g_mutex);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t sb = dk_tcp_tx_scan_tiles(n);
    const size_t ff_bytes = 3 * round16((size_t)nrows * 4);
    const size_t zero_bytes = 3 * round16((size_t)nrows * 4) + round16(3 * 8);
    const size_t need = ff_bytes + zero_bytes + 7 * round16((size_t)n * 4) + 2 * round16(n) + 3 * round16((size_t)n * 8) +
                        round16((size_t)sb * 8) + 16;
    CallScratch* pool = nullptr;
    if (int rc = enter_pool(g_pool, need, s, &pool)) return rc;
    Params P{};
    fill_common(P, rows, nrows, links, nlinks, now_ns, out, out_bytes, layout, max_frames, max_ready, flags, res);
    P.rx = *rx, P.n = n, P.conn_of_flow = conn_of_flow, P.nflows = nflows, P.link = link;
    Carver c{pool->scratch.p};
    P.term = c.take<uint32_t>(nrows);
    P.first = c.take<uint32_t>(nrows);
    P.head = c.take<uint32_t>(nrows);
    uint8_t* zz = c.b;
    P.cnt = c.take<uint32_t>(nrows);
    P.cnt2 = c.take<uint32_t>(nrows);
    P.work = c.take<uint32_t>(nrows);
    P.tot = c.take<uint64_t>(3);
    P.frow = c.take<uint32_t>(n);
    P.rank = c.take<uint32_t>(n);
    P.mlist = c.take<uint32_t>(n);
    P.gid = c.take<uint32_t>(n);
    P.gnext = c.take<uint32_t>(n);
    P.gcnt = c.take<uint32_t>(n);
    P.gsum = c.take<uint32_t>(n);
    P.kind = c.take<uint8_t>(n);
    P.act = c.take<uint8_t>(n);
    P.flag_r = c.take<uint64_t>(n);
    P.flag_y = c.take<uint64_t>(n);
    P.flag_m = c.take<uint64_t>(n);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if ((ff_bytes && hipMemsetAsync(P.term, 0xFF, ff_bytes, s) != hipSuccess) ||
        hipMemsetAsync(zz, 0, zero_bytes, s) != hipSuccess)
        return EIO;
    if (nrows) hipLaunchKernelGGL(con_check_kernel, grid_for(nrows), dim3(kBlock), 0, s, P);
    if (n && nrows) {
        hipLaunchKernelGGL(con_classify_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(con_multi_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(con_flag_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_m, n, bsum, P.tot + 2, s)) return EIO;
        hipLaunchKernelGGL(con_gather_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(con_rank_kernel, grid_for(n), dim3(kBlock), 0, s, P);  // a wave per 64 of the list: at most n
        hipLaunchKernelGGL(con_base_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(con_decide_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, n, bsum, P.tot, s) || dk_tcp_tx_scan(P.flag_y, n, bsum, P.tot + 1, s)) return EIO;
        hipLaunchKernelGGL(con_build_kernel, grid_for(n), dim3(kBlock), 0, s, P);
    } else if (n) {  // no row: every frame is SKIP
        if (hipMemsetAsync(res->action, 0, n, s) != hipSuccess ||
            hipMemsetAsync(res->row, 0xFF, (size_t)n * 4, s) != hipSuccess ||
            hipMemsetAsync(res->reply_frame, 0xFF, (size_t)n * 4, s) != hipSuccess)
            return EIO;
    }
    hipLaunchKernelGGL(con_finish_kernel, grid_for(nrows), dim3(kBlock), 0, s, P, nrows);
    return pool->record(s);
}

int dk_tcp_connect_timers(dk_tcp_connector* rows, uint32_t nrows, const dk_tx_link* links, uint32_t nlinks,
                          uint64_t now_ns, uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout,
                          uint32_t max_frames, uint32_t max_ready, uint32_t flags, const dk_tcp_con_results* res,
                          void* stream) {
    using namespace dk_tcp_connect;
    if (bad_common(rows, nrows, links, nlinks, out_bytes, layout, res)) return EINVAL;
    if (nrows && bad_outputs(out, max_frames, max_ready, res)) return EINVAL;
    std::lock_guard<std::mutex> lock(g_mutex);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t sb = dk_tcp_tx_scan_tiles(nrows);
    const size_t zero_bytes = round16(3 * 8);
    const size_t need = zero_bytes + round16((size_t)nrows * 4) + 2 * round16((size_t)nrows * 8) + round16((size_t)sb * 8) + 16;
    CallScratch* pool = nullptr;
    if (int rc = enter_pool(g_pool, need, s, &pool)) return rc;
    Params P{};
    fill_common(P, rows, nrows, links, nlinks, now_ns, out, out_bytes, layout, max_frames, max_ready, flags, res);
    Carver c{pool->scratch.p};
    P.tot = c.take<uint64_t>(3);
    P.work = c.take<uint32_t>(nrows);
    P.flag_r = c.take<uint64_t>(nrows);
    P.flag_y = c.take<uint64_t>(nrows);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if (hipMemsetAsync(P.tot, 0, zero_bytes, s) != hipSuccess) return EIO;
    if (nrows) {
        hipLaunchKernelGGL(con_sweep_kernel, grid_for(nrows), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, nrows, bsum, P.tot, s) || dk_tcp_tx_scan(P.flag_y, nrows, bsum, P.tot + 1, s)) return EIO;
        hipLaunchKernelGGL(con_expire_kernel, grid_for(nrows), dim3(kBlock), 0, s, P);
    }
    hipLaunchKernelGGL(con_finish_kernel, grid_for(nrows), dim3(kBlock), 0, s, P, nrows);
    return pool->record(s);
}

}  // extern "C"
