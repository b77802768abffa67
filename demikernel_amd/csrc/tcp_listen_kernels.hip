// tcp_listen_kernels.hip — the passive open on the GPU (include/dk_tcp.h, the dk_tcp_listen_* section): the
// connection table the device itself inserts into, and SharedPassiveSocket's state machine over a whole batch.
//
// The state machine is two deep per key, so a batch needs neither a sort nor a serial walk:
//   1. lsn_check_kernel      per listener: the listener checks (status), the device's own sum of max_backlog.
//   2. lsn_lookup_kernel     per frame: the read-only lookup of the persistent table; ESTABLISHED / FAILED hits are
//                            classified at once, the others join their key's group in a per-call scratch hash and a
//                            32-bit atomicMin finds the group's first valid SYN (no entry) or first frame (SYN_RCVD).
//   3. lsn_rank_kernel       those first SYNs are the only backlog and ISN candidates. The backlog only fills within
//                            a call, so a candidate is accepted iff its rank among its listener's candidates, in
//                            frame order, is below max_backlog - inflight, and its counter is isn_counter + rank.
//                            One wave per tile of frames walks it 64 frames at a time: the lanes group themselves
//                            by listener in registers, the first lane of each group adds the group's count to the
//                            tile's row of a tiles x listeners matrix (one round trip a step; a row's atomics come
//                            from one wave, in order); lsn_colscan_kernel turns each listener's column into the
//                            tiles' bases.
//   4. lsn_second_kernel     the accepted candidates' ISNs, and a second atomicMin over the frames behind an accepted
//                            SYN: the one wait_for_ack pops.
//   5. lsn_classify_kernel   every frame classifies itself; two scans (dk_tcp_tx_scan) number the replies and the
//                            ready records.
//   6. lsn_commit_kernel     inserts the accepted keys (a 64-bit compare-and-swap claims a FREE or TOMBSTONE key
//                            word) and writes the one row per slot that changed; lsn_build_kernel writes the frames,
//                            the ready records and the per-frame results; lsn_finish_kernel the listeners' two
//                            fields, the statuses and the two words. All three sit behind the call's one capacity
//                            test, made on the device. They run after the last lookup: the kernel boundary is the
//                            only ordering needed.
// No loop depends on another workgroup's progress: every probe loop is bounded by the table's size and a failed
// compare-and-swap moves on. Atomics are agent-scope integer __hip_atomic_* on global memory; everything else is
// plain vector stores. The replies (62 and 54 bytes, no payload to sum) are ctl_common.h's tcp_frame.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dk_tcp.h"
#include "ctl_common.h"

struct dk_tcp_listen_table {
    int device = 0;
    uint32_t cap = 0;
    dk_tcp_lsn_slot* slots = nullptr;
    uint64_t* consumed = nullptr;  // one device word: never-used slots consumed
    dk::ctl::CallScratch call;  // serialisation, as a context's; its event is made with the table
};

namespace dk_tcp_listen {
namespace {
using namespace dk::ctl;

constexpr uint32_t kNone = DK_TCP_LSN_NONE;
constexpr uint64_t kMatrixBudget = 1u << 22;  // tiles x listeners words of the rank matrix
constexpr uint32_t kTileMin = 1024;           // frames per tile, at least

// What the lookup leaves per frame: kind | listener << 16.
enum Kind : uint32_t { kSkip = 0, kForward = 1, kOrphaned = 2, kSynRcvd = 3, kNoEntry = 4, kNoEntrySyn = 5 };

__host__ __device__ inline uint64_t mix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xFF51AFD7ED558CCDull;
    k ^= k >> 33;
    k *= 0xC4CEB9FE1A85EC53ull;
    k ^= k >> 33;
    return k;
}
__host__ __device__ inline uint64_t make_key(uint32_t l, uint32_t ip, uint32_t port) {
    return (uint64_t)(l & 0xFFFFu) << 48 | (uint64_t)ip << 16 | (port & 0xFFFFu);
}

__device__ __forceinline__ uint64_t cas64(uint64_t* p, uint64_t expect, uint64_t want) {
    __hip_atomic_compare_exchange_strong(p, &expect, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;  // the value found
}

struct Params {
    dk_tcp_lsn_slot* slots;
    uint64_t* consumed;
    uint32_t cap;
    dk_rx_results rx;
    uint32_t n;
    dk_tcp_listener* lst;
    uint32_t nl;
    const uint32_t* lsn_of_flow;
    uint32_t nflows;
    const uint32_t* link;
    const dk_tx_link* links;
    uint32_t nlinks;
    uint64_t now;
    uint8_t* out;
    uint64_t out_bytes;
    uint32_t stride, lead, max_frames, max_ready, flags;
    dk_tcp_lsn_results res;
    // scratch
    uint32_t H;  // group hash size (a power of two >= 2 n)
    uint64_t* gkey;
    uint32_t *gfirst, *gsecond, *gslot;
    uint32_t tile, ntiles;
    uint32_t* mat;     // [ntiles][nl]
    uint32_t* lcand;   // [nl] candidates
    uint32_t* lwork;   // [nl] the listener had a frame
    uint64_t* bsum_bl; // the device's sum of max_backlog
    uint32_t *grp, *tslot, *kind, *rank, *lisn;  // [n]
    uint8_t* act;                                 // [n]
    uint64_t *flag_r, *flag_y, *tot;              // [n], [n], [2]
};

__device__ __forceinline__ bool table_ok(const Params& P) { return 2 * *P.bsum_bl <= (uint64_t)P.cap; }
__device__ __forceinline__ bool fits(const Params& P) {
    return dk::tcp_tx_fits(P.tot[0], P.max_frames, P.stride, P.out_bytes) && P.tot[1] <= P.max_ready;
}

__device__ __forceinline__ uint32_t room_of(const dk_tcp_listener& L) {
    return L.max_backlog > L.inflight ? L.max_backlog - L.inflight : 0u;
}

// The SYN's options as the entry keeps them: mss | wscale << 16 (the last entry of each kind wins, :299-311).
__device__ uint32_t syn_options(const Params& P, uint32_t i) {
    uint32_t mss = DK_TCP_LSN_FALLBACK_MSS, ws = DK_TCP_LSN_NO_WSCALE;
    if ((P.rx.meta[i] >> 28) > 5) {  // the record is written for option-bearing segments only
        const dk_tcp_opts& o = P.rx.tcp_opts[i];
        const uint32_t num = o.num < 5 ? o.num : 5;
        for (uint32_t k = 0; k < num; k++) {
            if (o.opt[k].kind == DK_TCPOPT_MSS) mss = o.opt[k].u16;
            else if (o.opt[k].kind == DK_TCPOPT_WS) ws = o.opt[k].u8;
        }
    }
    return mss | ws << 16;
}

// The listener checks of dk_tcp.h, in its order.
__device__ __forceinline__ uint32_t listener_check(const Params& P, const dk_tcp_listener& L) {
    if (L.window_scale > 14) return DK_TCP_LSN_E_WSCALE;
    if (L.link >= P.nlinks) return DK_TCP_LSN_E_LINK;
    if ((uint64_t)P.lead + DK_TCP_LSN_SYNACK_BYTES > P.stride) return DK_TCP_LSN_E_SLOT;
    return DK_TCP_LSN_OK;
}

__global__ __launch_bounds__(kBlock) void lsn_check_kernel(Params P) {
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= P.nl) return;
    const dk_tcp_listener& L = P.lst[l];
    P.res.status[l] = listener_check(P, L);
    if (P.bsum_bl) add64(P.bsum_bl, L.max_backlog);
}

__global__ __launch_bounds__(kBlock) void lsn_lookup_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    uint32_t kind = kSkip, l = 0, g = kNone, ts = kNone;
    const uint32_t meta = P.rx.meta[i];
    const uint32_t f = P.rx.flow_id[i];
    if ((meta & 0xFFu) == DK_V_OK_TCP && f < P.nflows && table_ok(P)) {
        l = P.lsn_of_flow[f];
        if (l < P.nl && P.lst[l].state == DK_TCP_LSN_LISTENING && P.res.status[l] == DK_TCP_LSN_OK) {
            const uint64_t key = make_key(l, P.rx.src_ip[i], P.rx.ports[i] & 0xFFFFu);
            const uint32_t mask = P.cap - 1;
            uint32_t s = (uint32_t)mix64(key) & mask, st = DK_TCP_LSN_FREE;
            for (uint32_t p = 0; p < P.cap; p++, s = (s + 1) & mask) {
                const uint64_t k = P.slots[s].key;
                if (k == key) {
                    ts = s, st = P.slots[s].state;
                    break;
                }
                if (k == DK_TCP_LSN_KEY_FREE) break;
            }
            if (st == DK_TCP_LSN_ESTAB) kind = kForward;
            else if (st == DK_TCP_LSN_FAILED) kind = kOrphaned;
            else {
                const uint32_t fl = meta >> 16;  // byte 13: FIN 1, SYN 2, RST 4, ACK 16
                const bool syn = (fl & 2u) && !(fl & 16u) && !(fl & 4u);
                kind = st == DK_TCP_LSN_SYN_RCVD ? kSynRcvd : syn ? kNoEntrySyn : kNoEntry;
                const uint32_t hm = P.H - 1;
                uint32_t h = (uint32_t)(mix64(key) >> 32) & hm;
                for (uint32_t p = 0; p < P.H; p++, h = (h + 1) & hm) {
                    uint64_t cur = P.gkey[h];
                    if (cur == DK_TCP_LSN_KEY_FREE) cur = cas64(P.gkey + h, DK_TCP_LSN_KEY_FREE, key);
                    if (cur == DK_TCP_LSN_KEY_FREE || cur == key) {
                        g = h;
                        break;
                    }
                }
                if (g == kNone) kind = kSkip;  // unreachable: H >= 2 n
                else if (kind != kNoEntry) min32(P.gfirst + g, i);
            }
            if (kind != kSkip) P.lwork[l] = 1;
        }
    }
    P.kind[i] = kind | l << 16;
    P.grp[i] = g;
    P.tslot[i] = ts;
}

__device__ __forceinline__ bool is_candidate(const Params& P, uint32_t i, uint32_t kd) {
    return (kd & 0xFFFFu) == kNoEntrySyn && P.gfirst[P.grp[i]] == i;
}
// A candidate's rank among its listener's candidates, in frame order (after lsn_colscan_kernel).
__device__ __forceinline__ uint32_t final_rank(const Params& P, uint32_t first, uint32_t l) {
    return P.mat[(size_t)(first / P.tile) * P.nl + l] + P.rank[first];
}

// One wave per tile of frames, 64 frames a step: rank[i] = the candidate's rank within its tile and listener.
__global__ __launch_bounds__(kBlock) void lsn_rank_kernel(Params P) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t t = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (t >= P.ntiles) return;  // whole waves leave
    const uint32_t lo = t * P.tile, hi = min(P.n, lo + P.tile);
    for (uint32_t base = lo; base < hi; base += kWave) {
        const uint32_t i = base + lane;
        const uint32_t kd = i < hi ? P.kind[i] : 0u;
        const bool cand = i < hi && is_candidate(P, i, kd);
        const uint32_t l = kd >> 16;
        uint64_t todo = __ballot(cand), mine = 0;
        while (todo) {  // uniform: one round per distinct listener among the wave's candidates, registers only
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t ll = (uint32_t)__shfl((int)l, leader);
            const uint64_t m = __ballot(cand && l == ll);
            if (cand && l == ll) mine = m;
            todo &= ~m;
        }
        // one round trip a step: the first lane of every listener adds its group's count
        const int lead = cand ? __ffsll((long long)mine) - 1 : (int)lane;
        uint32_t b = 0;
        if (cand && (int)lane == lead) b = add32(P.mat + (size_t)t * P.nl + l, (uint32_t)__popcll(mine));
        b = (uint32_t)__shfl((int)b, lead);
        if (cand) P.rank[i] = b + (uint32_t)__popcll(mine & ((1ull << lane) - 1));
    }
}

// Per listener: its column of the matrix becomes the exclusive prefix over the tiles; lcand = its candidates.
__global__ __launch_bounds__(kBlock) void lsn_colscan_kernel(Params P) {
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= P.nl) return;
    uint32_t run = 0;
    constexpr uint32_t kAhead = 8;  // the loads of eight tiles are in flight together
    for (uint32_t t0 = 0; t0 < P.ntiles; t0 += kAhead) {
        uint32_t c[kAhead];
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) c[k] = t0 + k < P.ntiles ? P.mat[(size_t)(t0 + k) * P.nl + l] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < kAhead; k++) {
            if (t0 + k < P.ntiles) P.mat[(size_t)(t0 + k) * P.nl + l] = run;
            run += c[k];
        }
    }
    P.lcand[l] = run;
}

__global__ __launch_bounds__(kBlock) void lsn_second_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t kd = P.kind[i], k = kd & 0xFFFFu, l = kd >> 16;
    if (k != kNoEntry && k != kNoEntrySyn) return;
    const uint32_t g = P.grp[i], first = P.gfirst[g];
    if (first == kNone || i < first) return;
    const dk_tcp_listener& L = P.lst[l];
    const uint32_t r = final_rank(P, first, l);
    if (r >= room_of(L)) return;
    if (i == first) {
        const uint32_t crc = isn_crc(P.rx.src_ip[i], P.rx.ports[i] & 0xFFFFu, L.local_ip, L.local_port, L.nonce);
        P.lisn[i] = crc + (uint32_t)(uint16_t)(L.isn_counter + r);
    } else {
        min32(P.gsecond + g, i);
    }
}

// Whether the handshake segment `j` completes an entry whose local ISN is lisn.
__device__ __forceinline__ bool ack_ok(const Params& P, uint32_t j, uint32_t lisn) { return P.rx.tcp_ack[j] == lisn + 1u; }

__global__ __launch_bounds__(kBlock) void lsn_classify_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t kd = P.kind[i], k = kd & 0xFFFFu, l = kd >> 16;
    uint32_t act = DK_TCP_LSN_SKIP;
    bool reply = false, ready = false;
    const bool data = (P.rx.payload[i] >> 16) != 0;
    if (k == kForward) act = DK_TCP_LSN_FORWARD;
    else if (k == kOrphaned) act = DK_TCP_LSN_ORPHANED;
    else if (k == kSynRcvd) {
        const uint32_t first = P.gfirst[P.grp[i]], lisn = P.slots[P.tslot[i]].local_isn;
        if (i == first) {
            act = !ack_ok(P, i, lisn) ? DK_TCP_LSN_BAD_ACK : data ? DK_TCP_LSN_ESTABLISHED_DATA : DK_TCP_LSN_ESTABLISHED;
            ready = true;
        } else {
            act = ack_ok(P, first, lisn) ? DK_TCP_LSN_FORWARD : DK_TCP_LSN_ORPHANED;
        }
    } else if (k == kNoEntry || k == kNoEntrySyn) {
        const uint32_t g = P.grp[i], first = P.gfirst[g];
        const bool accepted = first != kNone && final_rank(P, first, l) < room_of(P.lst[l]);
        if (!accepted || i < first) {
            act = k == kNoEntrySyn ? DK_TCP_LSN_RST_BACKLOG : DK_TCP_LSN_RST_FLAGS;
            reply = true;
        } else if (i == first) {
            act = DK_TCP_LSN_SYN_ACCEPTED;
            reply = true;
        } else {
            const uint32_t second = P.gsecond[g], lisn = P.lisn[first];
            if (i == second) {
                act = !ack_ok(P, i, lisn) ? DK_TCP_LSN_BAD_ACK : data ? DK_TCP_LSN_ESTABLISHED_DATA : DK_TCP_LSN_ESTABLISHED;
                ready = true;
            } else {
                act = ack_ok(P, second, lisn) ? DK_TCP_LSN_FORWARD : DK_TCP_LSN_ORPHANED;
            }
        }
    }
    P.act[i] = (uint8_t)act;
    P.flag_r[i] = reply;
    P.flag_y[i] = ready;
}

// Behind the capacity test: the accepted keys go into the table, and every slot that changed gets its row.
__device__ __forceinline__ void commit_frame(const Params& P, uint32_t i, bool& fresh) {
    const uint32_t act = P.act[i], kd = P.kind[i], k = kd & 0xFFFFu, l = kd >> 16;
    if (act == DK_TCP_LSN_SYN_ACCEPTED) {
        const dk_tcp_listener& L = P.lst[l];
        const uint32_t g = P.grp[i];
        const uint64_t key = make_key(l, P.rx.src_ip[i], P.rx.ports[i] & 0xFFFFu);
        const uint32_t mask = P.cap - 1;
        uint32_t s = (uint32_t)mix64(key) & mask, got = kNone;
        for (uint32_t p = 0; p < P.cap && got == kNone; p++, s = (s + 1) & mask) {
            uint64_t* kw = &P.slots[s].key;
            const uint64_t cur = *kw;
            if (cur != DK_TCP_LSN_KEY_FREE && cur != DK_TCP_LSN_KEY_TOMBSTONE) continue;
            if (cas64(kw, cur, key) == cur) {
                got = s;
                if (cur == DK_TCP_LSN_KEY_FREE) fresh = true;
            }
        }
        P.gslot[g] = got;
        if (got == kNone) return;  // unreachable under the backlog rule
        const uint32_t second = P.gsecond[g], so = syn_options(P, i);
        dk_tcp_lsn_slot& S = P.slots[got];
        const uint32_t a2 = second == kNone ? 0u : P.act[second];
        S.state = second == kNone ? DK_TCP_LSN_SYN_RCVD : a2 == DK_TCP_LSN_BAD_ACK ? DK_TCP_LSN_FAILED : DK_TCP_LSN_ESTAB;
        S.err = a2 == DK_TCP_LSN_BAD_ACK ? EBADMSG : 0;
        S.remote_isn = P.rx.tcp_seq[i];
        S.local_isn = P.lisn[i];
        S.syn_window = (uint16_t)P.rx.tcp_win[i];
        S.mss = (uint16_t)so;
        S.remote_wscale = (uint8_t)(so >> 16);
        S.reserved0 = 0, S.reserved1 = 0, S.reserved2 = 0;
        S.retries_left = L.handshake_retries;
        S.deadline_ns = P.now + L.handshake_timeout_ns;
    } else if (k == kSynRcvd && P.gfirst[P.grp[i]] == i) {
        dk_tcp_lsn_slot& S = P.slots[P.tslot[i]];
        S.state = act == DK_TCP_LSN_BAD_ACK ? DK_TCP_LSN_FAILED : DK_TCP_LSN_ESTAB;
        S.err = act == DK_TCP_LSN_BAD_ACK ? EBADMSG : 0;
    }
}

__global__ __launch_bounds__(kBlock) void lsn_commit_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool fresh = false;  // claimed a never-used slot
    if (i < P.n && fits(P)) commit_frame(P, i, fresh);
    const uint64_t m = __ballot(fresh);  // one add a wave: a million adds to one word would queue up behind each other
    if (fresh && (threadIdx.x & (kWave - 1)) == (uint32_t)(__ffsll((long long)m) - 1)) add64(P.consumed, (uint64_t)__popcll(m));
}

__device__ void write_ready(dk_tcp_lsn_ready* R, uint32_t l, const dk_tcp_listener& L, uint32_t rip, uint32_t rport,
                            uint32_t err, uint32_t frame, uint32_t remote_isn, uint32_t local_isn, uint32_t syn_window,
                            uint32_t mss, uint32_t rws, uint32_t slot) {
    const bool has = rws != DK_TCP_LSN_NO_WSCALE;
    const uint32_t lws = has ? L.window_scale : 0u, rw = has ? (rws < 14 ? rws : 14u) : 0u;
    R->listener = l;
    R->remote_ip = rip;
    R->remote_port = (uint16_t)rport;
    R->err = (uint16_t)err;
    R->frame = frame;
    R->rcv_nxt = remote_isn + 1;
    R->snd_nxt = local_isn + 1;
    R->local_window = (uint32_t)L.receive_window_size << lws;
    R->remote_window = (syn_window & 0xFFFFu) << rw;
    R->mss = mss;
    R->local_wscale = (uint8_t)lws;
    R->remote_wscale = (uint8_t)rw;
    R->reserved0 = 0;
    R->slot = slot;
    R->reserved1 = 0;
}

// The frames, the ready records and the per-frame results. Reads the table's unchanging fields only.
__global__ __launch_bounds__(kBlock) void lsn_build_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n || !fits(P)) return;
    const uint32_t act = P.act[i], kd = P.kind[i], k = kd & 0xFFFFu, l = kd >> 16;
    uint32_t slot = kNone, rf = kNone;
    if (act != DK_TCP_LSN_SKIP) {
        const dk_tcp_listener& L = P.lst[l];
        const uint32_t g = P.grp[i], rip = P.rx.src_ip[i], rport = P.rx.ports[i] & 0xFFFFu;
        if (k == kForward || k == kOrphaned || k == kSynRcvd) slot = P.tslot[i];
        else if (act != DK_TCP_LSN_RST_FLAGS && act != DK_TCP_LSN_RST_BACKLOG) slot = P.gslot[g];
        if (act == DK_TCP_LSN_SYN_ACCEPTED || act == DK_TCP_LSN_RST_FLAGS || act == DK_TCP_LSN_RST_BACKLOG) {
            const uint64_t f = P.flag_r[i];
            rf = (uint32_t)f;
            const uint32_t foff = (uint32_t)(f * P.stride + P.lead);
            const bool sa = act == DK_TCP_LSN_SYN_ACCEPTED;
            uint32_t lk = L.link;
            if (P.link && P.link[i] < P.nlinks) lk = P.link[i];
            uint32_t seq, ack, b13 = 0x14u, win = 0;
            if (sa) {
                seq = P.lisn[i], ack = P.rx.tcp_seq[i] + 1u, b13 = 0x12u, win = L.receive_window_size;
            } else if ((P.rx.meta[i] >> 16) & 16u) {
                seq = P.rx.tcp_ack[i], ack = seq + 1u;
            } else {
                const uint32_t hb = (P.rx.meta[i] >> 28) > 5 ? dk::tx_tcp_header_bytes(P.rx.tcp_opts + i) : 20u;
                seq = 0, ack = P.rx.tcp_seq[i] + hb;
            }
            P.res.off_out[f] = foff;
            P.res.len_out[f] = (uint16_t)(sa ? DK_TCP_LSN_SYNACK_BYTES : DK_TCP_LSN_RST_BYTES);
            if (P.res.frame_seg) P.res.frame_seg[f] = i;
            tcp_frame(P.out + foff, P.links + lk, L.ip_word, L.local_ip, rip, L.local_port, rport, seq, ack, b13, win, sa,
                      L.advertised_mss, L.window_scale, (P.flags & DK_TX_OFFLOAD_TCP) != 0);
        } else if (act == DK_TCP_LSN_ESTABLISHED || act == DK_TCP_LSN_ESTABLISHED_DATA || act == DK_TCP_LSN_BAD_ACK) {
            const uint32_t err = act == DK_TCP_LSN_BAD_ACK ? EBADMSG : 0;
            dk_tcp_lsn_ready* R = P.res.ready + P.flag_y[i];
            if (k == kSynRcvd) {
                const dk_tcp_lsn_slot& S = P.slots[slot];
                write_ready(R, l, L, rip, rport, err, i, S.remote_isn, S.local_isn, S.syn_window, S.mss, S.remote_wscale,
                            slot);
            } else {
                const uint32_t first = P.gfirst[g], so = syn_options(P, first);
                write_ready(R, l, L, rip, rport, err, i, P.rx.tcp_seq[first], P.lisn[first], P.rx.tcp_win[first],
                            so & 0xFFFFu, so >> 16, slot);
            }
        }
    }
    P.res.action[i] = (uint8_t)act;
    P.res.slot[i] = slot;
    P.res.reply_frame[i] = rf;
}

// The listeners' two fields and statuses, the two words.
__global__ __launch_bounds__(kBlock) void lsn_finish_kernel(Params P) {
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    const bool ok = fits(P);
    if (l == 0) {
        *P.res.n_frames = (uint32_t)P.tot[0];
        *P.res.n_ready = (uint32_t)P.tot[1];
    }
    if (l >= P.nl) return;
    if (P.bsum_bl && !table_ok(P)) {
        P.res.status[l] = DK_TCP_LSN_E_TABLE;
        return;
    }
    if (P.res.status[l] != DK_TCP_LSN_OK || !P.lwork[l]) return;
    if (!ok) {
        P.res.status[l] = DK_TCP_LSN_NO_ROOM;
        return;
    }
    if (!P.lcand) return;  // dk_tcp_listen_timers moves no listener field
    dk_tcp_listener& L = P.lst[l];
    const uint32_t took = min(P.lcand[l], room_of(L));
    L.inflight += took;
    L.isn_counter = (uint16_t)(L.isn_counter + took);
}

// dk_tcp_listen_timers. Slots take the place of frames: flag_r = the slot resends, flag_y = it times out.
__global__ __launch_bounds__(kBlock) void lsn_sweep_kernel(Params P) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P.cap) return;
    const dk_tcp_lsn_slot& S = P.slots[s];
    bool due = false;
    if (S.state == DK_TCP_LSN_SYN_RCVD && S.deadline_ns <= P.now) {
        const uint32_t l = (uint32_t)(S.key >> 48);
        if (l < P.nl && P.lst[l].state == DK_TCP_LSN_LISTENING && P.res.status[l] == DK_TCP_LSN_OK) {
            due = true;
            P.lwork[l] = 1;
        }
    }
    P.flag_r[s] = due && S.retries_left > 0;
    P.flag_y[s] = due && S.retries_left == 0;
}

__global__ __launch_bounds__(kBlock) void lsn_expire_kernel(Params P) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P.cap || !fits(P)) return;
    const uint64_t f = P.flag_r[s], y = P.flag_y[s];
    const bool resend = (s + 1 < P.cap ? P.flag_r[s + 1] : P.tot[0]) != f;
    const bool fail = (s + 1 < P.cap ? P.flag_y[s + 1] : P.tot[1]) != y;
    if (!resend && !fail) return;
    dk_tcp_lsn_slot& S = P.slots[s];
    const uint32_t l = (uint32_t)(S.key >> 48), rip = (uint32_t)(S.key >> 16), rport = (uint32_t)S.key & 0xFFFFu;
    const dk_tcp_listener& L = P.lst[l];
    if (resend) {
        S.retries_left -= 1;
        S.deadline_ns = P.now + L.handshake_timeout_ns;
        const uint32_t foff = (uint32_t)(f * P.stride + P.lead);
        P.res.off_out[f] = foff;
        P.res.len_out[f] = (uint16_t)DK_TCP_LSN_SYNACK_BYTES;
        if (P.res.frame_seg) P.res.frame_seg[f] = s;
        tcp_frame(P.out + foff, P.links + L.link, L.ip_word, L.local_ip, rip, L.local_port, rport, S.local_isn,
                  S.remote_isn + 1u, 0x12u, L.receive_window_size, true, L.advertised_mss, L.window_scale,
                  (P.flags & DK_TX_OFFLOAD_TCP) != 0);
    } else {
        S.state = DK_TCP_LSN_FAILED;
        S.err = ETIMEDOUT;
        write_ready(P.res.ready + y, l, L, rip, rport, ETIMEDOUT, kNone, S.remote_isn, S.local_isn, S.syn_window, S.mss,
                    S.remote_wscale, s);
    }
}

__global__ __launch_bounds__(kBlock) void lsn_release_kernel(dk_tcp_lsn_slot* slots, uint32_t cap, dk_tcp_listener* lst,
                                                             uint32_t nl, const uint64_t* keys, uint32_t nkeys,
                                                             uint32_t* found) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nkeys) return;
    const uint64_t key = keys[j];
    uint32_t hit = 0;
    const uint32_t l = (uint32_t)(key >> 48);
    if (l < nl && key != DK_TCP_LSN_KEY_TOMBSTONE) {
        const uint32_t mask = cap - 1;
        uint32_t s = (uint32_t)mix64(key) & mask;
        for (uint32_t p = 0; p < cap; p++, s = (s + 1) & mask) {
            const uint64_t k = slots[s].key;
            if (k == DK_TCP_LSN_KEY_FREE) break;
            if (k != key) continue;
            if (cas64(&slots[s].key, key, DK_TCP_LSN_KEY_TOMBSTONE) == key) {  // one of two equal keys wins
                dk_tcp_lsn_slot& S = slots[s];
                S.state = DK_TCP_LSN_TOMBSTONE;
                S.err = 0, S.remote_isn = 0, S.local_isn = 0, S.syn_window = 0, S.mss = 0, S.remote_wscale = 0;
                S.reserved0 = 0, S.reserved1 = 0, S.retries_left = 0, S.reserved2 = 0, S.deadline_ns = 0;
                add32(&lst[l].inflight, 0xFFFFFFFFu);
                hit = 1;
            }
            break;
        }
    }
    found[j] = hit;
}

}  // namespace
}  // namespace dk_tcp_listen

extern "C" {

uint64_t dk_tcp_listen_key(uint32_t listener, uint32_t remote_ip, uint16_t remote_port) {
    return dk_tcp_listen::make_key(listener, remote_ip, remote_port);
}

uint32_t dk_tcp_listen_home(uint32_t cap, uint64_t key) {
    return cap ? (uint32_t)dk_tcp_listen::mix64(key) & (cap - 1) : 0u;
}

int dk_tcp_listen_backlog_fits(uint32_t cap, uint64_t backlog_sum) {
    return backlog_sum <= (uint64_t)cap / 2 ? 0 : EINVAL;
}

int dk_tcp_listen_table_create(int32_t device, uint32_t cap, dk_tcp_listen_table** out) {
    using namespace dk_tcp_listen;
    if (!out || cap < 2 || (cap & (cap - 1))) return EINVAL;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return EINVAL;
    DeviceGuard g(device);
    dk_tcp_listen_table* t = new dk_tcp_listen_table();
    t->device = device, t->cap = cap;
    std::vector<dk_tcp_lsn_slot> rows(cap);
    std::memset(rows.data(), 0, rows.size() * sizeof(dk_tcp_lsn_slot));
    for (auto& r : rows) r.key = DK_TCP_LSN_KEY_FREE;
    const uint64_t zero = 0;
    if (hipMalloc(&t->slots, (size_t)cap * sizeof(dk_tcp_lsn_slot)) != hipSuccess ||
        hipMalloc(&t->consumed, sizeof(uint64_t)) != hipSuccess ||
        hipEventCreateWithFlags(&t->call.last, hipEventDisableTiming) != hipSuccess ||
        hipMemcpy(t->slots, rows.data(), rows.size() * sizeof(dk_tcp_lsn_slot), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t->consumed, &zero, sizeof(zero), hipMemcpyHostToDevice) != hipSuccess) {
        dk_tcp_listen_table_destroy(t);
        return ENOMEM;
    }
    *out = t;
    return 0;
}

void dk_tcp_listen_table_destroy(dk_tcp_listen_table* t) {
    if (!t) return;
    dk::ctl::DeviceGuard g(t->device);
    (void)t->call.drain();
    if (t->slots) (void)hipFree(t->slots);
    if (t->consumed) (void)hipFree(t->consumed);
    t->call.scratch.free();
    if (t->call.last) (void)hipEventDestroy(t->call.last);
    delete t;
}

int dk_tcp_listen_table_stats(dk_tcp_listen_table* t, uint32_t* cap, uint64_t* consumed) {
    if (!t) return EINVAL;
    dk::ctl::DeviceGuard g(t->device);
    if (cap) *cap = t->cap;
    if (consumed) {
        if (t->call.drain()) return EIO;
        if (hipMemcpy(consumed, t->consumed, sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return EIO;
    }
    return 0;
}

int dk_tcp_listen_table_read(dk_tcp_listen_table* t, dk_tcp_lsn_slot* rows) {
    if (!t || !rows) return EINVAL;
    dk::ctl::DeviceGuard g(t->device);
    if (t->call.drain()) return EIO;
    return hipMemcpy(rows, t->slots, (size_t)t->cap * sizeof(dk_tcp_lsn_slot), hipMemcpyDeviceToHost) == hipSuccess ? 0
                                                                                                                     : EIO;
}

int dk_tcp_listen_table_write(dk_tcp_listen_table* t, const dk_tcp_lsn_slot* rows) {
    if (!t || !rows) return EINVAL;
    dk::ctl::DeviceGuard g(t->device);
    if (t->call.drain()) return EIO;
    uint64_t consumed = 0;
    for (uint32_t s = 0; s < t->cap; s++) consumed += rows[s].state != DK_TCP_LSN_FREE;
    if (hipMemcpy(t->slots, rows, (size_t)t->cap * sizeof(dk_tcp_lsn_slot), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t->consumed, &consumed, sizeof(consumed), hipMemcpyHostToDevice) != hipSuccess)
        return EIO;
    return 0;
}

int dk_tcp_listen_process(dk_tcp_listen_table* t, const dk_rx_results* rx, uint32_t n, dk_tcp_listener* listeners,
                          uint32_t nl, uint64_t backlog_sum, const uint32_t* lsn_of_flow, uint32_t nflows,
                          const uint32_t* link, const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns, uint8_t* out,
                          uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready,
                          uint32_t flags, const dk_tcp_lsn_results* res, void* stream) {
    using namespace dk_tcp_listen;
    if (!t || !rx || !layout || !res || !res->n_frames || !res->n_ready || !links || nlinks == 0) return EINVAL;
    if (out_bytes > DK_RX_MAX_BLOB || nl > DK_TCP_LSN_MAX_LISTENERS || n > 0x7FFFFFFFu) return EINVAL;
    if (dk_tcp_listen_backlog_fits(t->cap, backlog_sum)) return EINVAL;
    if (nl && (!listeners || !res->status)) return EINVAL;
    if (reinterpret_cast<uintptr_t>(listeners) & 15) return EINVAL;
    if (n && (!rx->meta || !rx->src_ip || !rx->ports || !rx->payload || !rx->flow_id || !rx->tcp_seq || !rx->tcp_ack ||
              !rx->tcp_win || !rx->tcp_opts || !res->action || !res->slot || !res->reply_frame))
        return EINVAL;
    if (n && nl && ((nflows && !lsn_of_flow) || (max_frames && (!out || !res->off_out || !res->len_out)) ||
                    (max_ready && !res->ready)))
        return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    uint32_t H = 2;
    while (H < 2ull * n) H <<= 1;
    uint32_t tile = kTileMin;
    if ((uint64_t)n * nl > kMatrixBudget * (uint64_t)tile)
        tile = (uint32_t)((((uint64_t)n * nl + kMatrixBudget - 1) / kMatrixBudget + kWave - 1) / kWave * kWave);
    const uint32_t ntiles = n ? (n + tile - 1) / tile : 0, sb = dk_tcp_tx_scan_tiles(n);
    const size_t ff_bytes = round16((size_t)H * 8) + 3 * round16((size_t)H * 4);
    const size_t zero_bytes = round16((size_t)ntiles * nl * 4) + 2 * round16((size_t)nl * 4) + round16(8) + round16(16);
    const size_t need = ff_bytes + zero_bytes + 5 * round16((size_t)n * 4) + round16(n) + 2 * round16((size_t)n * 8) +
                        round16((size_t)sb * 8) + 16;
    if (int rc = t->call.grow(need)) return rc;
    if (t->call.order(s)) return EIO;
    Params P{};
    P.slots = t->slots, P.consumed = t->consumed, P.cap = t->cap;
    P.rx = *rx, P.n = n, P.lst = listeners, P.nl = nl, P.lsn_of_flow = lsn_of_flow, P.nflows = nflows;
    P.link = link, P.links = links, P.nlinks = nlinks, P.now = now_ns;
    P.out = out, P.out_bytes = out_bytes, P.stride = layout->slot_stride, P.lead = layout->frame_lead;
    P.max_frames = max_frames, P.max_ready = max_ready, P.flags = flags, P.res = *res;
    P.H = H, P.tile = tile, P.ntiles = ntiles;
    Carver c{t->call.scratch.p};
    uint8_t* ff = c.b;
    P.gkey = c.take<uint64_t>(H);
    P.gfirst = c.take<uint32_t>(H);
    P.gsecond = c.take<uint32_t>(H);
    P.gslot = c.take<uint32_t>(H);
    uint8_t* zz = c.b;
    P.mat = c.take<uint32_t>((size_t)ntiles * nl);
    P.lcand = c.take<uint32_t>(nl);
    P.lwork = c.take<uint32_t>(nl);
    P.bsum_bl = c.take<uint64_t>(1);
    P.tot = c.take<uint64_t>(2);
    P.grp = c.take<uint32_t>(n);
    P.tslot = c.take<uint32_t>(n);
    P.kind = c.take<uint32_t>(n);
    P.rank = c.take<uint32_t>(n);
    P.lisn = c.take<uint32_t>(n);
    P.act = c.take<uint8_t>(n);
    P.flag_r = c.take<uint64_t>(n);
    P.flag_y = c.take<uint64_t>(n);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if (hipMemsetAsync(ff, 0xFF, ff_bytes, s) != hipSuccess || hipMemsetAsync(zz, 0, zero_bytes, s) != hipSuccess)
        return EIO;
    if (nl) hipLaunchKernelGGL(lsn_check_kernel, grid_for(nl), dim3(kBlock), 0, s, P);
    if (n && nl) {
        hipLaunchKernelGGL(lsn_lookup_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(lsn_rank_kernel, dim3((ntiles + kBlock / kWave - 1) / (kBlock / kWave)), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(lsn_colscan_kernel, grid_for(nl), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(lsn_second_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(lsn_classify_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, n, bsum, P.tot, s) || dk_tcp_tx_scan(P.flag_y, n, bsum, P.tot + 1, s)) return EIO;
        hipLaunchKernelGGL(lsn_commit_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(lsn_build_kernel, grid_for(n), dim3(kBlock), 0, s, P);
    } else if (n) {  // no listener: every frame is SKIP
        if (hipMemsetAsync(res->action, 0, n, s) != hipSuccess ||
            hipMemsetAsync(res->slot, 0xFF, (size_t)n * 4, s) != hipSuccess ||
            hipMemsetAsync(res->reply_frame, 0xFF, (size_t)n * 4, s) != hipSuccess)
            return EIO;
    }
    hipLaunchKernelGGL(lsn_finish_kernel, grid_for(nl), dim3(kBlock), 0, s, P);
    return t->call.record(s);
}

int dk_tcp_listen_timers(dk_tcp_listen_table* t, const dk_tcp_listener* listeners, uint32_t nl, uint64_t backlog_sum,
                         const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns, uint8_t* out, uint64_t out_bytes,
                         const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready, uint32_t flags,
                         const dk_tcp_lsn_results* res, void* stream) {
    using namespace dk_tcp_listen;
    if (!t || !layout || !res || !res->n_frames || !res->n_ready || !links || nlinks == 0) return EINVAL;
    if (out_bytes > DK_RX_MAX_BLOB || nl > DK_TCP_LSN_MAX_LISTENERS) return EINVAL;
    if (dk_tcp_listen_backlog_fits(t->cap, backlog_sum)) return EINVAL;
    if (nl && (!listeners || !res->status)) return EINVAL;
    if (reinterpret_cast<uintptr_t>(listeners) & 15) return EINVAL;
    if (nl && ((max_frames && (!out || !res->off_out || !res->len_out)) || (max_ready && !res->ready))) return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t cap = t->cap, sb = dk_tcp_tx_scan_tiles(cap);
    const size_t zero_bytes = round16((size_t)nl * 4) + round16(16);
    const size_t need = zero_bytes + 2 * round16((size_t)cap * 8) + round16((size_t)sb * 8) + 16;
    if (int rc = t->call.grow(need)) return rc;
    if (t->call.order(s)) return EIO;
    Params P{};
    P.slots = t->slots, P.consumed = t->consumed, P.cap = cap;
    P.lst = const_cast<dk_tcp_listener*>(listeners), P.nl = nl;  // lcand == nullptr: the finish kernel writes no row
    P.links = links, P.nlinks = nlinks, P.now = now_ns;
    P.out = out, P.out_bytes = out_bytes, P.stride = layout->slot_stride, P.lead = layout->frame_lead;
    P.max_frames = max_frames, P.max_ready = max_ready, P.flags = flags, P.res = *res;
    Carver c{t->call.scratch.p};
    uint8_t* zz = c.b;
    P.lwork = c.take<uint32_t>(nl);
    P.tot = c.take<uint64_t>(2);
    P.flag_r = c.take<uint64_t>(cap);
    P.flag_y = c.take<uint64_t>(cap);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if (hipMemsetAsync(zz, 0, zero_bytes, s) != hipSuccess) return EIO;
    if (nl) {
        hipLaunchKernelGGL(lsn_check_kernel, grid_for(nl), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(lsn_sweep_kernel, grid_for(cap), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, cap, bsum, P.tot, s) || dk_tcp_tx_scan(P.flag_y, cap, bsum, P.tot + 1, s)) return EIO;
        hipLaunchKernelGGL(lsn_expire_kernel, grid_for(cap), dim3(kBlock), 0, s, P);
    }
    hipLaunchKernelGGL(lsn_finish_kernel, grid_for(nl), dim3(kBlock), 0, s, P);
    return t->call.record(s);
}

int dk_tcp_listen_release(dk_tcp_listen_table* t, dk_tcp_listener* listeners, uint32_t nl, const uint64_t* keys,
                          uint32_t nkeys, uint32_t* found, void* stream) {
    using namespace dk_tcp_listen;
    if (!t || nl > DK_TCP_LSN_MAX_LISTENERS) return EINVAL;
    if (nkeys && (!keys || !found || !listeners)) return EINVAL;
    if (reinterpret_cast<uintptr_t>(listeners) & 15) return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    if (t->call.order(s)) return EIO;
    if (nkeys) hipLaunchKernelGGL(lsn_release_kernel, grid_for(nkeys), dim3(kBlock), 0, s, t->slots, t->cap, listeners, nl,
                                  keys, nkeys, found);
    return t->call.record(s);
}

}  // extern "C"
