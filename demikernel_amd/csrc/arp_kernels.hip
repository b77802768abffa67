// arp_kernels.hip — the ARP peer on the GPU (include/dk_arp.h): SharedArpPeer::poll over a whole receive batch, query()
// up to its first await, the request timeout, try_query, and the HashTtlCache behind them as an open-addressing table
// in device memory.
//
// dk_arp_process follows the header's formulation: at a fixed clock a frame's outcome depends on f0 (the first covered
// frame whose sender has any entry or whose target is local), on whether its sender has a live entry, and on L(s), the
// first frame at or after f0 of its sender s that is addressed to us. So:
//   1. arp_classify_kernel   per frame: the sender's table slot (a read-only probe), its place in the call's own sender
//                            map (a scratch hash table of 2 n slots, claimed by one 64-bit compare-and-swap), and a
//                            32-bit atomicMin for f0.
//   2. arp_mark_kernel       per frame at or after f0: atomicMin / atomicMax per sender for its first and last frame
//                            and for L(s).
//   3. arp_decide_kernel     per frame: the action bits and whether a reply goes out; one scan numbers the replies.
//   4. arp_senders_kernel    per sender that inserts: its slot is kept (updated in place) or counted as new;
//      arp_census_kernel     per table slot: LIVE slots, and the expired ones that cleanup() removes at f0.
//   5. arp_rows_kernel       per WAITING row: the frame that wakes it, as a sort key; a stable radix sort of
//                            (frame, row) orders the ready records by waking frame and by row within one frame.
//   6. behind the call's one capacity test, made on the device: arp_build_kernel (per-frame results, replies),
//      arp_tomb_kernel (cleanup), arp_store_kernel (updates in place; inserts claim the first slot of the walk that is
//      not LIVE by a compare-and-swap on its state), arp_wake_kernel (rows, links, ready records), arp_finish_kernel.
// dk_arp_query_start and dk_arp_timers are flag, scan, build over start[] entries and rows. No loop depends on another
// workgroup's progress. Atomics are agent-scope integer __hip_atomic_* on global memory; everything else is plain
// vector loads and stores.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <cerrno>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dk_arp.h"
#include "ctl_common.h"

struct dk_arp_table {
    int device = 0;
    uint32_t cap = 0;
    dk_arp_cfg cfg{};
    dk_arp_slot* slots = nullptr;
    uint64_t* consumed = nullptr;  // one device word: never-used slots consumed
    dk::ctl::CallScratch call;  // serialisation, as a context's; its event is made with the table
};

namespace dk_arp {
namespace {
using namespace dk::ctl;

constexpr uint32_t kNone = DK_ARP_NONE;
constexpr uint32_t kBusy = 3;  // a slot an insert of this launch has claimed and not yet published
enum Tot : uint32_t { kFrames = 0, kReady = 1, kNew = 2, kRemoved = 3, kLive = 4, kTots = 5 };
enum Mode : uint32_t { kProcess = 0, kStart = 1, kTimers = 2 };

__host__ __device__ inline uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// The slot that holds ip, or kNone: the walk crosses tombstones and ends at a FREE slot or after cap steps.
__host__ __device__ inline uint32_t find_slot(const dk_arp_slot* S, uint32_t cap, uint32_t ip) {
    uint32_t s = mix32(ip) & (cap - 1);
    for (uint32_t k = 0; k < cap; k++, s = (s + 1) & (cap - 1)) {
        const uint32_t st = S[s].state;
        if (st == DK_ARP_SLOT_FREE) return kNone;
        if (st == DK_ARP_SLOT_LIVE && S[s].ip == ip) return s;
    }
    return kNone;
}

struct Params {
    dk_arp_slot* slots;
    uint32_t cap;
    uint64_t* consumed;
    dk_arp_cfg cfg;
    const uint8_t* frames;
    uint64_t frames_bytes;
    const uint32_t* off;
    const uint32_t *meta, *src, *dst;
    uint32_t n;
    dk_arp_query* rows;
    uint32_t nrows;
    dk_tx_link* links;
    uint32_t nlinks;
    const uint32_t* start;
    uint32_t nstart;
    uint64_t clock, now;
    uint8_t* out;
    uint64_t out_bytes;
    uint32_t stride, lead, max_frames, max_ready;
    dk_arp_results res;
    // scratch
    uint64_t* hkey;  // [hcap] the call's sender map: 1 << 32 | spa, 0 = empty
    uint32_t hcap;
    uint32_t *hL, *hfirst, *hlast, *hts;  // [hcap] L(s); the sender's first and last frame at or after f0; its table slot
    uint8_t* hfl;                         // [hcap] bit 0: the sender has an entry, bit 1: a live one
    uint32_t* sslot;                      // [n] the frame's place in the sender map, kNone: not covered
    uint8_t* act;                         // [items] the decision, written to the results behind the capacity test
    uint64_t *flag_r, *flag_y;            // [items] frames, ready records
    uint8_t* keep;                        // [cap] the slot's key inserts in this call: updated in place
    uint64_t* tot;                        // [kTots]
    uint32_t* f0;
    uint32_t *keys, *skeys, *svals;  // [nrows] the waking frame per row; sorted; the rows in that order
    uint32_t* term;                  // [nrows] start: the first entry that names the row
    uint32_t* ts;                    // [items] start, timers: the table slot of the row's address
};

__device__ __forceinline__ bool disabled(const Params& P) { return (P.cfg.flags & DK_ARP_DISABLED) != 0; }
__device__ __forceinline__ bool slot_room(const Params& P) { return (uint64_t)P.lead + DK_ARP_FRAME_BYTES <= P.stride; }
__device__ __forceinline__ uint64_t entries(const Params& P) { return P.tot[kLive] - P.tot[kRemoved] + P.tot[kNew]; }
__device__ __forceinline__ bool fits(const Params& P) {
    return dk::tcp_tx_fits(P.tot[kFrames], P.max_frames, P.stride, P.out_bytes) && P.tot[kReady] <= P.max_ready &&
           entries(P) <= P.cap / 2 && (P.tot[kFrames] == 0 || slot_room(P));
}

// One add per wave of the lanes that hold `pred`. Every lane of the wave calls it.
__device__ __forceinline__ void count(uint64_t* p, bool pred) {
    const uint64_t b = __ballot(pred);
    if (b && (threadIdx.x & (kWave - 1)) == (uint32_t)(__ffsll((long long)b) - 1))
        __hip_atomic_fetch_add(p, (uint64_t)__popcll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct Mac {
    uint8_t b[6];
};
__device__ __forceinline__ Mac frame_sha(const Params& P, uint32_t i) {
    Mac m;
    const uint8_t* f = P.frames + P.off[i] + 22;
#pragma unroll
    for (int k = 0; k < 6; k++) m.b[k] = f[k];
    return m;
}
__device__ __forceinline__ Mac slot_mac(const Params& P, uint32_t s) {
    Mac m;
#pragma unroll
    for (int k = 0; k < 6; k++) m.b[k] = s == kNone ? (uint8_t)0 : P.slots[s].mac[k];
    return m;
}
__device__ __forceinline__ void put_mac(uint8_t* d, const Mac& m) {
#pragma unroll
    for (int k = 0; k < 6; k++) d[k] = m.b[k];
}

// Frame f of the call: 42 bytes, Ethernet2 + the ARP PDU. op 1: a request for `ip`; op 2: the reply to (tha, ip).
__device__ void emit_frame(const Params& P, uint64_t f, uint32_t seg, uint32_t op, const Mac& tha, uint32_t ip) {
    const uint32_t foff = (uint32_t)(f * P.stride + P.lead);
    P.res.off_out[f] = foff;
    P.res.len_out[f] = (uint16_t)DK_ARP_FRAME_BYTES;
    if (P.res.frame_seg) P.res.frame_seg[f] = seg;
    uint8_t* a = P.out + foff;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const uint8_t t = op == 1 ? (uint8_t)0xFF : tha.b[k];
        a[k] = t;
        a[6 + k] = P.cfg.local_mac[k];
        a[22 + k] = P.cfg.local_mac[k];
        a[32 + k] = t;
    }
    a[12] = 0x08, a[13] = 0x06;
    a[14] = 0x00, a[15] = 0x01, a[16] = 0x08, a[17] = 0x00, a[18] = 6, a[19] = 4, a[20] = 0, a[21] = (uint8_t)op;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        a[28 + k] = (uint8_t)(P.cfg.local_ip >> (8 * k));
        a[38 + k] = (uint8_t)(ip >> (8 * k));
    }
}

__device__ void write_ready(const Params& P, uint64_t y, uint32_t r, const dk_arp_query& R, uint32_t frame, const Mac& m,
                            uint32_t err) {
    dk_arp_ready* Y = P.res.ready + y;
    Y->row = r, Y->tag = R.tag, Y->ip = R.ip, Y->frame = frame;
    put_mac(Y->mac, m);
    Y->err = (uint16_t)err;
}

// A row's query resolves: the row, its link.
__device__ void resolve_row(const Params& P, dk_arp_query& R, const Mac& m) {
    R.state = DK_ARP_Q_RESOLVED, R.err = 0;
    put_mac(R.mac, m);
    if (R.link != DK_ARP_NO_LINK && R.link < P.nlinks) put_mac(P.links[R.link].dst_mac, m);
}

// ---- dk_arp_process -------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool covered(const Params& P, uint32_t i) {
    return (P.meta[i] & 0xFFu) == DK_V_ARP && (uint64_t)P.off[i] + 28 <= P.frames_bytes;
}

__global__ __launch_bounds__(kBlock) void arp_classify_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    uint32_t h = kNone;
    if (covered(P, i)) {
        const uint32_t spa = P.src[i];
        uint32_t ts = kNone;
        bool pres = true, live = true;
        if (!disabled(P)) {
            ts = find_slot(P.slots, P.cap, spa);
            pres = ts != kNone;
            live = pres && P.slots[ts].expiration_ns > P.clock;
        }
        const uint64_t key = 1ull << 32 | spa;
        h = mix32(spa) & (P.hcap - 1);
        for (uint32_t k = 0; k < P.hcap; k++, h = (h + 1) & (P.hcap - 1)) {  // hcap >= 2 n: an empty slot exists
            uint64_t cur = 0;
            if (__hip_atomic_compare_exchange_strong(P.hkey + h, &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT) ||
                cur == key)
                break;
        }
        P.hts[h] = ts;  // every frame of a sender stores the same two values
        P.hfl[h] = (uint8_t)((pres ? 1u : 0u) | (live ? 2u : 0u));
        if (pres || P.dst[i] == P.cfg.local_ip) min32(P.f0, i);
    }
    P.sslot[i] = h;
}

__global__ __launch_bounds__(kBlock) void arp_mark_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t h = P.sslot[i];
    if (h == kNone || i < *P.f0) return;
    min32(P.hfirst + h, i);
    max32(P.hlast + h, i);
    if (P.dst[i] == P.cfg.local_ip) min32(P.hL + h, i);
}

// base(s) of the header.
__device__ __forceinline__ bool sender_base(const Params& P, uint32_t h) {
    const uint32_t fl = P.hfl[h], f0 = *P.f0;
    return (fl & 2u) || ((fl & 1u) && f0 != kNone && P.sslot[f0] == h);
}
// The first frame of sender h that inserts, kNone if none does.
__device__ __forceinline__ uint32_t sender_first(const Params& P, uint32_t h) {
    if (*P.f0 == kNone) return kNone;
    return sender_base(P, h) ? P.hfirst[h] : P.hL[h];
}

__global__ __launch_bounds__(kBlock) void arp_decide_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t h = P.sslot[i];
    uint32_t act = DK_ARP_SKIP;
    if (h != kNone) {
        if (i < *P.f0) {
            act = DK_ARP_DROPPED;
        } else {
            const bool hit = sender_base(P, h) || i > P.hL[h], local = P.dst[i] == P.cfg.local_ip;
            if (hit) act |= DK_ARP_HIT | DK_ARP_INSERTED;
            else if (local) act |= DK_ARP_LEARNED | DK_ARP_INSERTED;
            else act |= DK_ARP_DROPPED;
            if (local && (P.meta[i] >> 16) == 1u) act |= DK_ARP_REPLY;
        }
    }
    P.act[i] = (uint8_t)act;
    P.flag_r[i] = (act & DK_ARP_REPLY) != 0;
}

__global__ __launch_bounds__(kBlock) void arp_senders_kernel(Params P) {
    const uint32_t h = blockIdx.x * kBlock + threadIdx.x;
    bool fresh = false;
    if (h < P.hcap && P.hkey[h] != 0 && !disabled(P) && sender_first(P, h) != kNone) {
        const uint32_t ts = P.hts[h];
        if (ts != kNone) P.keep[ts] = 1;
        else fresh = true;
    }
    count(P.tot + kNew, fresh);
}

__global__ __launch_bounds__(kBlock) void arp_census_kernel(Params P, uint32_t cleans) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    bool live = false, gone = false;
    if (s < P.cap) {
        live = P.slots[s].state == DK_ARP_SLOT_LIVE;
        gone = cleans && live && !disabled(P) && *P.f0 != kNone && P.slots[s].expiration_ns <= P.clock && !P.keep[s];
    }
    count(P.tot + kLive, live);
    count(P.tot + kRemoved, gone);
}

__global__ __launch_bounds__(kBlock) void arp_rows_kernel(Params P) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    uint32_t key = kNone;
    if (r < P.nrows && P.rows[r].state == DK_ARP_Q_WAITING) {
        const uint32_t ip = P.rows[r].ip;
        const uint64_t want = 1ull << 32 | ip;
        uint32_t h = mix32(ip) & (P.hcap - 1);
        for (uint32_t k = 0; k < P.hcap; k++, h = (h + 1) & (P.hcap - 1)) {
            const uint64_t cur = P.hkey[h];
            if (cur == 0) break;
            if (cur == want) {
                key = sender_first(P, h);
                break;
            }
        }
    }
    if (r < P.nrows) P.keys[r] = key;
    count(P.tot + kReady, key != kNone);
}

__global__ __launch_bounds__(kBlock) void arp_build_kernel(Params P) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n || !fits(P)) return;
    const uint32_t act = P.act[i];
    uint32_t rf = kNone;
    if (act & DK_ARP_REPLY) {
        rf = (uint32_t)P.flag_r[i];
        emit_frame(P, P.flag_r[i], i, 2u, frame_sha(P, i), P.src[i]);
    }
    P.res.action[i] = (uint8_t)act;
    P.res.reply_frame[i] = rf;
}

// cleanup() at f0.
__global__ __launch_bounds__(kBlock) void arp_tomb_kernel(Params P) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P.cap || !fits(P) || disabled(P) || *P.f0 == kNone) return;
    dk_arp_slot& S = P.slots[s];
    if (S.state != DK_ARP_SLOT_LIVE || S.expiration_ns > P.clock || P.keep[s]) return;
    S.state = DK_ARP_SLOT_TOMBSTONE, S.ip = 0, S.reserved = 0, S.expiration_ns = 0;
    put_mac(S.mac, Mac{});
}

// Per sender that inserts: the entry ends with the sha of its last frame and expiration clock + ttl.
__global__ __launch_bounds__(kBlock) void arp_store_kernel(Params P) {
    const uint32_t h = blockIdx.x * kBlock + threadIdx.x;
    if (h >= P.hcap || P.hkey[h] == 0 || !fits(P) || disabled(P) || sender_first(P, h) == kNone) return;
    const uint32_t ip = (uint32_t)P.hkey[h];
    const Mac m = frame_sha(P, P.hlast[h]);
    uint32_t s = P.hts[h];
    if (s == kNone) {  // absent: the first slot of the walk that is not LIVE. The capacity test left one.
        s = mix32(ip) & (P.cap - 1);
        uint32_t k = 0;
        for (; k < P.cap; k++, s = (s + 1) & (P.cap - 1)) {
            uint32_t st = P.slots[s].state;
            if (st == DK_ARP_SLOT_LIVE || st == kBusy) continue;
            if (__hip_atomic_compare_exchange_strong(&P.slots[s].state, &st, kBusy, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                if (st == DK_ARP_SLOT_FREE)
                    __hip_atomic_fetch_add(P.consumed, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
        if (k == P.cap) return;
    }
    dk_arp_slot& S = P.slots[s];
    S.ip = ip, S.reserved = 0;
    put_mac(S.mac, m);
    S.expiration_ns = P.clock + P.cfg.cache_ttl_ns;
    S.state = DK_ARP_SLOT_LIVE;
}

__global__ __launch_bounds__(kBlock) void arp_wake_kernel(Params P) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= P.nrows || p >= P.tot[kReady] || !fits(P)) return;
    const uint32_t r = P.svals[p], f = P.skeys[p];
    dk_arp_query& R = P.rows[r];
    const Mac m = frame_sha(P, f);
    resolve_row(P, R, m);
    write_ready(P, p, r, R, f, m, 0);
}

// The three words, and the status: one word (process, timers), or NO_ROOM for the start[] entries that passed.
__global__ __launch_bounds__(kBlock) void arp_finish_kernel(Params P, uint32_t mode) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    const bool ok = fits(P);
    if (j == 0) {
        *P.res.n_frames = (uint32_t)P.tot[kFrames];
        *P.res.n_ready = (uint32_t)P.tot[kReady];
        *P.res.n_entries = (uint32_t)entries(P);
        if (mode != kStart && P.res.status)
            P.res.status[0] = ok ? DK_ARP_OK : P.tot[kFrames] && !slot_room(P) ? DK_ARP_E_SLOT : DK_ARP_NO_ROOM;
    }
    if (mode == kStart && j < P.nstart && !ok && P.res.status[j] == DK_ARP_OK) P.res.status[j] = DK_ARP_NO_ROOM;
}

// ---- dk_arp_query_start ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void arp_claim_kernel(Params P) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= P.nstart) return;
    const uint32_t r = P.start[k];
    if (r < P.nrows) min32(P.term + r, k);  // the first entry that names the row
}

__global__ __launch_bounds__(kBlock) void arp_admit_kernel(Params P) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= P.nstart) return;
    const uint32_t r = P.start[k];
    uint32_t st = DK_ARP_E_ROW, ts = kNone;
    bool hit = false;
    if (r < P.nrows) {
        const dk_arp_query& R = P.rows[r];
        if (R.state != DK_ARP_Q_IDLE || P.term[r] != k) st = DK_ARP_E_STATE;
        else if (R.link != DK_ARP_NO_LINK && R.link >= P.nlinks) st = DK_ARP_E_LINK;
        else if (!slot_room(P)) st = DK_ARP_E_SLOT;
        else {
            st = DK_ARP_OK;
            if (disabled(P)) hit = true;
            else ts = find_slot(P.slots, P.cap, R.ip), hit = ts != kNone;
        }
    }
    P.res.status[k] = st;
    P.ts[k] = ts;
    P.act[k] = (uint8_t)hit;
    P.flag_r[k] = st == DK_ARP_OK && !hit;
    P.flag_y[k] = st == DK_ARP_OK && hit;
}

__global__ __launch_bounds__(kBlock) void arp_open_kernel(Params P) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= P.nstart || !fits(P) || P.res.status[k] != DK_ARP_OK) return;
    const uint32_t r = P.start[k];
    dk_arp_query& R = P.rows[r];
    if (P.act[k]) {
        const Mac m = slot_mac(P, P.ts[k]);
        resolve_row(P, R, m);
        write_ready(P, P.flag_y[k], r, R, kNone, m, 0);
    } else {
        emit_frame(P, P.flag_r[k], k, 1u, Mac{}, R.ip);
        R.state = DK_ARP_Q_WAITING, R.err = 0, R.sent = 1;
        R.deadline_ns = P.now + P.cfg.request_timeout_ns;
    }
}

// ---- dk_arp_timers --------------------------------------------------------------------------------------------------
enum Due : uint32_t { kIdle = 0, kResendMiss = 1, kResendHit = 2, kFail = 3 };

__global__ __launch_bounds__(kBlock) void arp_sweep_kernel(Params P) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= P.nrows) return;
    const dk_arp_query& R = P.rows[r];
    uint32_t due = kIdle, ts = kNone;
    if (R.state == DK_ARP_Q_WAITING && R.deadline_ns <= P.now) {
        if ((uint32_t)R.sent < P.cfg.retry_count + 1u) {
            bool hit = true;
            if (!disabled(P)) ts = find_slot(P.slots, P.cap, R.ip), hit = ts != kNone;
            due = hit ? kResendHit : kResendMiss;
        } else {
            due = kFail;
        }
    }
    P.act[r] = (uint8_t)due;
    P.ts[r] = ts;
    P.flag_r[r] = due == kResendMiss || due == kResendHit;
    P.flag_y[r] = due == kResendHit || due == kFail;
}

__global__ __launch_bounds__(kBlock) void arp_expire_kernel(Params P) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= P.nrows || !fits(P)) return;
    const uint32_t due = P.act[r];
    if (due == kIdle) return;
    dk_arp_query& R = P.rows[r];
    if (due == kFail) {
        R.state = DK_ARP_Q_FAILED, R.err = ETIMEDOUT;
        write_ready(P, P.flag_y[r], r, R, kNone, Mac{}, ETIMEDOUT);
        return;
    }
    emit_frame(P, P.flag_r[r], r, 1u, Mac{}, R.ip);
    R.sent = (uint16_t)(R.sent + 1);
    if (due == kResendHit) {
        const Mac m = slot_mac(P, P.ts[r]);
        resolve_row(P, R, m);
        write_ready(P, P.flag_y[r], r, R, kNone, m, 0);
    } else {
        R.deadline_ns = P.now + P.cfg.request_timeout_ns;
    }
}

// ---- dk_arp_lookup --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void arp_lookup_kernel(Params P, const uint32_t* ips, const uint32_t* link,
                                                            uint8_t* macs_out, uint32_t* found) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P.n) return;
    uint32_t ts = kNone;
    bool hit = true;
    if (!disabled(P)) ts = find_slot(P.slots, P.cap, ips[i]), hit = ts != kNone;
    const Mac m = slot_mac(P, ts);
    put_mac(macs_out + 6ull * i, m);
    found[i] = hit;
    if (hit && link && link[i] < P.nlinks) put_mac(P.links[link[i]].dst_mac, m);
}

// ---- the host side --------------------------------------------------------------------------------------------------
// What dk_arp_process, dk_arp_query_start and dk_arp_timers check before any GPU work.
bool bad_common(const dk_arp_table* t, const void* rows, uint32_t nrows, const dk_tx_link* links, uint32_t nlinks,
                uint64_t out_bytes, const dk_tcp_tx_layout* layout, const dk_arp_results* res) {
    if (!t || !layout || !res || !res->n_frames || !res->n_ready || !res->n_entries || !res->status) return true;
    if (nlinks && !links) return true;
    if (out_bytes > DK_RX_MAX_BLOB || nrows > 0x7FFFFFFFu) return true;
    if (nrows && !rows) return true;
    return (reinterpret_cast<uintptr_t>(rows) & 15) != 0;
}
bool bad_outputs(const uint8_t* out, uint32_t max_frames, uint32_t max_ready, const dk_arp_results* res) {
    return (max_frames && (!out || !res->off_out || !res->len_out)) || (max_ready && !res->ready);
}

void fill_common(Params& P, dk_arp_table* t, dk_arp_query* rows, uint32_t nrows, dk_tx_link* links, uint32_t nlinks,
                 uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames,
                 uint32_t max_ready, const dk_arp_results* res) {
    P.slots = t->slots, P.cap = t->cap, P.consumed = t->consumed, P.cfg = t->cfg;
    P.rows = rows, P.nrows = nrows, P.links = links, P.nlinks = nlinks;
    P.out = out, P.out_bytes = out_bytes, P.stride = layout->slot_stride, P.lead = layout->frame_lead;
    P.max_frames = max_frames, P.max_ready = max_ready, P.res = *res;
}

// The host's insert: cleanup(), then the entry with clock + ttl. False if no slot is left for it.
bool host_insert(std::vector<dk_arp_slot>& S, uint32_t ip, const uint8_t* mac, uint64_t clock, uint64_t ttl) {
    const uint32_t cap = (uint32_t)S.size();
    for (auto& e : S)
        if (e.state == DK_ARP_SLOT_LIVE && e.expiration_ns <= clock) {
            std::memset(&e, 0, sizeof(e));
            e.state = DK_ARP_SLOT_TOMBSTONE;
        }
    uint32_t s = find_slot(S.data(), cap, ip);
    if (s == kNone) {
        s = mix32(ip) & (cap - 1);
        uint32_t k = 0;
        for (; k < cap && S[s].state == DK_ARP_SLOT_LIVE; k++) s = (s + 1) & (cap - 1);
        if (k == cap) return false;
    }
    std::memset(&S[s], 0, sizeof(dk_arp_slot));
    S[s].ip = ip, S[s].state = DK_ARP_SLOT_LIVE, S[s].expiration_ns = clock + ttl;
    std::memcpy(S[s].mac, mac, 6);
    return true;
}

}  // namespace
}  // namespace dk_arp

extern "C" {

uint32_t dk_arp_home(uint32_t cap, uint32_t ip) { return cap ? dk_arp::mix32(ip) & (cap - 1) : 0u; }

int dk_arp_fits(uint32_t cap, uint64_t entries) { return entries <= (uint64_t)cap / 2 ? 0 : EINVAL; }

int dk_arp_table_create(int32_t device, uint32_t cap, const dk_arp_cfg* cfg, dk_arp_table** out) {
    using namespace dk_arp;
    if (!out || !cfg || cap < 2 || (cap & (cap - 1))) return EINVAL;
    if (!(cfg->flags & DK_ARP_DISABLED) && cfg->cache_ttl_ns == 0) return EINVAL;
    if ((cfg->flags & ~DK_ARP_DISABLED) || cfg->retry_count > DK_ARP_MAX_RETRIES) return EINVAL;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return EINVAL;
    DeviceGuard g(device);
    dk_arp_table* t = new dk_arp_table();
    t->device = device, t->cap = cap, t->cfg = *cfg;
    if (hipMalloc(&t->slots, (size_t)cap * sizeof(dk_arp_slot)) != hipSuccess ||
        hipMalloc(&t->consumed, sizeof(uint64_t)) != hipSuccess ||
        hipEventCreateWithFlags(&t->call.last, hipEventDisableTiming) != hipSuccess ||
        hipMemset(t->slots, 0, (size_t)cap * sizeof(dk_arp_slot)) != hipSuccess ||
        hipMemset(t->consumed, 0, sizeof(uint64_t)) != hipSuccess) {
        dk_arp_table_destroy(t);
        return ENOMEM;
    }
    *out = t;
    return 0;
}

void dk_arp_table_destroy(dk_arp_table* t) {
    if (!t) return;
    dk::ctl::DeviceGuard g(t->device);
    (void)t->call.drain();
    if (t->slots) (void)hipFree(t->slots);
    if (t->consumed) (void)hipFree(t->consumed);
    t->call.scratch.free();
    if (t->call.last) (void)hipEventDestroy(t->call.last);
    delete t;
}

int dk_arp_table_stats(dk_arp_table* t, uint32_t* cap, uint64_t* consumed) {
    if (!t) return EINVAL;
    dk::ctl::DeviceGuard g(t->device);
    if (cap) *cap = t->cap;
    if (consumed) {
        if (t->call.drain()) return EIO;
        if (hipMemcpy(consumed, t->consumed, sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return EIO;
    }
    return 0;
}

int dk_arp_table_read(dk_arp_table* t, dk_arp_slot* rows) {
    if (!t || !rows) return EINVAL;
    dk::ctl::DeviceGuard g(t->device);
    if (t->call.drain()) return EIO;
    return hipMemcpy(rows, t->slots, (size_t)t->cap * sizeof(dk_arp_slot), hipMemcpyDeviceToHost) == hipSuccess ? 0 : EIO;
}

int dk_arp_table_write(dk_arp_table* t, const dk_arp_slot* rows) {
    if (!t || !rows) return EINVAL;
    dk::ctl::DeviceGuard g(t->device);
    if (t->call.drain()) return EIO;
    uint64_t consumed = 0;
    for (uint32_t s = 0; s < t->cap; s++) {
        if (rows[s].state > DK_ARP_SLOT_TOMBSTONE) return EINVAL;
        consumed += rows[s].state != DK_ARP_SLOT_FREE;
    }
    if (hipMemcpy(t->slots, rows, (size_t)t->cap * sizeof(dk_arp_slot), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t->consumed, &consumed, sizeof(consumed), hipMemcpyHostToDevice) != hipSuccess)
        return EIO;
    return 0;
}

int dk_arp_table_insert(dk_arp_table* t, const uint32_t* ips, const uint8_t* macs, uint32_t n, uint64_t clock_ns) {
    using namespace dk_arp;
    if (!t || (n && (!ips || !macs))) return EINVAL;
    if (n == 0 || (t->cfg.flags & DK_ARP_DISABLED)) return 0;
    std::vector<dk_arp_slot> S(t->cap);
    if (int rc = dk_arp_table_read(t, S.data())) return rc;
    for (uint32_t i = 0; i < n; i++) {
        if (!host_insert(S, ips[i], macs + 6ull * i, clock_ns, t->cfg.cache_ttl_ns)) return ENOMEM;
        uint64_t live = 0;
        for (const auto& e : S) live += e.state == DK_ARP_SLOT_LIVE;
        if (dk_arp_fits(t->cap, live)) return ENOMEM;
    }
    return dk_arp_table_write(t, S.data());
}

int dk_arp_process(dk_arp_table* t, const dk_rx_batch* batch, const dk_rx_results* rx, uint32_t n, dk_arp_query* rows,
                   uint32_t nrows, dk_tx_link* links, uint32_t nlinks, uint64_t clock_ns, uint8_t* out,
                   uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready,
                   const dk_arp_results* res, void* stream) {
    using namespace dk_arp;
    if (!batch || !rx || bad_common(t, rows, nrows, links, nlinks, out_bytes, layout, res) || n > 0x7FFFFFFFu)
        return EINVAL;
    if (n && (!batch->frames || !batch->off || !rx->meta || !rx->src_ip || !rx->dst_ip || !res->action ||
              !res->reply_frame || batch->frames_bytes > DK_RX_MAX_BLOB))
        return EINVAL;
    if ((n || nrows) && bad_outputs(out, max_frames, max_ready, res)) return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    uint32_t hcap = 2;
    while (hcap < 2ull * n) hcap *= 2;
    const rocprim::counting_iterator<uint32_t> index(0);
    size_t sort_bytes = 0;
    if (nrows && rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, index,
                                           (uint32_t*)nullptr, nrows, 0, 32, s) != hipSuccess)
        return EIO;
    const uint32_t sb = dk_tcp_tx_scan_tiles(n);
    const size_t ff_bytes = 3 * round16((size_t)hcap * 4) + 16;
    const size_t zero_bytes = round16((size_t)hcap * 8) + round16((size_t)hcap * 4) + round16(t->cap) + round16(kTots * 8);
    const size_t need = ff_bytes + zero_bytes + round16((size_t)hcap * 4) + round16(hcap) + round16((size_t)n * 4) +
                        round16(n) + round16((size_t)n * 8) + round16((size_t)sb * 8) + 3 * round16((size_t)nrows * 4) +
                        round16(sort_bytes) + 16;
    if (int rc = t->call.grow(need)) return rc;
    if (int rc = t->call.order(s)) return rc;
    Params P{};
    fill_common(P, t, rows, nrows, links, nlinks, out, out_bytes, layout, max_frames, max_ready, res);
    P.frames = batch->frames, P.frames_bytes = batch->frames_bytes, P.off = batch->off;
    P.meta = rx->meta, P.src = rx->src_ip, P.dst = rx->dst_ip, P.n = n, P.clock = clock_ns, P.hcap = hcap;
    Carver c{t->call.scratch.p};
    P.hL = c.take<uint32_t>(hcap);
    P.hfirst = c.take<uint32_t>(hcap);
    P.hts = c.take<uint32_t>(hcap);
    P.f0 = c.take<uint32_t>(1);
    uint8_t* zz = c.b;
    P.hkey = c.take<uint64_t>(hcap);
    P.hlast = c.take<uint32_t>(hcap);
    P.keep = c.take<uint8_t>(t->cap);
    P.tot = c.take<uint64_t>(kTots);
    P.hfl = c.take<uint8_t>(hcap);
    P.sslot = c.take<uint32_t>(n);
    P.act = c.take<uint8_t>(n);
    P.flag_r = c.take<uint64_t>(n);
    uint64_t* bsum = c.take<uint64_t>(sb);
    P.keys = c.take<uint32_t>(nrows);
    P.skeys = c.take<uint32_t>(nrows);
    P.svals = c.take<uint32_t>(nrows);
    void* temp = c.take<uint8_t>(sort_bytes);
    if (hipMemsetAsync(P.hL, 0xFF, ff_bytes, s) != hipSuccess || hipMemsetAsync(zz, 0, zero_bytes, s) != hipSuccess)
        return EIO;
    if (n) {
        hipLaunchKernelGGL(arp_classify_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(arp_mark_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(arp_decide_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, n, bsum, P.tot + kFrames, s)) return EIO;
        hipLaunchKernelGGL(arp_senders_kernel, grid_for(hcap), dim3(kBlock), 0, s, P);
    }
    hipLaunchKernelGGL(arp_census_kernel, grid_for(t->cap), dim3(kBlock), 0, s, P, 1u);
    if (nrows) {
        hipLaunchKernelGGL(arp_rows_kernel, grid_for(nrows), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        size_t b = sort_bytes;
        if (rocprim::radix_sort_pairs(temp, b, P.keys, P.skeys, index, P.svals, nrows, 0, 32, s) != hipSuccess) return EIO;
    }
    if (n) {
        hipLaunchKernelGGL(arp_build_kernel, grid_for(n), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(arp_tomb_kernel, grid_for(t->cap), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(arp_store_kernel, grid_for(hcap), dim3(kBlock), 0, s, P);
        if (nrows) hipLaunchKernelGGL(arp_wake_kernel, grid_for(nrows), dim3(kBlock), 0, s, P);
    }
    hipLaunchKernelGGL(arp_finish_kernel, dim3(1), dim3(kBlock), 0, s, P, (uint32_t)kProcess);
    return t->call.record(s);
}

int dk_arp_query_start(dk_arp_table* t, dk_arp_query* rows, uint32_t nrows, const uint32_t* start, uint32_t nstart,
                       dk_tx_link* links, uint32_t nlinks, uint64_t now_ns, uint8_t* out, uint64_t out_bytes,
                       const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready,
                       const dk_arp_results* res, void* stream) {
    using namespace dk_arp;
    if (bad_common(t, rows, nrows, links, nlinks, out_bytes, layout, res) || nstart > 0x7FFFFFFFu) return EINVAL;
    if (nstart && (!start || bad_outputs(out, max_frames, max_ready, res))) return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t sb = dk_tcp_tx_scan_tiles(nstart);
    const size_t ff_bytes = round16((size_t)nrows * 4) + 16, zero_bytes = round16(kTots * 8);
    const size_t need = ff_bytes + zero_bytes + round16(t->cap) + round16((size_t)nstart * 4) + round16(nstart) +
                        2 * round16((size_t)nstart * 8) + round16((size_t)sb * 8) + 16;
    if (int rc = t->call.grow(need)) return rc;
    if (int rc = t->call.order(s)) return rc;
    Params P{};
    fill_common(P, t, rows, nrows, links, nlinks, out, out_bytes, layout, max_frames, max_ready, res);
    P.start = start, P.nstart = nstart, P.now = now_ns;
    Carver c{t->call.scratch.p};
    P.term = c.take<uint32_t>(nrows);
    P.f0 = c.take<uint32_t>(1);
    P.tot = c.take<uint64_t>(kTots);
    P.keep = c.take<uint8_t>(t->cap);  // not read: the census counts LIVE slots only
    P.ts = c.take<uint32_t>(nstart);
    P.act = c.take<uint8_t>(nstart);
    P.flag_r = c.take<uint64_t>(nstart);
    P.flag_y = c.take<uint64_t>(nstart);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if (hipMemsetAsync(P.term, 0xFF, ff_bytes, s) != hipSuccess || hipMemsetAsync(P.tot, 0, zero_bytes, s) != hipSuccess)
        return EIO;
    hipLaunchKernelGGL(arp_census_kernel, grid_for(t->cap), dim3(kBlock), 0, s, P, 0u);
    if (nstart) {
        hipLaunchKernelGGL(arp_claim_kernel, grid_for(nstart), dim3(kBlock), 0, s, P);
        hipLaunchKernelGGL(arp_admit_kernel, grid_for(nstart), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, nstart, bsum, P.tot + kFrames, s) ||
            dk_tcp_tx_scan(P.flag_y, nstart, bsum, P.tot + kReady, s))
            return EIO;
        hipLaunchKernelGGL(arp_open_kernel, grid_for(nstart), dim3(kBlock), 0, s, P);
    }
    hipLaunchKernelGGL(arp_finish_kernel, grid_for(nstart), dim3(kBlock), 0, s, P, (uint32_t)kStart);
    return t->call.record(s);
}

int dk_arp_timers(dk_arp_table* t, dk_arp_query* rows, uint32_t nrows, dk_tx_link* links, uint32_t nlinks,
                  uint64_t now_ns, uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout,
                  uint32_t max_frames, uint32_t max_ready, const dk_arp_results* res, void* stream) {
    using namespace dk_arp;
    if (bad_common(t, rows, nrows, links, nlinks, out_bytes, layout, res)) return EINVAL;
    if (nrows && bad_outputs(out, max_frames, max_ready, res)) return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t sb = dk_tcp_tx_scan_tiles(nrows);
    const size_t zero_bytes = round16(kTots * 8);
    const size_t need = 16 + zero_bytes + round16(t->cap) + round16((size_t)nrows * 4) + round16(nrows) +
                        2 * round16((size_t)nrows * 8) + round16((size_t)sb * 8) + 16;
    if (int rc = t->call.grow(need)) return rc;
    if (int rc = t->call.order(s)) return rc;
    Params P{};
    fill_common(P, t, rows, nrows, links, nlinks, out, out_bytes, layout, max_frames, max_ready, res);
    P.now = now_ns;
    Carver c{t->call.scratch.p};
    P.f0 = c.take<uint32_t>(1);
    P.tot = c.take<uint64_t>(kTots);
    P.keep = c.take<uint8_t>(t->cap);
    P.ts = c.take<uint32_t>(nrows);
    P.act = c.take<uint8_t>(nrows);
    P.flag_r = c.take<uint64_t>(nrows);
    P.flag_y = c.take<uint64_t>(nrows);
    uint64_t* bsum = c.take<uint64_t>(sb);
    if (hipMemsetAsync(P.tot, 0, zero_bytes, s) != hipSuccess) return EIO;
    hipLaunchKernelGGL(arp_census_kernel, grid_for(t->cap), dim3(kBlock), 0, s, P, 0u);
    if (nrows) {
        hipLaunchKernelGGL(arp_sweep_kernel, grid_for(nrows), dim3(kBlock), 0, s, P);
        if (hipGetLastError() != hipSuccess) return EIO;
        if (dk_tcp_tx_scan(P.flag_r, nrows, bsum, P.tot + kFrames, s) ||
            dk_tcp_tx_scan(P.flag_y, nrows, bsum, P.tot + kReady, s))
            return EIO;
        hipLaunchKernelGGL(arp_expire_kernel, grid_for(nrows), dim3(kBlock), 0, s, P);
    }
    hipLaunchKernelGGL(arp_finish_kernel, dim3(1), dim3(kBlock), 0, s, P, (uint32_t)kTimers);
    return t->call.record(s);
}

int dk_arp_lookup(dk_arp_table* t, const uint32_t* ips, const uint32_t* link, uint32_t n, dk_tx_link* links,
                  uint32_t nlinks, uint8_t* macs_out, uint32_t* found, void* stream) {
    using namespace dk_arp;
    if (!t || n > 0x7FFFFFFFu || (nlinks && !links)) return EINVAL;
    if (n && (!ips || !macs_out || !found)) return EINVAL;
    DeviceGuard g(t->device);
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = t->call.order(s)) return rc;
    Params P{};
    P.slots = t->slots, P.cap = t->cap, P.cfg = t->cfg, P.links = links, P.nlinks = nlinks, P.n = n;
    if (n) hipLaunchKernelGGL(arp_lookup_kernel, grid_for(n), dim3(kBlock), 0, s, P, ips, link, macs_out, found);
    return t->call.record(s);
}

}  // extern "C"
