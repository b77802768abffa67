/*
 * dk_arp.h — the ARP peer on the GPU: its cache, its replies and its queries.
 *
 * What SharedArpPeer does (layer3/arp/peer.rs) with ArpCache / HashTtlCache behind it (layer3/arp/cache/mod.rs,
 * collections/hashttlcache.rs): poll() over the ARP frames of one dk_rx_process batch (dk_arp_process), query() up to
 * its first await (dk_arp_query_start), the request timeout and its retries (dk_arp_timers) and try_query()
 * (dk_arp_lookup). The cache is a table in device memory that the device inserts into; replies and requests are built
 * on the device; a pending query() is a row in device memory that a received frame resolves; a resolved row writes the
 * MAC into links[] (dk_tx_link, dk_rx.h), so the send-side calls take that array unread by the host.
 * Additive: DK_RX_ABI_VERSION stays 4.
 *
 * ---- the cache ----------------------------------------------------------------------------------------------------
 * dk_arp_table is an open-addressing table of `cap` slots (a power of two, at least 2) on one device; a slot is
 * {ip, mac, expiration_ns, state FREE / LIVE / TOMBSTONE}. A key's walk starts at dk_arp_home(cap, ip), steps by one
 * and wraps; a lookup walks across tombstones and ends at a FREE slot (or after cap steps); an insert of an absent key
 * claims the first slot of its walk that is not LIVE, a tombstone included. The slot a key lands in is unspecified.
 * At most cap / 2 slots are LIVE (dk_arp_fits). Removing an entry leaves a tombstone; rebuilding a worn table is out
 * of scope, as is eviction (the reference has none).
 *
 * The cache clock. HashTtlCache::clock advances only under cfg(test) in the reference, so in production nothing ever
 * expires. That stays visible here: every call that inserts takes clock_ns, the value of HashTtlCache::clock, as its
 * own argument, and no call takes now_ns for it. A caller that wants the production behaviour passes the creation time
 * forever; a caller that wants entries to age passes its clock. clock_ns must not go backwards: that is the caller's
 * contract and is not checked on the device. now_ns is used for query deadlines only.
 *   get(ip)     the entry's MAC if the table holds one, expired or not (HashTtlCache::get does not test expiry).
 *   insert      cleanup() removes every entry of the whole table with expiration_ns <= clock_ns, then the entry is
 *               stored with expiration_ns = clock_ns + cache_ttl_ns.
 * With DK_ARP_DISABLED in cfg.flags, ArpCache(None) applies: every get answers 00:00:00:00:00:00, nothing is stored,
 * and replies still go out. With ARP enabled, cache_ttl_ns == 0 is EINVAL (the reference asserts).
 *
 * ---- queries ------------------------------------------------------------------------------------------------------
 * dk_arp_query is one row per pending query(), 32 bytes, in 16-byte aligned device memory, updated in place. Rows are
 * independent of each other: the reference's do_drop(ip), which on one query's failure also removes the waiters of
 * other queries for the same address, is not reproduced. Rows that share a `link` must name the same `ip`: that is
 * the caller's contract.
 *
 * ---- dk_arp_process -----------------------------------------------------------------------------------------------
 * SharedArpPeer::poll over one dk_rx_process batch: the dk_rx_batch (for the hardware-address bytes) and its
 * dk_rx_results, of which meta, src_ip and dst_ip are required. Covered are the frames with verdict DK_V_ARP, in batch
 * order; every other frame gets action 0 (DK_ARP_SKIP), DK_V_ARP_SHORT and DK_V_ARP_UNSUP included (the reference
 * drops them with a warning). For a covered frame sha = frame bytes [22, 28), spa = src_ip, tpa = dst_ip,
 * op = meta >> 16. Per frame:
 *   1. hit = get(spa) answers (an expired entry that is still in the table counts).          DK_ARP_HIT
 *   2. if hit: do_insert(spa, sha).                                                           DK_ARP_INSERTED
 *   3. if tpa != local_ip the frame is done: HIT | INSERTED, or                               DK_ARP_DROPPED
 *   4. if not hit: do_insert(spa, sha).                                          DK_ARP_LEARNED | DK_ARP_INSERTED
 *   5. a Request: a reply frame goes out (DK_ARP_REPLY, reply_frame = its index); a Reply: cache.insert(spa, sha) once
 *      more, which at a fixed clock changes nothing.
 * do_insert first wakes every WAITING row whose ip is spa: the row becomes RESOLVED, mac = sha, links[link].dst_mac =
 * sha if the row has a link (src_mac and reserved are not touched), and a ready record is appended. Then it inserts.
 * A row keeps the MAC of the first insert that woke it even if a later frame of the batch changes the cache entry:
 * that is what the oneshot channel delivers.
 *
 * The outcome is a function of the following, which is what lets the call run in parallel. The clock is fixed for the
 * call. Let f0 be the first covered frame whose spa has any entry (expired or not) or whose tpa is local.
 *   - If f0 does not exist, nothing changes and nothing is cleaned up; every covered frame is DROPPED.
 *   - Frames before f0 are DROPPED.
 *   - At f0 every expired entry leaves the table, keys absent from the batch included.
 *   - After f0, a key counts as present only if it has a live entry or an earlier frame at or after f0 inserted it.
 *     The one exception is f0's own hit test, which still sees an expired entry.
 *   - So with base(s) = s has a live entry, or s is f0's sender and has any entry, and L(s) = the first frame at or
 *     after f0 of sender s whose tpa is local: a frame i >= f0 of sender s hits iff base(s) or i > L(s); the first
 *     insert of s is its first frame at or after f0 if base(s), else L(s); the entry ends with the sha of the last
 *     frame of s if s inserts at all.
 *   - Frames of different senders are independent. Frames of one sender are ordered.
 * Under DK_ARP_DISABLED every covered frame hits, f0 is the first covered frame and the table is not touched.
 * One lane works per frame, per sender, per table slot and per row; no lane walks the batch.
 *
 * ---- frames -------------------------------------------------------------------------------------------------------
 * 42 bytes, no padding: 14 bytes of Ethernet with ethertype 0x0806, then the 28 bytes ArpHeader::create_and_serialize
 * writes (htype 1, ptype 0x0800, hlen 6, plen 4, op, sha, spa, tha, tpa).
 *   reply:    Ethernet dst = the request's sha, src = local_mac; op 2, sha = local_mac, spa = local_ip, tha = the
 *             request's sha, tpa = the request's spa.
 *   request:  Ethernet dst = ff:ff:ff:ff:ff:ff, src = local_mac; op 1, sha = local_mac, spa = local_ip, tha =
 *             ff:ff:ff:ff:ff:ff (the reference passes MacAddress::broadcast() there), tpa = the queried address.
 * Frame f of a call lies at out[f * slot_stride + frame_lead] (dk_tcp_tx_layout's slot rule), off_out[f] is that
 * offset, len_out[f] = 42 and frame_seg[f] (nullable) the item that caused it: the batch frame (process), the start[]
 * entry (start), the row (timers). Replies are numbered in the order of the frames that triggered them, requests in
 * start[] order and in ascending row order. No byte of out outside the frames is written.
 *
 * ---- dk_arp_query_start -------------------------------------------------------------------------------------------
 * query() up to its first await, for the rows named in start[0 .. nstart), in that order. The first check that applies
 * is reported in status[k] and the row is left untouched:
 *   E_ROW    start[k] >= nrows
 *   E_STATE  the row is not IDLE, or an earlier entry of start[] names the same row (the lowest k wins)
 *   E_LINK   link >= nlinks and link != DK_ARP_NO_LINK
 *   E_SLOT   frame_lead + 42 > slot_stride
 * For a row that passes: a cache hit (get: an expired but present entry counts, and the all-zero MAC counts under
 * DK_ARP_DISABLED) makes the row RESOLVED with its link written and a ready record, and sends no frame. Otherwise a
 * request goes out, sent = 1, the row becomes WAITING and deadline_ns = now_ns + request_timeout_ns.
 *
 * ---- dk_arp_timers ------------------------------------------------------------------------------------------------
 * The conditional_yield_with_timeout expiry, for every WAITING row with deadline_ns <= now_ns, in ascending row order.
 * If sent < retry_count + 1 the request goes out again and sent += 1; then the cache is looked at, as do_wait_link_addr
 * does after the transmit: a hit resolves the row although its frame still goes out, on a miss deadline_ns = now_ns +
 * request_timeout_ns. Otherwise the row becomes FAILED / ETIMEDOUT with an error ready record and no frame. A query
 * therefore sends retry_count + 1 requests in all and fails at the expiry after the last one. status[0] is the call's
 * one status word (as for dk_arp_process): OK, NO_ROOM, or E_SLOT when a frame is due and frame_lead + 42 >
 * slot_stride, which leaves everything unwritten as NO_ROOM does.
 *
 * ---- dk_arp_lookup ------------------------------------------------------------------------------------------------
 * try_query for ips[0 .. n): found[i] (1 or 0), macs_out[6 i .. 6 i + 6) (zero where not found) and
 * links[link[i]].dst_mac where link is given, link[i] < nlinks and the address is found. It inserts nothing. It is
 * what a passive side needs before it answers a SYN.
 *
 * ---- ready records ------------------------------------------------------------------------------------------------
 * dk_arp_process emits them in the order of the waking frames and by ascending row within one frame; start in start[]
 * order; timers in ascending row order. The host reads n_ready and the records and builds start[] for
 * dk_tcp_connect_start from the tags; links[] needs no host touch.
 *
 * ---- capacity -----------------------------------------------------------------------------------------------------
 * All or nothing, tested on the device. n_frames, n_ready and n_entries (the table's LIVE count after the call) always
 * report the call's need. The call fails for room if n_frames > max_frames, or n_frames * slot_stride > out_bytes, or
 * n_ready > max_ready, or n_entries > cap / 2. Then nothing else is written: no frame, record, per-frame result, table
 * slot, row field or link; status reports NO_ROOM (status[0] for process and timers; every start[] entry that passed
 * its checks for start). There is no host round trip in any call.
 *
 * ---- calling conventions ------------------------------------------------------------------------------------------
 * Return values are 0, EINVAL, ENOMEM or EIO. EINVAL covers a null required pointer, misaligned rows, n >= 2^31 and
 * out_bytes > DK_RX_MAX_BLOB, all found before any GPU work. n == 0 and nrows == 0 are valid calls. links may be null
 * only with nlinks == 0. Calls on one table are serialised as a context's calls are; they are asynchronous on the
 * caller's stream, except create, destroy, stats, read, write and insert, which are synchronous. The environment is
 * never read.
 *
 * Out of scope: the ICMPv4 peer (echo replies and ping: its reply path begins with arp.query); eviction;
 * dk_arp_query_start driven by a device-side count; the reference's do_drop interplay between concurrent queries for
 * one address.
 */
#ifndef DK_ARP_H
#define DK_ARP_H

#include <stdint.h>

#include "dk_rx.h"
#include "dk_tcp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DK_ARP_NONE 0xFFFFFFFFu    /* reply_frame: no reply; ready.frame: not caused by a batch frame */
#define DK_ARP_NO_LINK 0xFFFFFFFFu /* dk_arp_query.link: the row writes no link */
#define DK_ARP_FRAME_BYTES 42u
#define DK_ARP_DISABLED 1u         /* dk_arp_cfg.flags */
#define DK_ARP_MAX_RETRIES 65534u  /* retry_count above it: EINVAL (sent is 16 bits) */

/* dk_arp_results.action: a set of bits, 0 for a frame that is not covered */
#define DK_ARP_SKIP 0u
#define DK_ARP_HIT 1u
#define DK_ARP_INSERTED 2u
#define DK_ARP_REPLY 4u
#define DK_ARP_LEARNED 8u
#define DK_ARP_DROPPED 16u

enum dk_arp_slot_state {
    DK_ARP_SLOT_FREE = 0,
    DK_ARP_SLOT_LIVE = 1,
    DK_ARP_SLOT_TOMBSTONE = 2,
};

enum dk_arp_query_state {
    DK_ARP_Q_IDLE = 0,
    DK_ARP_Q_WAITING = 1,
    DK_ARP_Q_RESOLVED = 2,
    DK_ARP_Q_FAILED = 3,
};

enum dk_arp_status {
    DK_ARP_OK = 0,
    DK_ARP_E_ROW = 1,
    DK_ARP_E_STATE = 2,
    DK_ARP_E_LINK = 3,
    DK_ARP_E_SLOT = 4,
    DK_ARP_NO_ROOM = 5,
};

typedef struct dk_arp_cfg {
    uint32_t local_ip; /* octet order as in dk_rx.h: the first octet is the low byte */
    uint8_t local_mac[6];
    uint16_t reserved0;
    uint32_t flags; /* DK_ARP_DISABLED */
    uint32_t retry_count;
    uint32_t reserved1;
    uint64_t cache_ttl_ns;
    uint64_t request_timeout_ns;
} dk_arp_cfg; /* 40 bytes */

typedef struct dk_arp_slot {
    uint32_t ip;
    uint32_t state; /* enum dk_arp_slot_state */
    uint8_t mac[6];
    uint16_t reserved;
    uint64_t expiration_ns;
} dk_arp_slot; /* 24 bytes */

typedef struct dk_arp_query {
    uint32_t ip;
    uint32_t link;  /* index into links[], or DK_ARP_NO_LINK */
    uint32_t tag;   /* the caller's word, for example a connector row */
    uint16_t state; /* enum dk_arp_query_state */
    uint16_t err;   /* 0 or ETIMEDOUT */
    uint64_t deadline_ns;
    uint8_t mac[6];
    uint16_t sent; /* requests sent so far */
} dk_arp_query;    /* 32 bytes */

typedef struct dk_arp_ready {
    uint32_t row;
    uint32_t tag;
    uint32_t ip;
    uint32_t frame; /* the triggering batch frame, or DK_ARP_NONE from start and timers */
    uint8_t mac[6];
    uint16_t err; /* 0 or ETIMEDOUT */
} dk_arp_ready;   /* 24 bytes */

typedef struct dk_arp_results {
    uint8_t* action;       /* [n] process */
    uint32_t* reply_frame; /* [n] process */
    uint32_t* off_out;     /* [max_frames] */
    uint16_t* len_out;     /* [max_frames] */
    uint32_t* frame_seg;   /* [max_frames], nullable */
    dk_arp_ready* ready;   /* [max_ready] */
    uint32_t* status;      /* start: [nstart]; process, timers: one word */
    uint32_t* n_frames;
    uint32_t* n_ready;
    uint32_t* n_entries;
} dk_arp_results;

typedef struct dk_arp_table dk_arp_table;

/* Pure host functions: the slot a key's walk starts at, and whether `entries` LIVE entries fit (0 or EINVAL). */
uint32_t dk_arp_home(uint32_t cap, uint32_t ip);
int dk_arp_fits(uint32_t cap, uint64_t entries);

int dk_arp_table_create(int32_t device, uint32_t cap, const dk_arp_cfg* cfg, dk_arp_table** out);
void dk_arp_table_destroy(dk_arp_table* t);
/* cap, and the never-used slots consumed (slots that are not FREE). Synchronous. */
int dk_arp_table_stats(dk_arp_table* t, uint32_t* cap, uint64_t* consumed);
/* All slots to / from rows[0 .. cap) in host memory. Synchronous. */
int dk_arp_table_read(dk_arp_table* t, dk_arp_slot* rows);
int dk_arp_table_write(dk_arp_table* t, const dk_arp_slot* rows);
/* The constructor's initial_values loop from host arrays (macs: 6 bytes a pair): cache.insert per pair, a later
 * duplicate wins. Synchronous. ENOMEM, with the table unchanged, if more than cap / 2 entries would be LIVE. Under
 * DK_ARP_DISABLED nothing is stored. */
int dk_arp_table_insert(dk_arp_table* t, const uint32_t* ips, const uint8_t* macs, uint32_t n, uint64_t clock_ns);

int dk_arp_process(dk_arp_table* t, const dk_rx_batch* batch, const dk_rx_results* rx, uint32_t n, dk_arp_query* rows,
                   uint32_t nrows, dk_tx_link* links, uint32_t nlinks, uint64_t clock_ns, uint8_t* out,
                   uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready,
                   const dk_arp_results* res, void* stream);

int dk_arp_query_start(dk_arp_table* t, dk_arp_query* rows, uint32_t nrows, const uint32_t* start, uint32_t nstart,
                       dk_tx_link* links, uint32_t nlinks, uint64_t now_ns, uint8_t* out, uint64_t out_bytes,
                       const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready,
                       const dk_arp_results* res, void* stream);

int dk_arp_timers(dk_arp_table* t, dk_arp_query* rows, uint32_t nrows, dk_tx_link* links, uint32_t nlinks,
                  uint64_t now_ns, uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout,
                  uint32_t max_frames, uint32_t max_ready, const dk_arp_results* res, void* stream);

int dk_arp_lookup(dk_arp_table* t, const uint32_t* ips, const uint32_t* link, uint32_t n, dk_tx_link* links,
                  uint32_t nlinks, uint8_t* macs_out, uint32_t* found, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DK_ARP_H */
