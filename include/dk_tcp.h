/*
 * dk_tcp.h — established-state TCP receive processing on the GPU: the sequence-space checks
 * and per-connection in-order delivery that ControlBlock::poll runs on every segment TcpPeer::receive queued for an
 * established socket (tcp/socket.rs:308-314 -> tcp/established/ctrlblk.rs:345-440), for a whole dk_rx batch at once.
 *
 * Per segment, in arrival order within each connection (paths relative to /root/reference/src/rust/inetstack/
 * protocols/layer4/tcp/):
 *   check_segment_in_window   established/ctrlblk.rs:447-567  duplicate / out-of-window drops, front and end trims
 *   check_rst, check_syn      :570-604
 *   process_ack               :607-650   only the ack_num <= SND.NXT test (the send side is not modelled)
 *   process_data              :652-695   in order -> receive_data (:951-1001, also recovers stored segments),
 *                                        else the out-of-order store (:836-941, MAX_OUT_OF_ORDER_SIZE_FRAMES = 16)
 *   process_remote_close      :1003-1024 FIN: EOF buffer, RCV.NXT + 1, the connection stops processing
 * SeqNumber comparisons are sequence_number.rs:76-101 (sign of the wrapping difference). Reference quirks are kept:
 * the end-overlap adjust of the out-of-order store is one byte short (ctrlblk.rs:916), a front-overlapping segment is
 * inserted at the back of the store (ctrlblk.rs:891-899 leave action_index at the end), a FIN-only in-order segment
 * pushes an empty buffer before the EOF buffer (ctrlblk.rs:693 + :1008).
 * The sender's reaction to the ACKs those segments carry (SND.UNA, the send window, the unacknowledged queue, the RTT
 * estimate and the retransmit deadline) is dk_tcp_ack_process and cutting pushed buffers into segments is
 * dk_tcp_tx_segment, both below; resending the front of the unacknowledged queue (retransmit() and the timeout's
 * back-off) is dk_tcp_retransmit; the ACKs the segments trigger and the delayed-ACK timer are dk_tcp_ack_emit and
 * dk_tcp_ack_timer, at the end.
 * Congestion control (CUBIC's on_ack_received, on_rto, on_fast_retransmit and its two send hooks) and deciding which
 * timers have expired are dk_tcp_cc_ack, dk_tcp_timers and dk_tcp_cc_send, the last section: where the sections
 * between say that cwnd is an input or that the host fills fire[], those calls are what computes them on the device.
 * Creating a connection (the passive open: SYN, SYN+ACK, the handshake ACK and its timeout, the backlog) is the
 * dk_tcp_listen_* section; the active open (the ISN, the SYN and its retries, the tests on the answer, the handshake
 * ACK) is the dk_tcp_connect_* section at the end.
 * Ending a connection (ControlBlock::close: FIN-WAIT-1/2, CLOSING, TIME-WAIT and LAST-ACK over the segments that arrive
 * after poll() has returned) is the dk_tcp_close_* section, the last one.
 * Not modelled: the persist timer, repacketization.
 *
 * Conventions as dk_rx.h: 0 or a positive errno; device pointers; asynchronous on the caller's stream. A context holds
 * one set of scratch buffers: calls on one context are serialised — a call on another stream than the previous call
 * first waits (on the device) for the previous call's work — so use one context per stream for concurrent batches.
 * The engine picks its per-connection walk from the batch (one lane per connection; one wave per connection at
 * >= 8 segments per connection; at >= 1,024 segments per connection and <= 256 connections the scan walk: windows
 * precomputed across the chip, 64 windows per wave scan per connection, the rest in parallel); the diagnostic
 * dk_diag_tcp_set_walk (dk_diag.h) forces one (relay: 8 waves per connection passing its state window to window).
 * The environment is never read. Results are identical.
 */
#ifndef DK_TCP_H
#define DK_TCP_H

#include <stdint.h>

#include "dk_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DK_TCP_OOO_MAX 16u          /* MAX_OUT_OF_ORDER_SIZE_FRAMES (ctrlblk.rs:53)                              */
#define DK_TCP_DELIV_EXTRA 18u      /* delivery slots per connection beyond its segment count (stored + 2 EOF)   */
#define DK_TCP_REF_EOF 0xFFFFFFFFu  /* dk_tcp_view.ref of the empty EOF buffer process_remote_close pushes       */

enum dk_tcp_state {
    DK_TCP_NONE = 0,        /* not a connection: its frames are left alone (DK_TCP_SKIP)                          */
    DK_TCP_ESTABLISHED = 1,
    DK_TCP_CLOSED = 2       /* after RST or FIN: ControlBlock::poll has returned (ctrlblk.rs:381-396)             */
};

/* A DemiBuffer view: `len` bytes at byte `off` of frame `ref` (the frame's index in the dk_rx batch it came in, or
 * whatever the caller keeps in state carried between batches; DK_TCP_REF_EOF for the EOF buffer). */
typedef struct dk_tcp_view {
    uint32_t ref;
    uint32_t off;
    uint32_t len;
} dk_tcp_view;

/* Receive side of one connection's ControlBlock (ctrlblk.rs:145-220), indexed by the flow_id dk_rx gives its frames. */
typedef struct dk_tcp_conn {
    uint32_t state;         /* enum dk_tcp_state                                                                   */
    uint32_t receive_next;  /* RCV.NXT, Receiver::receive_next (ctrlblk.rs:98)                                     */
    uint32_t reader_next;   /* Receiver::reader_next (ctrlblk.rs:95); window = buffer_size - (RCV.NXT - reader_next) */
    uint32_t buffer_size;   /* receive_buffer_size_frames (ctrlblk.rs:191)                                         */
    uint32_t send_next;     /* SND.NXT, for process_ack's ack_num <= SND.NXT (ctrlblk.rs:623-633)                  */
    uint32_t fin_pending;   /* receive_out_of_order_fin is Some (ctrlblk.rs:220)                                   */
    uint32_t fin_seq;
    uint32_t ooo_count;     /* receive_out_of_order_frames (ctrlblk.rs:208), in store order; entries past the count
                               are zero                                                                            */
    uint32_t ooo_start[DK_TCP_OOO_MAX];
    dk_tcp_view ooo[DK_TCP_OOO_MAX];
} dk_tcp_conn;              /* 288 bytes */

enum dk_tcp_action {
    DK_TCP_SKIP = 0,           /* not a delivered TCP segment of a connection in the table                        */
    DK_TCP_DELIVERED = 1,      /* in order: pushed to the receive queue (with any stored segments it unblocked)   */
    DK_TCP_STORED = 2,         /* out of order: kept for later (data and/or FIN)                                  */
    DK_TCP_STORE_DUP = 3,      /* out of order, inside stored data: dropped (ctrlblk.rs:903-908)                  */
    DK_TCP_NO_DATA = 4,        /* acceptable, no data and no FIN                                                  */
    DK_TCP_FIN = 5,            /* FIN reached in order: EOF pushed, connection closes (ECONNRESET, :1003-1024)    */
    DK_TCP_DUPLICATE = 6,      /* entirely old (ctrlblk.rs:495-504)                              EBADMSG          */
    DK_TCP_OUT_OF_WINDOW = 7,  /* starts at or beyond the window end (ctrlblk.rs:525-535)        EBADMSG          */
    DK_TCP_RST = 8,            /* reset (ctrlblk.rs:570-583): connection closes                  ECONNRESET       */
    DK_TCP_SYN = 9,            /* in-window SYN (ctrlblk.rs:586-604)                             EBADMSG          */
    DK_TCP_NO_ACK = 10,        /* ACK bit clear (ctrlblk.rs:608-613)                             EBADMSG          */
    DK_TCP_ACK_UNSENT = 11,    /* acknowledges beyond SND.NXT (ctrlblk.rs:640-647)               EBADMSG          */
    DK_TCP_UNPROCESSED = 12    /* queued behind the close: never processed (ctrlblk.rs:355-363)                   */
};

/* Outputs of one call (device arrays). action, view: [n], per frame of the batch; view = the segment's data after
 * check_segment_in_window's adjust/trim (the payload as dk_rx gave it for frames that are dropped before or never
 * processed). deliv: the buffers pushed to each connection's receive queue, in order: connection c's are
 * deliv[deliv_start[c] .. deliv_start[c] + deliv_count[c]), where the engine sets deliv_start[c] = (segments of
 * connections < c) + DK_TCP_DELIV_EXTRA * c; deliv must hold n + DK_TCP_DELIV_EXTRA * nconns entries. */
typedef struct dk_tcp_out {
    uint8_t* action;
    dk_tcp_view* view;
    dk_tcp_view* deliv;
    uint32_t* deliv_start;  /* [nconns] */
    uint32_t* deliv_count;  /* [nconns] */
} dk_tcp_out;

typedef struct dk_tcp_ctx dk_tcp_ctx;

/* Scratch (sort buffers) for dk_tcp_rx_process on `device`. Returns 0 or EINVAL. */
int dk_tcp_ctx_create(int32_t device, dk_tcp_ctx** out);
void dk_tcp_ctx_destroy(dk_tcp_ctx* ctx);

/* Run the TCP segments of one dk_rx_process batch through their connections: rx = that call's device results (meta,
 * flow_id, payload, tcp_seq and tcp_ack are required), conns[0 .. nconns) = the connections by flow_id (device,
 * 16-byte aligned as hipMalloc returns it, updated in place). Asynchronous on `stream`. Returns 0, EINVAL (also for a
 * misaligned conns) or ENOMEM. */
int dk_tcp_rx_process(dk_tcp_ctx* ctx, const dk_rx_results* rx, uint32_t n, dk_tcp_conn* conns, uint32_t nconns,
                      const dk_tcp_out* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * TCP send segmentation: cut the buffers an application pushed into finished TCP frames, for a whole batch of
 * connections at once. Bit-exact to a loop of Sender::send_segment (tcp/established/sender.rs:124-208) over each
 * connection's buffers with no ACK arriving meanwhile, the headers from ControlBlock::tcp_header (ctrlblk.rs:699-709:
 * ACK set, ack_num = RCV.NXT, window = hdr_window_size() :786-803) and the Ethernet / IPv4 / TCP bytes exactly
 * what dk_tx_serialize writes for the same descriptor (no options: 54 header bytes). For every connection, its
 * buffers in push order:
 *   loop: sent = snd_nxt - snd_una (wrapping)
 *         open = (snd_wnd == 0 || snd_wnd < sent || cwnd < sent) ? 0 : min(snd_wnd - sent, mss, cwnd - sent)
 *         open == 0 -> the connection stops: the rest of this buffer and every later one stay unsent
 *         remaining > open -> frame of `open` bytes, flags ACK
 *         else             -> frame of `remaining` bytes, ACK|PSH (remaining > 0) or ACK|FIN (a zero-length buffer, the
 *                             end-of-send marker: consumes 1), buffer done
 *         seq = snd_nxt before the frame; snd_nxt += bytes (or 1)
 * A sent FIN sets fin_sent; buffers behind a marker, or on a connection whose fin_sent is set, are not sent. The
 * payload is copied from the source blob into frame slots (a pushed buffer has no headroom between its pieces) and
 * summed while it is copied: each payload byte is read once and written once.
 * Not modelled (they stay with the host): the timers' firing (retransmission itself is dk_tcp_retransmit, below), cwnd
 * updates (cwnd is an input, fixed for the call: CUBIC's decrement of its limited-transmit increase in on_send and its
 * idle restart in on_cwnd_check_before_send are not applied between the frames of a call), the persist timer. The
 * unacknowledged queue and the RTT estimate are dk_tcp_ack_process's (below).
 * These entry points are additive: DK_RX_ABI_VERSION stays 4.
 * ------------------------------------------------------------------------------------------------------------- */
/* Send side of one connection (Sender + what ControlBlock::tcp_header reads). Device memory, 16-byte aligned, updated
 * in place (snd_nxt, fin_sent). */
typedef struct dk_tcp_tx_conn {
    uint32_t state;       /* enum dk_tcp_state; only DK_TCP_ESTABLISHED sends                                     */
    uint32_t snd_una;     /* Sender::send_unacked                                                                  */
    uint32_t snd_nxt;     /* Sender::send_next                                                                     */
    uint32_t snd_wnd;     /* Sender::send_window                                                                   */
    uint32_t cwnd;        /* the effective congestion window (cwnd + limited-transmit increase), fixed for the
                             call; congestion control None: 0xFFFFFFFF                                             */
    uint32_t mss;         /* 0 never opens the window; above 65,481 (54 + mss must fit len_out) is a connection
                             error                                                                                 */
    uint32_t rcv_nxt;     /* ack number when no receive table is passed                                            */
    uint32_t rcv_wscale;  /* receive_window_scale_shift_bits (used with a receive table)                           */
    uint32_t local_ip;    /* addresses and ports in dk_tx_segs' packing: src = local, dst = remote                 */
    uint32_t remote_ip;
    uint32_t ports;       /* local_port | remote_port << 16                                                        */
    uint32_t ip_word;     /* identification | ttl << 16 | (dscp << 2 | ecn) << 24 (dk_tx_segs.ip_word)             */
    uint32_t link;        /* index into links[]                                                                    */
    uint32_t fin_sent;    /* a FIN went out: nothing more is sent                                                  */
    uint16_t rcv_wnd_hdr; /* header window when no receive table is passed                                         */
    uint16_t reserved0;
    uint32_t reserved1;
} dk_tcp_tx_conn;         /* 64 bytes */

/* The pushed buffers of one call, struct of device arrays, [nbufs] each. conn is non-decreasing: the buffers of one
 * connection are adjacent and in push order. (off, len) is the buffer's byte range in the source blob; len == 0 is the
 * end-of-send marker. */
typedef struct dk_tcp_tx_push {
    const uint32_t* conn;
    const uint32_t* off;
    const uint32_t* len;
} dk_tcp_tx_push;

/* Where the frames go: frame f of the call starts at out + f * slot_stride + frame_lead and owns slot f, the bytes
 * [f * slot_stride, (f + 1) * slot_stride) of out. No alignment is required of either value. */
typedef struct dk_tcp_tx_layout {
    uint32_t slot_stride;
    uint32_t frame_lead;
} dk_tcp_tx_layout;

enum dk_tcp_tx_status {
    DK_TCP_TX_SENT = 0,    /* the whole buffer (or the FIN) went out                                               */
    DK_TCP_TX_PARTIAL = 1, /* the window closed inside the buffer: its first `sent` bytes went out                 */
    DK_TCP_TX_UNSENT = 2,  /* the window was closed before the buffer                                              */
    DK_TCP_TX_CLOSED = 3,  /* behind an end-of-send marker, or fin_sent was set                                    */
    DK_TCP_TX_E_CONN = 4,  /* connection-level failure (below): nothing of the connection is sent                  */
    DK_TCP_TX_NO_ROOM = 5  /* the buffer has frames in the plan, but the call's frames do not fit max_frames /
                              out_bytes: nothing of the call is sent                                               */
};

/* Outputs (device). Per frame, [max_frames]: off_out, len_out (a dk_rx_batch over `out`), frame_buf (optional: the
 * push-list index the frame came from). Per buffer, [nbufs]: sent (sequence space consumed: bytes, or 1 for a FIN),
 * first_frame, frame_count (the plan's, also when the call ran out of room; saturating at 0xFFFFFFFF), status (enum
 * dk_tcp_tx_status). n_frames: one word, the frames the plan needs (saturating at 0xFFFFFFFF). */
typedef struct dk_tcp_tx_results {
    uint32_t* off_out;
    uint16_t* len_out;
    uint32_t* frame_buf;
    uint32_t* sent;
    uint32_t* first_frame;
    uint32_t* frame_count;
    uint32_t* status;
    uint32_t* n_frames;
} dk_tcp_tx_results;

typedef struct dk_tcp_tx_ctx dk_tcp_tx_ctx;

/* Scratch (scan buffers, the per-buffer plan) for dk_tcp_tx_segment on `device`; calls on one context are serialised
 * as dk_tcp_ctx's are. Returns 0, EINVAL or ENOMEM. */
int dk_tcp_tx_ctx_create(int32_t device, dk_tcp_tx_ctx** out);
void dk_tcp_tx_ctx_destroy(dk_tcp_tx_ctx* ctx);

/* Upper bound of the frames a push list can need, from host-side lengths: the sum of max(1, ceil(len / mss)) (0 when
 * mss == 0: nothing is ever sent). Pure host function. */
uint64_t dk_tcp_tx_frame_bound(const uint32_t* len, uint32_t nbufs, uint32_t mss);

/* Cut push->*[0 .. nbufs) (ranges of src[0 .. src_bytes), only read) into frames in out[0 .. out_bytes), asynchronously
 * on `stream`. tx_conns[0 .. nconns) is updated in place. Header fields: with rx_conns (the dk_tcp_conn table of the same
 * connections, e.g. as dk_tcp_rx_process just left it on this stream) ack = rx_conns[c].receive_next and window =
 * (buffer_size - (receive_next - reader_next)) >> rcv_wscale; with rx_conns == NULL they are rcv_nxt and rcv_wnd_hdr.
 * The TCP checksum is computed over the copied payload, or written as 0 under DK_TX_OFFLOAD_TCP in `flags`.
 * Frames are numbered in push-list order, so a connection's frames are consecutive and in sequence order. No byte of
 * out outside the frames is written. src and out must not overlap.
 * Connection-level failures (every buffer of the connection gets DK_TCP_TX_E_CONN, its state is untouched): conn index
 * >= nconns, state != ESTABLISHED, a window that does not fit 16 bits (hdr_window_size would panic), link >= nlinks,
 * frame_lead + 54 + mss > slot_stride, mss > 65,481 (the frame of 54 + mss bytes, not the IPv4 datagram, is what the
 * 16-bit len_out and dk_rx_batch.len must hold), a buffer range outside src_bytes.
 * Capacity is all or nothing: n_frames always reports the frames the plan needs; if that exceeds max_frames, or
 * n_frames * slot_stride exceeds out_bytes, no frame is written, no connection is updated, `sent` is 0 everywhere and
 * the buffers that had frames report DK_TCP_TX_NO_ROOM; the caller retries with more room. The test is made on the
 * device: there is no host round trip.
 * Returns 0, EINVAL (null required pointer, misaligned tx_conns, src_bytes or out_bytes > DK_RX_MAX_BLOB, nlinks == 0),
 * ENOMEM or EIO. */
int dk_tcp_tx_segment(dk_tcp_tx_ctx* ctx, const uint8_t* src, uint64_t src_bytes, const dk_tcp_tx_push* push,
                      uint32_t nbufs, dk_tcp_tx_conn* tx_conns, uint32_t nconns, const dk_tcp_conn* rx_conns,
                      const dk_tx_link* links, uint32_t nlinks, uint8_t* out, uint64_t out_bytes,
                      const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t flags,
                      const dk_tcp_tx_results* results, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The sender's reaction to ACKs: what ControlBlock::process_ack (ctrlblk.rs:607-650) hands to Sender::process_ack
 * (sender.rs:406-474, with update_retransmit_deadline :476-488, update_send_window :490-508 and
 * RtoCalculator::add_sample / update_rto, rto.rs:40-79, in f64), for every connection of a batch at once. The
 * segments that reach it are those dk_tcp_rx_process gave DELIVERED, STORED, STORE_DUP, NO_DATA or FIN, in arrival
 * order within their connection. With una = snd_una, per such segment (seq, ack, win = the raw header window):
 *   acked = ack - una (wrapping; 0 = a duplicate ACK, >= 2^31 = an old one)
 *   ack == una: dup_acks += 1
 *   una <seq ack (a new ACK): new_acks += 1; pop ack - una bytes from the unacknowledged queue; una = ack;
 *       if wl1 <seq seq or (wl1 == seq and wl2 <=seq ack): snd_wnd = win << snd_wscale, wl1 = seq, wl2 = ack;
 *       the retransmit deadline follows the queue's front.
 * The unacknowledged queue of connection c is pool[q_first .. q_first + q_count): entries {off, len, tx_time}, len == 0
 * the end-of-send marker, tx_time in nanoseconds or DK_TCP_TX_TIME_NONE (retransmitted, or trimmed: Karn). Popping r
 * bytes, while r != 0, takes the front entry: tx_time != NONE adds the sample now - tx_time (saturating at 0) to the
 * RTO state; len > r trims it (off += r, len -= r, tx_time = NONE) and stops; the marker ends the pop (r = 0) and
 * leaves the queue; otherwise r -= len and the entry leaves the queue. `now_ns` is one value per call. After a new
 * ACK rtx_armed = the queue is not empty and rtx_base_ns = the front's tx_time (now_ns when that is NONE, 0 when the
 * queue is empty); the host adds rto (the Duration conversion stays there). srtt, rttvar and rto are the
 * reference's f64 values bit for bit: rtt = (double)(d / 10^9) + (double)(d % 10^9) / 1e9; the first sample sets
 * srtt = rtt, rttvar = rtt / 2; later ones rttvar = 0.75 rttvar + 0.25 |srtt - rtt|, then srtt = 0.875 srtt + 0.125
 * rtt; rto = clamp(srtt + max(0.001, 4 rttvar), 0.1, 60.0), no operation contracted.
 * One deviation: an ack at wrapping distance exactly 2^31 behind a una that equals snd_nxt compares as new in the
 * reference, which then spins on the empty queue; here it is an old ACK (acked = 2^31, no effect).
 * Congestion control stays with the host: acked[] in arrival order with new_acks / dup_acks is what on_ack_received
 * needs.
 * ------------------------------------------------------------------------------------------------------------- */
#define DK_TCP_TX_TIME_NONE (~0ull)

/* The sender state dk_tcp_tx_conn does not hold, indexed by flow id. Device memory, 16-byte aligned, updated in
 * place. */
typedef struct dk_tcp_ack_conn {
    uint32_t wl1, wl2;         /* SND.WL1 / SND.WL2: send_window_last_update_seq / _ack                            */
    uint32_t snd_wscale;       /* send_window_scale_shift_bits                                                     */
    uint32_t received_sample;  /* RtoCalculator::received_sample                                                   */
    uint32_t q_first, q_count; /* the connection's entries: pool[q_first .. q_first + q_count)                     */
    uint32_t rtx_armed;        /* retransmit_deadline_time_secs is Some                                            */
    uint32_t reserved;
    double srtt, rttvar, rto;  /* RtoCalculator's state (new(): 1.0, 0.0, 1.0)                                      */
    uint64_t rtx_base_ns;      /* the deadline is rtx_base_ns + rto                                                */
} dk_tcp_ack_conn;             /* 64 bytes */

/* The pool of unacknowledged-queue entries, struct of device arrays, [nq] each. */
typedef struct dk_tcp_unacked {
    uint32_t* off;
    uint32_t* len;
    uint64_t* tx_time;
} dk_tcp_unacked;

enum dk_tcp_ack_status {
    DK_TCP_ACK_OK = 0,
    DK_TCP_ACK_E_STATE = 1,    /* tx_conns[c].state != DK_TCP_ESTABLISHED                                          */
    DK_TCP_ACK_E_SND_NXT = 2,  /* rx_conns[c].send_next != tx_conns[c].snd_nxt: the walk judged ack <= SND.NXT
                                  against the former                                                               */
    DK_TCP_ACK_E_FLIGHT = 3,   /* snd_nxt - snd_una >= 2^31                                                        */
    DK_TCP_ACK_E_WSCALE = 4,   /* snd_wscale > 14                                                                  */
    DK_TCP_ACK_E_WL2 = 5,      /* wl2 ahead of snd_una ((int32_t)(wl2 - snd_una) > 0)                              */
    DK_TCP_ACK_E_QUEUE = 6,    /* q_first + q_count beyond the pool                                                */
    DK_TCP_ACK_E_DRY = 7       /* the queue ran dry before the acknowledged bytes were consumed                    */
};

/* Outputs (device). acked: [n], per frame, 0 for frames that are not ACK-processed. Per connection, [nconns]: status
 * (enum dk_tcp_ack_status), new_acks, dup_acks, bytes_acked (SND.UNA's advance), samples (RTT samples taken). A
 * connection-level failure leaves the connection's state and queue untouched, acked 0 for its segments and its
 * counts 0. */
typedef struct dk_tcp_ack_out {
    uint32_t* acked;
    uint32_t* status;
    uint32_t* new_acks;
    uint32_t* dup_acks;
    uint32_t* bytes_acked;
    uint32_t* samples;
} dk_tcp_ack_out;

/* Follows the dk_tcp_rx_process call of the same ctx, with that call's rx, n and nconns, `action` that call's
 * dk_tcp_out.action and rx_conns its table, with no other call on the context between them: it reuses that call's
 * per-connection arrival order, which is still in the context's scratch. Asynchronous on `stream`, serialised with the
 * context's other calls as they are. Writes snd_una and snd_wnd of tx_conns, the ack_conns entries, the pool entry at
 * each queue's front, and `out`; nothing else. The engine runs one lane per connection; one wave per connection at
 * >= 8 segments per connection; at >= 1,024 segments per connection and <= 256 connections the chip form (each
 * 64-segment window's part computed across the chip, one wave per connection for the scan over the windows, the queue
 * and the commit). In the two parallel forms a connection whose wl1 / wl2 / sequence numbers do not allow their ordering
 * argument, or whose pop meets a marker anywhere but as its last byte, is redone by one lane;
 * dk_diag_tcp_ack_set_form (dk_diag.h) forces a form. Results are identical. The environment is never read.
 * Returns 0, ENOMEM, EINVAL (a null required pointer, rx->tcp_win missing, misaligned tx_conns / ack_conns, a call out of turn
 * or with another n / nconns than the dk_tcp_rx_process call before it: nothing is written). */
int dk_tcp_ack_process(dk_tcp_ctx* ctx, const dk_rx_results* rx, uint32_t n, const uint8_t* action,
                       const dk_tcp_conn* rx_conns, dk_tcp_tx_conn* tx_conns, dk_tcp_ack_conn* ack_conns,
                       uint32_t nconns, const dk_tcp_unacked* q, uint32_t nq, uint64_t now_ns,
                       const dk_tcp_ack_out* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Retransmission: Sender::retransmit (sender.rs:375-403) and the timeout branch of background_retransmitter
 * (sender.rs:347-364) with RtoCalculator::back_off (rto.rs:82-84), for every connection of a table at once. The
 * unacknowledged queue holds only {off, len, tx_time} into the source blob, which lives in device memory: the frame
 * is that payload again under fresh headers, copied and summed in one pass as dk_tcp_tx_segment does it.
 * fire[0 .. nconns) is a device array the host fills: DK_TCP_RTX_TIMEOUT for a connection whose deadline
 * rtx_base_ns + Duration(rto) has passed, DK_TCP_RTX_FAST for one its congestion control flagged (retransmit_now),
 * 0 for the others. Deciding who fires stays with the host, as do congestion_control_on_rto / on_fast_retransmit and
 * the Duration::from_secs_f64 conversion: after a TIMEOUT the host re-arms its timer at rtx_base_ns (= now_ns) +
 * Duration(the connection's new rto).
 * Per connection c with fire[c] != 0, in connection order, the first of these that applies gives its status:
 *   the connection's own checks: E_FIRE, E_STATE, E_QUEUE, E_LINK, E_WINDOW (the header window as dk_tcp_tx_segment
 *     computes it: from rx_conns[c] when given, else rcv_wnd_hdr);
 *   IDLE: q_count == 0 (retransmit() returns at once), or TIMEOUT with rtx_armed == 0 (a None deadline cannot
 *     time out);
 *   the front entry's checks: E_RANGE, E_SLOT.
 * Every status but SENT leaves everything of the connection untouched and builds no frame. One deviation: in the
 * reference an armed timer over an empty queue would still back off and re-arm; that state is unreachable there
 * (process_ack disarms on an empty queue, sender.rs:461-468, and send_segment arms only when it pushes), and here it
 * is IDLE.
 * The frame is built from the front entry e = q_first as it stands (an off / len a partial ACK moved included), sent
 * whole even when it is longer than the connection's current mss (sender.rs:391: no repacketization): the 54 header
 * bytes dk_tcp_tx_segment writes for this connection (ack / window from rx_conns[c] when given, else rcv_nxt /
 * rcv_wnd_hdr; Ethernet / IPv4 from links[link], ip_word, the addresses and ports), seq = snd_una, flags ACK|PSH, or
 * ACK|FIN when len == 0 (the end-of-send marker), payload src[off, off + len), the TCP checksum over it, or 0 under
 * DK_TX_OFFLOAD_TCP. Frames are numbered in connection order; frame f owns slot f under dk_tcp_tx_layout's rule. No
 * byte of out outside the frames is written. src and out must not overlap.
 * State: q.tx_time[e] = DK_TCP_TX_TIME_NONE for both kinds (Karn, sender.rs:384-386). TIMEOUT additionally:
 * rto = clamp(rto * 2.0, 0.1, 60.0) in f64, bit for bit; rtx_base_ns = now_ns; rtx_armed = 1. FAST leaves rto,
 * rtx_base_ns and rtx_armed alone. Never written: tx_conns, q.off / q.len, every other pool entry, every other field
 * of ack_conns.
 * Capacity is all or nothing, tested on the device exactly as dk_tcp_tx_segment tests it: n_frames always reports the
 * frames the call needs; if that exceeds max_frames, or n_frames * slot_stride exceeds out_bytes, no frame, no tx_time
 * and no ack_conns field is written, the connections that had a frame report NO_ROOM and every frame[c] is 0xFFFFFFFF.
 * Ordering against dk_tcp_ack_process and dk_tcp_tx_commit, which touch the same rows, is the caller's: they run on
 * one stream. This entry point is additive: DK_RX_ABI_VERSION stays 4.
 * ------------------------------------------------------------------------------------------------------------- */
enum dk_tcp_rtx_fire { DK_TCP_RTX_NONE = 0, DK_TCP_RTX_TIMEOUT = 1, DK_TCP_RTX_FAST = 2 };

enum dk_tcp_rtx_status {
    DK_TCP_RTX_NOT_FIRED = 0,
    DK_TCP_RTX_SENT = 1,      /* a frame was built                                                               */
    DK_TCP_RTX_IDLE = 2,      /* nothing to resend (above): nothing changed                                      */
    DK_TCP_RTX_E_FIRE = 3,    /* fire[c] > 2                                                                     */
    DK_TCP_RTX_E_STATE = 4,   /* tx_conns[c].state != DK_TCP_ESTABLISHED                                         */
    DK_TCP_RTX_E_QUEUE = 5,   /* q_first + q_count beyond the pool                                               */
    DK_TCP_RTX_E_RANGE = 6,   /* the front's off + len beyond src_bytes                                          */
    DK_TCP_RTX_E_SLOT = 7,    /* frame_lead + 54 + len > slot_stride, or len > 65,481                            */
    DK_TCP_RTX_E_LINK = 8,    /* link >= nlinks                                                                  */
    DK_TCP_RTX_E_WINDOW = 9,  /* the header window does not fit 16 bits (as dk_tcp_tx_segment judges it)         */
    DK_TCP_RTX_NO_ROOM = 10   /* had a frame, but the call's frames do not fit: nothing of the call is done      */
};

/* Outputs (device). Per frame, [max_frames]: off_out, len_out (a dk_rx_batch over `out`), frame_conn (optional: the
 * connection the frame belongs to). Per connection, [nconns]: status (enum dk_tcp_rtx_status), frame (the
 * connection's frame index, 0xFFFFFFFF when it has none). n_frames: one word, the frames the call needs. */
typedef struct dk_tcp_rtx_results {
    uint32_t* off_out;
    uint16_t* len_out;
    uint32_t* frame_conn;
    uint32_t* status;
    uint32_t* frame;
    uint32_t* n_frames;
} dk_tcp_rtx_results;

/* Asynchronous on `stream`; calls on one dk_tcp_tx_ctx (dk_tcp_retransmit and dk_tcp_tx_segment alike) are serialised.
 * tx_conns, rx_conns (optional), the pool's off / len and fire are only read. nconns == 0 and an all-zero fire are
 * valid calls that write n_frames = 0.
 * Returns 0, EINVAL (a null required pointer, tx_conns / ack_conns / rx_conns not 16-byte aligned, src_bytes or
 * out_bytes > DK_RX_MAX_BLOB, nlinks == 0), ENOMEM or EIO. */
int dk_tcp_retransmit(dk_tcp_tx_ctx* ctx, const uint8_t* src, uint64_t src_bytes, const uint8_t* fire,
                      const dk_tcp_tx_conn* tx_conns, dk_tcp_ack_conn* ack_conns, uint32_t nconns,
                      const dk_tcp_conn* rx_conns, const dk_tcp_unacked* q, uint32_t nq, uint64_t now_ns,
                      const dk_tx_link* links, uint32_t nlinks, uint8_t* out, uint64_t out_bytes,
                      const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t flags,
                      const dk_tcp_rtx_results* results, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The receiver's ACKs: what ControlBlock::process_packet (ctrlblk.rs:403-440) decides per segment and send_ack
 * (:712-720, tcp_header :699-709, emit :723-776) sends, for every connection of a batch at once, and the delayed-ACK
 * timer's expiry (background/acknowledger.rs). An ACK is a frame of 54 bytes, no payload and no options: exactly what
 * dk_tcp_tx_segment would write for the connection with an empty payload (Ethernet / IPv4 from links[link], ip_word,
 * the addresses and ports; IPv4 total length 40; both checksums filled, the TCP checksum 0 under DK_TX_OFFLOAD_TCP;
 * no padding), flags ACK, seq = tx_conns[c].snd_nxt, ack = RCV.NXT and window = (buffer_size - (RCV.NXT -
 * reader_next)) >> rcv_wscale, both as they stood when the ACK was sent: after the segment that triggered it, not at
 * the end of the batch. reader_next, buffer_size and SND.NXT do not move during a call.
 * Per segment of a connection, in arrival order, by the action dk_tcp_rx_process gave it (armed =
 * receive_ack_deadline_time_secs.is_some()):
 *   DELIVERED, NO_DATA       an ACK only if armed; armed toggles: 0 -> 1 with deadline_ns = now_ns + delay_ns, 1 -> 0
 *                            (ctrlblk.rs:426-437)
 *   STORED, STORE_DUP        an ACK; armed = 1, deadline_ns = now_ns + delay_ns (:680-682 sends and clears, then
 *                            :426-431 finds the deadline None and arms it: the reference's quirk, kept)
 *   FIN                      an ACK, after RCV.NXT moved over the FIN; armed = 0 (:1011-1016 returns before the toggle)
 *   DUPLICATE, OUT_OF_WINDOW an ACK and armed = 0, unless the segment has RST set: then nothing (:495-501, :525-531)
 *   ACK_UNSENT               an ACK; armed = 0 (:640-646)
 *   RST, SYN, NO_ACK, UNPROCESSED, SKIP: nothing (:570-613, :355-363)
 * deadline_ns is left as it is when armed is cleared; a connection none of whose segments touched armed keeps its row
 * byte for byte. `now_ns` is one value per call. armed != 0 counts as armed; 0 or 1 is written.
 * RCV.NXT at a segment is not in the table after the call, but it moves only at DELIVERED and FIN segments, and those
 * start exactly at RCV.NXT once their front is trimmed: RCV.NXT after frame i is the trimmed start (seq + the view's
 * offset into the payload + 1 for a trimmed SYN) of the connection's next DELIVERED / FIN frame, the table's
 * receive_next when there is none. The pass needs that call's action and view, and the order it left in the context.
 * Connection-level failures, the first that applies, in this order (the connection's row is untouched, nothing is
 * emitted for it, n_acks 0):
 *   E_STATE    tx_conns[c].state != DK_TCP_ESTABLISHED
 *   E_SND_NXT  rx_conns[c].send_next != tx_conns[c].snd_nxt
 *   E_LINK     link >= nlinks
 *   E_WSCALE   rcv_wscale > 14
 *   E_WINDOW   buffer_size >> rcv_wscale > 0xFFFF: the full-open window is what hdr_window_size would panic on, and
 *              judged this way the check does not depend on where RCV.NXT stood (a table whose RCV.NXT - reader_next
 *              exceeds buffer_size gets the low 16 bits of the wrapped difference)
 *   E_SLOT     frame_lead + 54 > slot_stride
 * Frames are numbered in the order of the batch frames that triggered them (dk_tcp_ack_timer: in connection order),
 * so a connection's ACKs are in arrival order; frame f owns slot f under dk_tcp_tx_layout's rule. No byte of out
 * outside the frames is written. Capacity is all or nothing, tested on the device as dk_tcp_tx_segment tests it:
 * n_frames always reports the frames the call needs; if that exceeds max_frames, or n_frames * slot_stride exceeds
 * out_bytes, no frame and no dack field is written, ack_frame is 0xFFFFFFFF everywhere and the connections that had
 * frames report NO_ROOM (n_acks still holds their need). Such a dk_tcp_ack_emit call has taken its turn all the same
 * (the test is made on the device): n slots are the most a batch can need. Nothing but dack, the frames and the
 * outputs is ever written.
 * Clearing armed when a data frame of the connection piggybacks the ACK (emit, :761) is not done by
 * dk_tcp_tx_segment and dk_tcp_retransmit themselves, which do not touch dack: it is dk_tcp_tx_commit's and
 * dk_tcp_rtx_piggyback's (below), the calls that follow them.
 * These entry points are additive: DK_RX_ABI_VERSION stays 4.
 * ------------------------------------------------------------------------------------------------------------- */
/* The delayed-ACK state of one connection, indexed by flow id. Device memory, 16-byte aligned, updated in place. */
typedef struct dk_tcp_dack_conn {
    uint32_t armed;        /* receive_ack_deadline_time_secs is Some                                              */
    uint32_t reserved;
    uint64_t delay_ns;     /* receive_ack_delay_timeout_secs (input)                                              */
    uint64_t deadline_ns;  /* now_ns + delay_ns (wrapping) of the call that armed it last                         */
    uint64_t reserved1;
} dk_tcp_dack_conn;        /* 32 bytes */

enum dk_tcp_ackemit_status {
    DK_TCP_ACKEMIT_OK = 0,         /* dk_tcp_ack_timer: the ACK was sent                                          */
    DK_TCP_ACKEMIT_E_STATE = 1,
    DK_TCP_ACKEMIT_E_SND_NXT = 2,
    DK_TCP_ACKEMIT_E_LINK = 3,
    DK_TCP_ACKEMIT_E_WSCALE = 4,
    DK_TCP_ACKEMIT_E_WINDOW = 5,
    DK_TCP_ACKEMIT_E_SLOT = 6,
    DK_TCP_ACKEMIT_NO_ROOM = 7,    /* had frames, but the call's frames do not fit: nothing of the call is done   */
    DK_TCP_ACKEMIT_NOT_FIRED = 8,  /* dk_tcp_ack_timer: fire[c] == 0                                              */
    DK_TCP_ACKEMIT_IDLE = 9        /* dk_tcp_ack_timer: armed == 0, nothing changed                               */
};

/* Outputs (device). Per frame, [max_frames]: off_out, len_out (a dk_rx_batch over `out`), frame_conn (optional: the
 * frame's connection), frame_seg (optional, dk_tcp_ack_emit only: the batch frame that triggered it). ack_frame: per
 * batch frame [n] (dk_tcp_ack_emit) or per connection [nconns] (dk_tcp_ack_timer), its ACK's frame index or
 * 0xFFFFFFFF. Per connection, [nconns]: status (enum dk_tcp_ackemit_status), n_acks (the ACKs it needs). n_frames:
 * one word, the frames the call needs. */
typedef struct dk_tcp_ackemit_results {
    uint32_t* off_out;
    uint16_t* len_out;
    uint32_t* frame_conn;
    uint32_t* frame_seg;
    uint32_t* ack_frame;
    uint32_t* status;
    uint32_t* n_acks;
    uint32_t* n_frames;
} dk_tcp_ackemit_results;

/* Follows the dk_tcp_rx_process call of the same ctx, with that call's rx (flow_id is required), n and nconns, `action`
 * and `view` that call's dk_tcp_out arrays and rx_conns its table, as dk_tcp_ack_process does. It keeps a turn counter
 * of its own: dk_tcp_ack_emit and dk_tcp_ack_process may both follow one dk_tcp_rx_process call, in either order, with
 * identical results; a second dk_tcp_ack_emit on the same call, a call out of turn or one with another n / nconns
 * returns EINVAL and writes nothing. rx_conns and tx_conns are only read. Asynchronous on `stream`, serialised with
 * the context's other calls as they are. The engine runs one lane per connection (the specification in code); at >= 8
 * segments per connection the scan form (the armed bit and the RCV.NXT of each moment as two scans over the whole
 * batch in its order by connection); dk_diag_tcp_ack_emit_set_form (dk_diag.h) forces a form. Results are identical;
 * the frames are written frame-major in both. The environment is never read.
 * Returns 0, EINVAL (also: a null required pointer, rx_conns / tx_conns / dack not 16-byte aligned, out_bytes >
 * DK_RX_MAX_BLOB, nlinks == 0), ENOMEM or EIO. */
int dk_tcp_ack_emit(dk_tcp_ctx* ctx, const dk_rx_results* rx, uint32_t n, const uint8_t* action,
                    const dk_tcp_view* view, const dk_tcp_conn* rx_conns, const dk_tcp_tx_conn* tx_conns,
                    dk_tcp_dack_conn* dack, uint32_t nconns, const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns,
                    uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames,
                    uint32_t flags, const dk_tcp_ackemit_results* results, void* stream);

/* The acknowledger's expiry: fire[0 .. nconns) is a device array the host fills, nonzero for a connection whose
 * deadline_ns has passed on its clock. Per fired connection, in connection order: the connection-level checks above,
 * then armed == 0 is IDLE and changes nothing, else one ACK from the tables as they stand (rx_conns is required) and
 * armed = 0. The frames come from the same device builder as dk_tcp_ack_emit's; the capacity rule is the same;
 * results->frame_seg is not used. A call on dk_tcp_tx_ctx, serialised as dk_tcp_retransmit is. nconns == 0 and an
 * all-zero fire are valid calls that write n_frames = 0. Returns 0, EINVAL, ENOMEM or EIO as above. */
int dk_tcp_ack_timer(dk_tcp_tx_ctx* ctx, const uint8_t* fire, const dk_tcp_tx_conn* tx_conns,
                     const dk_tcp_conn* rx_conns, dk_tcp_dack_conn* dack, uint32_t nconns, const dk_tx_link* links,
                     uint32_t nlinks, uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout,
                     uint32_t max_frames, uint32_t flags, const dk_tcp_ackemit_results* results, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Congestion control and timer expiry: CUBIC as established/congestion_control/cubic.rs states it (the reference's
 * default algorithm), called as ControlBlock::process_ack calls it (ctrlblk.rs:622-630: on_ack_received for every
 * segment that reaches process_ack, before the ack_num <= SND.NXT test), as Sender::send_segment calls it
 * (sender.rs:124-177: on_cwnd_check_before_send, then on_send with the bytes in flight) and as
 * background_retransmitter calls it (sender.rs:320-364: the retransmit_now flag and on_fast_retransmit, the deadline
 * and on_rto), for every connection of a table at once. With these the "Not modelled" list at the top of this file
 * and dk_tcp_retransmit's "deciding who fires stays with the host" are superseded: tx_conns[c].cwnd and fire[] are
 * computed on the device.
 *
 * Arithmetic, bit for bit:
 *   u32 arithmetic wraps, as in the reference's release build (the debug build's overflow panics are not modelled);
 *     saturating_sub saturates. Sequence comparisons take the sign of the wrapping difference
 *     (sequence_number.rs:76-101).
 *   `f32 as u32` is Rust's cast: NaN and negative values give 0, values >= 2^32 give 0xFFFFFFFF, otherwise truncation.
 *   Every f32 operation is rounded once, in source order, none contracted; the constants fold in f32: BETA_CUBIC =
 *     0.7f, C = 0.4f, `1. - BETA_CUBIC` = fl(1 - 0.7f), `1. + BETA_CUBIC` = fl(1 + 0.7f), `3.*(1.-bc)/(1.+bc)` =
 *     fl(fl(3 fl(1 - bc)) / fl(1 + bc)). Division is IEEE, denormals are kept. powi(3) of d is fl(fl(d d) d).
 *   Duration::as_secs_f32 of ns nanoseconds is (float)(ns / 10^9) + (float)(ns % 10^9) / 1e9f. t =
 *     as_secs_f32(now_ns - ca_start_ns), the difference saturating at 0 (Instant::elapsed); rtt =
 *     as_secs_f32(rto_ns(rto)).
 *   rto_ns(double rto) is Duration::from_secs_f64 (the reference's toolchain, nightly-2024-09-25): the real value
 *     rto * 10^9 rounded to nearest, ties to even, computed exactly from rto's mantissa by a 64 x 64 -> 128-bit
 *     product, never as an f64 product. One helper serves the device and the host: dk_tcp_rto_ns below. A row whose
 *     rto is not in [0, 1e9] seconds (NaN included) is the connection-level failure E_RTO: the reference would panic.
 *   K's cube root (cubic.rs:200) is the correctly rounded f32 cube root. A stated deviation: the reference calls the
 *     platform's cbrtf, which is only faithful (glibc 2.35's differs from correct rounding on about a tenth of
 *     uniform inputs, always by one ulp), so there is no single reference bit pattern to match. The device takes the
 *     f64 cube root, rounds it to f32 and, where the f64 value lies within 2^-46 of the midpoint m of two f32
 *     values, decides by the sign of x - m^3 computed exactly (m^2 is exact in f64, m^3 = p + e by one fma).
 *
 * The congestion-control state of one connection, indexed by flow id. Device memory, 16-byte aligned, updated in
 * place. mss is tx_conns[c].mss. A row with DK_TCP_CC_CUBIC clear is the algorithm None (congestion_control/none.rs):
 * every call leaves the row and tx_conns[c].cwnd untouched; dk_tcp_timers' deadline still works for it.
 * ------------------------------------------------------------------------------------------------------------- */
#define DK_TCP_CC_CUBIC 1u            /* clear: the algorithm None                                                 */
#define DK_TCP_CC_FAST_CONVERGENCE 2u /* Cubic::fast_convergence (cubic.rs:42)                                     */
#define DK_TCP_CC_IN_RECOVERY 4u      /* in_fast_recovery                                                          */
#define DK_TCP_CC_LAST_WAS_RTO 8u     /* last_congestion_was_rto                                                   */
#define DK_TCP_CC_RETRANSMIT_NOW 16u  /* fast_retransmit_now                                                       */

typedef struct dk_tcp_cc_conn {
    uint32_t flags;         /* DK_TCP_CC_*                                                                         */
    uint32_t cwnd;          /* Cubic::cwnd (cubic.rs:41); Cubic::new: 4 / 3 / 2 x mss (mss <= 1095 / <= 2190 / above) */
    uint32_t ssthresh;      /* new(): 0xFFFFFFFF                                                                   */
    uint32_t w_max;         /* new(): 0                                                                            */
    uint32_t initial_cwnd;
    uint32_t ltci;          /* limited_transmit_cwnd_increase                                                      */
    uint32_t dup_acks;      /* duplicate_ack_count                                                                 */
    uint32_t rpif;          /* retransmitted_packets_in_flight                                                     */
    uint32_t recover;       /* new(): the initial send sequence number                                             */
    uint32_t prev_ack;      /* prev_ack_seq_no; new(): the initial send sequence number                            */
    uint64_t ca_start_ns;   /* ca_start                                                                            */
    uint64_t last_send_ns;  /* last_send_time                                                                      */
    uint64_t rtt_at_last_send_ns;  /* rtt_at_last_send; new(): 10^9                                                */
} dk_tcp_cc_conn;           /* 64 bytes */

/* Duration::from_secs_f64(rto).as_nanos() as above; 0 for an rto outside [0, 1e9] (E_RTO's condition). Pure host
 * function: the same code the kernels run. */
uint64_t dk_tcp_rto_ns(double rto);

enum dk_tcp_cc_status {
    DK_TCP_CC_OK = 0,
    DK_TCP_CC_E_STATE = 1,    /* tx_conns[c].state != DK_TCP_ESTABLISHED                                          */
    DK_TCP_CC_E_SND_NXT = 2,  /* rx_conns[c].send_next != tx_conns[c].snd_nxt (dk_tcp_cc_ack only)                */
    DK_TCP_CC_E_MSS = 3,      /* a CUBIC row with mss == 0: the reference divides by it                           */
    DK_TCP_CC_E_RTO = 4       /* rto outside [0, 1e9] seconds or NaN                                              */
};

/* dk_tcp_cc_ack: SlowStartCongestionAvoidance::on_ack_received (cubic.rs:307-328 with :113-246) for a whole batch.
 * It follows the dk_tcp_rx_process call of the same ctx as dk_tcp_ack_emit does (that call's rx, n, nconns, `action`
 * and rx_conns), with a turn counter of its own, and it must precede that batch's dk_tcp_ack_process: it reads
 * snd_una and rto as that call has not yet moved them. A call after the batch's dk_tcp_ack_process, a second call, a
 * call out of turn or one with another n / nconns returns EINVAL and writes nothing. Its order with dk_tcp_ack_emit
 * is free, with identical results.
 * One lane per connection walks the connection's segments in arrival order and visits those whose action is DELIVERED,
 * STORED, STORE_DUP, NO_DATA, FIN or ACK_UNSENT (ctrlblk.rs:629 calls congestion control before the ack <= SND.NXT
 * test of :633). With a running una that starts at tx_conns[c].snd_una, per visited segment:
 *   1. on_ack_received(rto, una, snd_nxt, ack), literally. Its quirks are kept: an old ACK (ack - una >= 2^31) is
 *      "new data" to CUBIC (bytes_acknowledged != 0); retransmitted_packets_in_flight decrements on every duplicate;
 *      recovery starts at the third duplicate by `ack - 1 > recover` or by the "retransmitted packet dropped" heuristic
 *      (cwnd > mss and ack - prev_ack <= 4 mss); ca_start = now_ns on a full acknowledgement.
 *   2. una = ack if the action is not ACK_UNSENT and 0 < ack - una < 2^31: dk_tcp_ack_process's rule, its 2^31
 *      deviation included.
 * Then the row is written and tx_conns[c].cwnd = cwnd + limited_transmit_cwnd_increase (wrapping), the effective
 * window dk_tcp_tx_segment expects.
 * One deviation: rto is one value per call, ack_conns[c].rto as the call finds it, as now_ns is. The reference reads
 * it per segment; the two agree whenever no earlier segment of the same connection in the batch took an RTT sample
 * (rto moves only in RtoCalculator::add_sample, and only congestion avoidance reads it).
 * Connection-level failures, the first that applies (the row and tx_conns[c].cwnd stay untouched, counts 0): E_STATE,
 * E_SND_NXT, E_MSS, E_RTO. A None row reports OK with counts 0.
 * Outputs (device): status, new_acks (visited segments with ack != una), dup_acks (ack == una): [nconns];
 * cwnd_after (optional): [n], cwnd after each visited segment, 0 elsewhere.
 * Returns 0, EINVAL (also: a null required pointer, tx_conns / ack_conns / cc not 16-byte aligned) or EIO. */
typedef struct dk_tcp_cc_ack_out {
    uint32_t* status;
    uint32_t* new_acks;
    uint32_t* dup_acks;
    uint32_t* cwnd_after;
} dk_tcp_cc_ack_out;

int dk_tcp_cc_ack(dk_tcp_ctx* ctx, const dk_rx_results* rx, uint32_t n, const uint8_t* action,
                  const dk_tcp_conn* rx_conns, dk_tcp_tx_conn* tx_conns, const dk_tcp_ack_conn* ack_conns,
                  dk_tcp_cc_conn* cc, uint32_t nconns, uint64_t now_ns, const dk_tcp_cc_ack_out* out, void* stream);

/* dk_tcp_timers: one turn of background_retransmitter's loop (sender.rs:325-364) and the acknowledger's deadline for
 * every connection. Per connection c, after the checks E_STATE, E_MSS (a CUBIC row with mss == 0: on_rto divides by
 * it) and E_RTO, the first that applies (the row untouched, rtx_fire[c] = 0):
 *   fast_retransmit_now set (a CUBIC row): on_fast_retransmit clears it (cubic.rs:346-351), rtx_fire[c] =
 *     DK_TCP_RTX_FAST;
 *   else rtx_armed and now_ns >= rtx_base_ns + rto_ns(rto) (the timer fires at expiry <= now, runtime/timer.rs:215; the
 *     sum saturates): on_rto(snd_una) (cubic.rs:248-278, :330-334; nothing for None), rtx_fire[c] = DK_TCP_RTX_TIMEOUT;
 *   else rtx_fire[c] = 0.
 * on_rto runs before the retransmission, as in the reference; the back-off and the re-arming stay in dk_tcp_retransmit,
 * which follows on the same stream with rtx_fire as its fire[]. A CUBIC connection whose queue is empty still consumes
 * its flag, as the reference's loop does; an armed timer over an empty queue (unreachable in the reference, see
 * dk_tcp_retransmit's IDLE note) still runs on_rto and fires here, and dk_tcp_retransmit then reports IDLE for it
 * and leaves it armed: the caller that builds such a row gets a TIMEOUT at every call.
 * tx_conns[c].cwnd is refreshed to cwnd + limited_transmit_cwnd_increase for CUBIC rows without a failure.
 * With dack and ack_fire: ack_fire[c] = dack[c].armed != 0 && now_ns >= dack[c].deadline_ns, dk_tcp_ack_timer's fire[],
 * whatever the row's status; dack is only read. Both or neither are given.
 * Outputs (device): status [nconns]; n_fast, n_timeout, n_ack: one word each, the connections set in rtx_fire /
 * ack_fire, so that the host can skip the follow-up calls without reading an array (n_ack = 0 without ack_fire).
 * A call on dk_tcp_tx_ctx, serialised as dk_tcp_retransmit is. ack_conns is only read. nconns == 0 is a valid call that
 * writes the three words. Returns 0, EINVAL (a null required pointer, a misaligned table) or EIO. */
typedef struct dk_tcp_timers_out {
    uint32_t* status;
    uint32_t* n_fast;
    uint32_t* n_timeout;
    uint32_t* n_ack;
} dk_tcp_timers_out;

int dk_tcp_timers(dk_tcp_tx_ctx* ctx, dk_tcp_tx_conn* tx_conns, const dk_tcp_ack_conn* ack_conns, dk_tcp_cc_conn* cc,
                  const dk_tcp_dack_conn* dack, uint32_t nconns, uint64_t now_ns, uint8_t* rtx_fire, uint8_t* ack_fire,
                  const dk_tcp_timers_out* out, void* stream);

/* dk_tcp_cc_send: the two hooks of Sender::send_segment, around one dk_tcp_tx_segment call on the same stream.
 * DK_TCP_CC_BEFORE_SEND, on_cwnd_check_before_send (cubic.rs:290-298), for every CUBIC row: if now_ns - last_send_ns
 *   (saturating at 0) is strictly greater than rtt_at_last_send_ns, cwnd = min(initial_cwnd, cwnd) and
 *   limited_transmit_cwnd_increase = 0; then tx_conns[c].cwnd = cwnd + limited_transmit_cwnd_increase. push, nbufs
 *   and results are not used.
 * DK_TCP_CC_AFTER_SEND, on_send (cubic.rs:300-305), takes the push list, nbufs and the dk_tcp_tx_results of the
 *   dk_tcp_tx_segment call just made: for every CUBIC connection that got at least one frame, last_send_ns = now_ns,
 *   rtt_at_last_send_ns = rto_ns(rto), and limited_transmit_cwnd_increase = saturating_sub(it, the sum over the
 *   connection's frames j of (snd_nxt before frame j - snd_una)): on_send is given the bytes in flight, not the bytes
 *   sent, and it is called before send_segment moves SND.NXT over the frame (sender.rs:177, ahead of :193), so the
 *   first frame of an idle connection takes nothing off; a quirk kept. A chain of saturating subtractions of
 *   non-negative terms is one saturating subtraction of their sum, so the lane stops once the increase is 0.
 *   tx_conns[c].cwnd is refreshed for those connections. A call that reported NO_ROOM sent nothing and changes
 *   nothing.
 * As dk_tcp_tx_segment's section says, cwnd does not move between the frames of one segmentation call.
 * status [nconns]: OK, E_STATE, E_RTO (AFTER_SEND only, for a connection that got frames; the row untouched).
 * A call on dk_tcp_tx_ctx, serialised as dk_tcp_tx_segment is. Returns 0, EINVAL (a phase that is neither, a null
 * required pointer, a misaligned table) or EIO. */
enum dk_tcp_cc_phase { DK_TCP_CC_BEFORE_SEND = 0, DK_TCP_CC_AFTER_SEND = 1 };

int dk_tcp_cc_send(dk_tcp_tx_ctx* ctx, uint32_t phase, dk_tcp_tx_conn* tx_conns, const dk_tcp_ack_conn* ack_conns,
                   dk_tcp_cc_conn* cc, uint32_t nconns, const dk_tcp_tx_push* push, uint32_t nbufs,
                   const dk_tcp_tx_results* results, uint64_t now_ns, uint32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The send side's bookkeeping: the "post-send operations" of Sender::send_segment (sender.rs:195-206) and of
 * ControlBlock::emit (ctrlblk.rs:761), for every connection of one dk_tcp_tx_segment call at once. Every frame that
 * call sent is pushed onto its connection's unacknowledged queue with its transmit time, a disarmed retransmit timer
 * is armed, and the delayed-ACK deadline of a connection that sent anything is cancelled: the frames carried the ACK.
 * Regions: connection c owns pool[c * q_cap, (c + 1) * q_cap); its live entries pool[q_first, q_first + q_count) lie
 * inside it.
 * Which frames: the frames of buffer b count iff results->status[b] is DK_TCP_TX_SENT or DK_TCP_TX_PARTIAL; they are
 * first_frame[b] .. first_frame[b] + frame_count[b]), and a connection's frames are consecutive. k = their number for
 * the connection. Nothing is read by the host: n_frames stays on the device.
 * Per connection c with k > 0, the first of these that applies (64-bit arithmetic):
 *   E_QUEUE  q_count > q_cap, or q_count > 0 and [q_first, q_first + q_count) is not inside the region
 *   E_FULL   q_count + k > q_cap. A sizing error of the caller's: the frames are already on the wire and cannot be
 *            queued later, so they will never be retransmitted. Size q_cap for the largest window in segments
 *            (dk_tcp_tx_segment is not limited by queue room).
 *   both leave the row and the region untouched, appended = 0.
 *   q_count == 0: q_first' = c * q_cap, whatever q_first was;
 *   q_first + q_count + k <= (c + 1) * q_cap: the entries go in place, q_first' = q_first;
 *   otherwise the live entries move, in order, to the start of the region and q_first' = c * q_cap.
 * Entry j of the connection, for frame f of buffer b, is pool[q_first' + q_count + j] = {off = push->off[b] + the
 * payload bytes of b's earlier frames (wrapping), len = len_out[f] - 54 (the FIN frame becomes the end-of-send marker,
 * len 0), tx_time = now_ns}. Then q_count' = q_count + k, and if rtx_armed == 0: rtx_armed = 1, rtx_base_ns = now_ns
 * (a nonzero rtx_armed is armed and keeps its base). No other field of the row is written. Entries of the region
 * outside the new live range hold unspecified values after a successful commit.
 * With dack: dack[c].armed = 0 for every connection with k > 0, whatever its status; deadline_ns is left as it is
 * (dk_tcp_ack_emit's rule); every other dack row keeps its bytes.
 * Never written: the rows of connections with k == 0 (malformed ones too: their status is OK), other connections'
 * regions, pool entries at or beyond nconns * q_cap, tx_conns, push, results.
 * Turn: the call follows one dk_tcp_tx_segment call of the same ctx that returned 0, with that call's push, nbufs,
 * results (frame_buf is required) and max_frames; dk_tcp_cc_send, dk_tcp_retransmit, dk_tcp_timers and dk_tcp_ack_timer
 * may come between. Its order with dk_tcp_cc_send(AFTER_SEND) is free, with identical results. A second commit for
 * one segmentation call, a commit with none before it or with another nbufs returns EINVAL and writes nothing. A
 * segmentation call that reported NO_ROOM sent nothing: its commit is a valid call that changes nothing and writes
 * status OK, appended 0 everywhere.
 * The engine runs one wave per connection; at >= 1,024 frame slots (max_frames) per connection the chip form (one
 * wave per connection for the decision, the move and the row, then one lane per frame across the chip for the
 * entries); dk_diag_tcp_commit_set_form (dk_diag.h) forces a form. Results are identical. The environment is never
 * read.
 * Asynchronous on `stream`, serialised with the context's other calls as they are. nbufs == 0 and nconns == 0 are
 * valid. Returns 0, EIO, ENOMEM or EINVAL (decided before any GPU work: a null required pointer, ack_conns / dack not
 * 16-byte aligned, nconns * q_cap > nq, now_ns == DK_TCP_TX_TIME_NONE, which would read as "retransmitted", a call out
 * of turn). This entry point is additive: DK_RX_ABI_VERSION stays 4.
 * ------------------------------------------------------------------------------------------------------------- */
enum dk_tcp_commit_status { DK_TCP_COMMIT_OK = 0, DK_TCP_COMMIT_E_QUEUE = 1, DK_TCP_COMMIT_E_FULL = 2 };

/* Outputs (device), [nconns] each. */
typedef struct dk_tcp_commit_out {
    uint32_t* status;    /* enum dk_tcp_commit_status                 */
    uint32_t* appended;  /* entries appended (0 on a failure)         */
} dk_tcp_commit_out;

int dk_tcp_tx_commit(dk_tcp_tx_ctx* ctx, const dk_tcp_tx_push* push, uint32_t nbufs,
                     const dk_tcp_tx_results* results, uint32_t max_frames, dk_tcp_ack_conn* ack_conns,
                     uint32_t nconns, const dk_tcp_unacked* q, uint32_t nq, uint32_t q_cap,
                     dk_tcp_dack_conn* dack /* optional */, uint64_t now_ns, const dk_tcp_commit_out* out,
                     void* stream);

/* A retransmitted frame carries the ACK too: dack[c].armed = 0 where results->status[c] == DK_TCP_RTX_SENT, for the
 * results of any dk_tcp_retransmit call; every other byte is untouched. Idempotent; it takes no turn. A call on
 * dk_tcp_tx_ctx, serialised as dk_tcp_retransmit is. Returns 0, EINVAL (a null required pointer, a misaligned dack)
 * or EIO. */
int dk_tcp_rtx_piggyback(dk_tcp_tx_ctx* ctx, const dk_tcp_rtx_results* results, dk_tcp_dack_conn* dack,
                         uint32_t nconns, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The passive open: what SharedPassiveSocket does with the frames that reach a listening socket (passive_open.rs:
 * poll :137-195, handle_new_syn :197-240, send_rst :243-285, send_syn_ack_and_wait_for_ack :287-359, send_syn_ack
 * :361-393, wait_for_ack :395-481), for every listener-bound frame of one dk_rx_process batch at once. The
 * `connections` maps of all listeners are one open-addressing table in device memory that the device itself inserts
 * into (dk_tcp_listen_table); the listeners are rows of dk_tcp_listener; lsn_of_flow[nflows] maps a frame's flow_id (a
 * DK_FLOW_TCP_PASSIVE entry of the socket table) to its listener row, DK_TCP_LSN_NONE for every other flow.
 *
 * dk_tcp_listen_process covers the frames with verdict DK_V_OK_TCP whose flow_id maps to a listener that is
 * LISTENING and passes the listener checks below; every other frame gets action SKIP. Frames are taken in arrival
 * order (batch index), and each coroutine is taken to have run to its next await before the next frame arrives (the
 * reference's scheduler leaves that open). The key is (listener row, remote ip, remote port). Per frame:
 *   1. The key has an entry.
 *      SYN_RCVD     the segment wait_for_ack pops. ack_num != local_isn + 1: the entry becomes FAILED / EBADMSG, action
 *                   BAD_ACK, an error record goes to the ready list. Otherwise the entry becomes ESTABLISHED, action
 *                   ESTABLISHED, or ESTABLISHED_DATA when the payload is not empty (the reference re-queues the segment
 *                   for the new socket), and a ready record is appended. Nothing else is tested, as in the reference:
 *                   not the ACK bit, RST, SYN or seq. A retransmitted SYN therefore fails the handshake.
 *      ESTABLISHED  action FORWARD: the frame is for the socket's ControlBlock::poll; the host routes it by slot[].
 *      FAILED       action ORPHANED. The reference never removes the entry of a failed handshake: it stays, swallows
 *                   the remote's frames and counts against the backlog until dk_tcp_listen_release. The quirk is kept.
 *   2. No entry.
 *      !syn || ack || rst: a RST reply, action RST_FLAGS.
 *      Otherwise a SYN (its payload is ignored). inflight >= max_backlog: a RST reply, action RST_BACKLOG. Otherwise
 *      an entry is made: local_isn = crc + isn_counter (wrapping u32), then isn_counter += 1 (wrapping u16);
 *      remote_isn = seq; syn_window = the raw header window; mss = the SYN's last MaximumSegmentSize entry, else
 *      DK_TCP_LSN_FALLBACK_MSS; remote_wscale = its last WindowScale entry, else DK_TCP_LSN_NO_WSCALE; retries_left =
 *      handshake_retries; deadline_ns = now_ns + handshake_timeout_ns; inflight += 1. A SYN+ACK reply, action
 *      SYN_ACCEPTED.
 * crc (isn_generator.rs:28-42, the non-test build) is CRC-32/CKSUM (polynomial 0x04C11DB7, initial value 0, not
 * reflected, final XOR 0xFFFFFFFF; check value 0x765E7680) over 16 bytes: the remote ip's octets, the remote port
 * big-endian, the local ip's octets, the local port big-endian, the nonce big-endian.
 *
 * Replies are the bytes dk_tx_serialize writes for the same descriptor with an empty payload; DK_TX_OFFLOAD_TCP in
 * `flags` writes the TCP checksum as 0 (the reference passes its *rx* checksum-offload setting to
 * serialize_and_attach here, :278 and :388; the caller decides what to pass). Addresses and ports are the frame's,
 * swapped (source = the listener's local_ip / local_port); ip_word is the listener's; the link is link[i] when a
 * per-frame link[] is given and link[i] < nlinks, else the listener's.
 *   SYN+ACK  62 bytes: flags SYN|ACK, seq = local_isn, ack = remote_isn + 1, window = receive_window_size unscaled,
 *            options [MSS(advertised_mss), WindowScale(window_scale)] (a 28-byte TCP header).
 *   RST      54 bytes: flags RST|ACK, window 0. The frame had ACK: seq = its ack_num, ack = ack_num + 1. Otherwise
 *            seq = 0, ack = seq_num + compute_size(), where compute_size() (header.rs:408-421) is taken over the
 *            *parsed* option list: dk_tx_header_bytes(6, opts) - 34, not the received data offset.
 * Replies are numbered in the order of the frames that triggered them; reply f owns slot f under dk_tcp_tx_layout's
 * rule; no byte of out outside the frames is written.
 * The ready list holds one record per ESTABLISHED / ESTABLISHED_DATA / BAD_ACK frame, in the order of those frames
 * (the accept queue's order), with every argument EstablishedSocket::new receives at :457-478: see dk_tcp_lsn_ready.
 *
 * Listener checks, the first that applies (status[l]; the listener's frames are SKIP, nothing of it changes):
 *   E_WSCALE  window_scale > 14 (the reference would panic on the shift)
 *   E_LINK    link >= nlinks
 *   E_SLOT    frame_lead + 62 > slot_stride
 *   E_TABLE   2 x the sum of max_backlog over all rows exceeds the table's cap (every listener reports it, nothing is
 *             done): with the rule kept an insert can never find the table full. The host states the sum as
 *             backlog_sum (EINVAL when it breaks the rule); the device adds the rows up all the same.
 * A CLOSED listener reports OK and its frames are SKIP.
 * Capacity is all or nothing and tested on the device: n_frames and n_ready always report the call's need; if
 * n_frames > max_frames, or n_frames * slot_stride > out_bytes, or n_ready > max_ready, then nothing else is written
 * (no frame, ready record, per-frame result, table field or listener field) and the listeners that had a frame of
 * theirs in the batch report NO_ROOM. There is no host round trip anywhere in the call.
 * The slot a key lands in is not specified (concurrent inserts may win in either order); everything else is.
 *
 * dk_tcp_listen_timers is the handshake timeout (:316-357): every SYN_RCVD slot of a LISTENING listener that passes
 * the checks with deadline_ns <= now_ns either has retries_left > 0: retries_left -= 1, deadline_ns = now_ns +
 * handshake_timeout_ns and the same SYN+ACK goes out again from the slot's fields; or becomes FAILED / ETIMEDOUT with
 * an error ready record (frame = DK_TCP_LSN_NONE). Same builder, same capacity rule. Its frames and records follow
 * slot order, which is unspecified. Per-frame results (action, slot, reply_frame) are not used; frame_seg holds the slot.
 * dk_tcp_listen_release is the socket_queue removal (:144-150): each key present becomes a TOMBSTONE, its listener's
 * inflight goes down by one and found[k] = 1; an absent key gets found[k] = 0 (of two equal keys in one call exactly
 * one is found; which one is not specified). A later
 * insert may claim a tombstone; a lookup walks on across one. Tombstones lengthen walks over time: the count of
 * never-used slots consumed is dk_tcp_listen_table_stats'. Rebuilding a worn table is out of scope.
 *
 * Calls on one table are serialised as a context's calls are; asynchronous on the caller's stream; the environment is
 * never read. These entry points are additive: DK_RX_ABI_VERSION stays 4.
 * Out of scope: turning a ready record into rows of the five TCP tables and an Active socket-table entry on the device
 * (that needs a link and a queue region, which are the host's to give); feeding FORWARD frames to dk_tcp_rx_process
 * before that entry exists; the active open (the dk_tcp_connect_* section below); the closing states (the dk_tcp_close_* section); SYN cookies (the
 * reference has none).
 * ------------------------------------------------------------------------------------------------------------- */
#define DK_TCP_LSN_NONE 0xFFFFFFFFu
#define DK_TCP_LSN_NO_WSCALE 0xFFu
#define DK_TCP_LSN_FALLBACK_MSS 536u         /* FALLBACK_MSS (tcp/constants.rs)                                     */
#define DK_TCP_LSN_MAX_LISTENERS 65535u      /* listener rows 0 .. 65,534: the row is 16 bits of the key            */
#define DK_TCP_LSN_SYNACK_BYTES 62u
#define DK_TCP_LSN_RST_BYTES 54u
#define DK_TCP_LSN_KEY_FREE (~0ull)          /* the key word of a never-used slot                                   */
#define DK_TCP_LSN_KEY_TOMBSTONE (0xFFFFull << 48)

enum dk_tcp_lsn_listener_state { DK_TCP_LSN_CLOSED = 0, DK_TCP_LSN_LISTENING = 1 };

/* One listening socket. Device memory, 16-byte aligned, updated in place (inflight, isn_counter). */
typedef struct dk_tcp_listener {
    uint32_t state;                /* enum dk_tcp_lsn_listener_state                                               */
    uint32_t flow_id;              /* its index in the socket table (informational: lsn_of_flow is what is used)   */
    uint32_t local_ip;             /* octet order, as dk_rx.h                                                      */
    uint16_t local_port;
    uint16_t receive_window_size;  /* TcpConfig::get_receive_window_size                                           */
    uint32_t max_backlog;
    uint32_t nonce;                /* IsnGenerator::nonce                                                          */
    uint16_t advertised_mss;
    uint8_t window_scale;          /* TcpConfig::get_window_scale                                                  */
    uint8_t reserved0;
    uint32_t handshake_retries;
    uint64_t handshake_timeout_ns;
    uint32_t ip_word;              /* dk_tx_segs.ip_word of the replies                                            */
    uint32_t link;                 /* index into links[]                                                           */
    uint32_t inflight;             /* connections.len(): moved by process (up) and release (down)                  */
    uint16_t isn_counter;          /* IsnGenerator::counter                                                        */
    uint16_t reserved1;
    uint64_t reserved2;
} dk_tcp_listener;                 /* 64 bytes */

enum dk_tcp_lsn_slot_state {
    DK_TCP_LSN_FREE = 0,       /* never used: a lookup stops here                                                  */
    DK_TCP_LSN_SYN_RCVD = 1,
    DK_TCP_LSN_ESTAB = 2,
    DK_TCP_LSN_FAILED = 3,     /* err = EBADMSG or ETIMEDOUT                                                       */
    DK_TCP_LSN_TOMBSTONE = 4   /* released: a lookup walks on, an insert may claim it                              */
};

/* One slot of the table, as dk_tcp_listen_table_read / _write move it. key = listener row << 48 | remote_ip << 16 |
 * remote_port (dk_tcp_listen_key); DK_TCP_LSN_KEY_FREE / _TOMBSTONE for slots in those states, whose other fields
 * are zero. */
typedef struct dk_tcp_lsn_slot {
    uint64_t key;
    uint32_t state;          /* enum dk_tcp_lsn_slot_state                                                         */
    uint32_t err;
    uint32_t remote_isn;
    uint32_t local_isn;
    uint16_t syn_window;     /* the SYN's raw header window                                                        */
    uint16_t mss;
    uint8_t remote_wscale;   /* DK_TCP_LSN_NO_WSCALE: the SYN carried none                                         */
    uint8_t reserved0;
    uint16_t reserved1;
    uint32_t retries_left;
    uint32_t reserved2;
    uint64_t deadline_ns;
} dk_tcp_lsn_slot;           /* 48 bytes */

enum dk_tcp_lsn_action {
    DK_TCP_LSN_SKIP = 0,
    DK_TCP_LSN_SYN_ACCEPTED = 1,
    DK_TCP_LSN_ESTABLISHED = 2,
    DK_TCP_LSN_ESTABLISHED_DATA = 3,
    DK_TCP_LSN_BAD_ACK = 4,
    DK_TCP_LSN_FORWARD = 5,
    DK_TCP_LSN_ORPHANED = 6,
    DK_TCP_LSN_RST_FLAGS = 7,
    DK_TCP_LSN_RST_BACKLOG = 8
};

/* A ready-list record: what EstablishedSocket::new gets (:457-478), or the error ready.push(Err(..)) carries. The
 * derived fields are computed for error records too. */
typedef struct dk_tcp_lsn_ready {
    uint32_t listener;
    uint32_t remote_ip;
    uint16_t remote_port;
    uint16_t err;            /* 0, EBADMSG or ETIMEDOUT                                                            */
    uint32_t frame;          /* the triggering batch frame; DK_TCP_LSN_NONE from dk_tcp_listen_timers              */
    uint32_t rcv_nxt;        /* remote_isn + 1                                                                     */
    uint32_t snd_nxt;        /* local_isn + 1                                                                      */
    uint32_t local_window;   /* receive_window_size << local_wscale                                                */
    uint32_t remote_window;  /* syn_window << remote_wscale                                                        */
    uint32_t mss;
    uint8_t local_wscale;    /* the listener's window_scale when the SYN carried a WindowScale option, else 0      */
    uint8_t remote_wscale;   /* the option's value when below 14, else 14; 0 when the SYN carried none             */
    uint16_t reserved0;
    uint32_t slot;           /* the entry's slot: an opaque handle (slot[] of FORWARD frames names the same one)   */
    uint32_t reserved1;
} dk_tcp_lsn_ready;          /* 48 bytes */

enum dk_tcp_lsn_status {
    DK_TCP_LSN_OK = 0,
    DK_TCP_LSN_E_WSCALE = 1,
    DK_TCP_LSN_E_LINK = 2,
    DK_TCP_LSN_E_SLOT = 3,
    DK_TCP_LSN_E_TABLE = 4,
    DK_TCP_LSN_NO_ROOM = 5
};

/* Outputs (device). Per batch frame, [n] (dk_tcp_listen_process only): action (enum dk_tcp_lsn_action), slot (the
 * entry's slot for every action but SKIP, RST_FLAGS and RST_BACKLOG, else DK_TCP_LSN_NONE), reply_frame (its reply's
 * frame index or DK_TCP_LSN_NONE). Per reply, [max_frames]: off_out, len_out (a dk_rx_batch over `out`), frame_seg
 * (optional: the batch frame that triggered it; dk_tcp_listen_timers: the slot). ready: [max_ready]. status: [nl], enum
 * dk_tcp_lsn_status. n_frames, n_ready: one word each, the call's need. */
typedef struct dk_tcp_lsn_results {
    uint8_t* action;
    uint32_t* slot;
    uint32_t* reply_frame;
    uint32_t* off_out;
    uint16_t* len_out;
    uint32_t* frame_seg;
    dk_tcp_lsn_ready* ready;
    uint32_t* status;
    uint32_t* n_frames;
    uint32_t* n_ready;
} dk_tcp_lsn_results;

typedef struct dk_tcp_listen_table dk_tcp_listen_table;

/* The table of `cap` slots (a power of two, at least 2) on `device`, all FREE, with the scratch of the calls on it.
 * Returns 0, EINVAL (null out, cap not a power of two or below 2) or ENOMEM. */
int dk_tcp_listen_table_create(int32_t device, uint32_t cap, dk_tcp_listen_table** out);
void dk_tcp_listen_table_destroy(dk_tcp_listen_table* t);
/* cap and the never-used slots consumed so far (either pointer may be null). Synchronous: waits for the table's calls.
 * Returns 0, EINVAL or EIO. */
int dk_tcp_listen_table_stats(dk_tcp_listen_table* t, uint32_t* cap, uint64_t* consumed);
/* Copy the slots out to / in from rows[cap] (host memory). Synchronous: waits for the table's calls. _write recounts
 * the consumed slots (those whose state is not FREE); the rows' placement is the caller's responsibility (a key must
 * be reachable from its home slot across non-FREE slots). Returns 0, EINVAL or EIO. */
int dk_tcp_listen_table_read(dk_tcp_listen_table* t, dk_tcp_lsn_slot* rows);
int dk_tcp_listen_table_write(dk_tcp_listen_table* t, const dk_tcp_lsn_slot* rows);

/* Pure host functions. The key word of (listener row, remote ip in octet order, remote port); the slot a key's probe
 * walk starts at in a table of `cap` slots (the walk goes on to the next slot, modulo cap), so tests can craft
 * collisions; the backlog rule: 0 when 2 * backlog_sum <= cap, else EINVAL. */
uint64_t dk_tcp_listen_key(uint32_t listener, uint32_t remote_ip, uint16_t remote_port);
uint32_t dk_tcp_listen_home(uint32_t cap, uint64_t key);
int dk_tcp_listen_backlog_fits(uint32_t cap, uint64_t backlog_sum);

/* rx = the results of the batch's dk_rx_process call (meta, src_ip, ports, payload, flow_id, tcp_seq, tcp_ack, tcp_win
 * and tcp_opts are required), n its frames; listeners[0 .. nl) with nl <= DK_TCP_LSN_MAX_LISTENERS; link optional.
 * Returns 0, EINVAL (a null required pointer, misaligned listeners, nl too large, n >= 2^31, out_bytes >
 * DK_RX_MAX_BLOB, nlinks == 0, the backlog rule: all before any GPU work), ENOMEM or EIO. n == 0 and nl == 0 are valid
 * calls. */
int dk_tcp_listen_process(dk_tcp_listen_table* t, const dk_rx_results* rx, uint32_t n, dk_tcp_listener* listeners,
                          uint32_t nl, uint64_t backlog_sum, const uint32_t* lsn_of_flow, uint32_t nflows,
                          const uint32_t* link, const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns, uint8_t* out,
                          uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready,
                          uint32_t flags, const dk_tcp_lsn_results* results, void* stream);

/* Returns as dk_tcp_listen_process (backlog_sum is checked on the host only: the call inserts nothing).
 * results->action, slot and reply_frame are not used. */
int dk_tcp_listen_timers(dk_tcp_listen_table* t, const dk_tcp_listener* listeners, uint32_t nl, uint64_t backlog_sum,
                         const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns, uint8_t* out, uint64_t out_bytes,
                         const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready, uint32_t flags,
                         const dk_tcp_lsn_results* results, void* stream);

/* keys[0 .. nkeys): device array of key words; found[nkeys]: device. Returns 0, EINVAL or EIO. */
int dk_tcp_listen_release(dk_tcp_listen_table* t, dk_tcp_listener* listeners, uint32_t nl, const uint64_t* keys,
                          uint32_t nkeys, uint32_t* found, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The active open: what TcpPeer::connect (peer.rs:149-179) and SharedActiveOpenSocket (active_open.rs: process_ack
 * :101-223, connect :225-294, close :296-298) do for a connecting socket, from the ISN to the arguments of
 * EstablishedSocket::new. A connecting socket is a row of dk_tcp_connector in device memory; there is no hash table:
 * the socket table already maps the 4-tuple to a flow id (a DK_FLOW_TCP_ACTIVE entry), and conn_of_flow[nflows] maps a
 * flow id to its connector row, DK_TCP_CON_NONE for every other flow. The peer's one IsnGenerator (peer.rs:171) is a
 * dk_tcp_isn_gen in device memory.
 *
 * dk_tcp_connect_start is connect() up to its first await. start[0 .. nstart) names rows in connect-call order. Entry k
 * takes the counter value counter + k (wrapping u16) whatever becomes of its row (the reference generates the ISN before
 * anything can fail), and the generator ends at counter + nstart. local_isn = crc + that value (wrapping u32), crc being
 * the CRC-32/CKSUM of the listen section over the same 16 bytes: the remote ip's octets, the remote port big-endian, the
 * local ip's octets, the local port big-endian, the nonce big-endian. Row checks, the first that applies (status[k]; a
 * row that fails one is left untouched):
 *   E_ROW     start[k] >= nrows
 *   E_STATE   the row is not IDLE, or an earlier entry of start[] names the same row (the lowest k wins)
 *   E_WSCALE  window_scale > 14
 *   E_LINK    link >= nlinks
 *   E_SLOT    frame_lead + 62 > slot_stride
 * A row with handshake_retries == 0 sends nothing: it becomes FAILED / ECONNREFUSED (the loop body never runs, this is
 * connect()'s last line) with an error ready record of cause EXHAUSTED. Every other row becomes CONNECTING with
 * local_isn set, syns_left = handshake_retries - 1 and deadline_ns = now_ns + handshake_timeout_ns, and a SYN goes out.
 * handshake_retries therefore counts SYNs in all, as in the reference (connect-refused.pkt: 5 gives five SYNs).
 * SYNs are numbered in start[] order; frame_seg holds k, and so does `frame` of the error records. The per-frame
 * results (action, row, reply_frame) are not used.
 *
 * dk_tcp_connect_process covers the frames of one dk_rx_process batch with verdict DK_V_OK_TCP whose flow_id maps to a
 * connector row; every other frame gets action SKIP. Frames are taken in arrival order per row, and each coroutine is
 * taken to have run to its next await before the next frame arrives (the listen section's assumption). By the row's
 * state:
 *   CONNECTING   process_ack (:101-126), in its order:
 *                  1. !(ack && ack_num == local_isn + 1): EAGAIN
 *                  2. rst: refused (a RST whose ack does not match is only an EAGAIN; SYN+RST with a matching ack is
 *                     refused)
 *                  3. !syn: EAGAIN
 *                  4. otherwise accepted.
 *                EAGAIN is the loop's `continue`, the same as a timeout: with syns_left > 0 a SYN goes out again,
 *                syns_left -= 1, deadline_ns = now_ns + handshake_timeout_ns, action RETRY_SYN; with syns_left == 0 the
 *                row becomes FAILED / ECONNREFUSED, action EXHAUSTED, an error ready record of cause EXHAUSTED, no reply.
 *                That a stray segment costs a retry is the reference's quirk; it is kept.
 *                Refused: FAILED / ECONNREFUSED, action REFUSED, an error ready record of cause RST, no reply.
 *                Accepted: action ESTABLISHED, the row becomes ESTABLISHED, the handshake ACK goes out and a ready
 *                record is appended. A payload on the SYN+ACK is dropped: connect() discards the buffer (:276), unlike
 *                the passive side.
 *   ESTABLISHED  (already, or by an earlier frame of this batch) action FORWARD: recv_queue is shared with the
 *                established socket, the host routes the frame by row[].
 *   FAILED       (already, or earlier in this batch) action ORPHANED: the reference removes the address entry, which is
 *                the host's job.
 *   IDLE, CLOSED SKIP. A host that closes a connecting socket (close(), ECONNABORTED) writes state = CLOSED between
 *                calls; no entry point is needed.
 * Negotiation (:150-194), in the ready record: mss = the frame's last MaximumSegmentSize entry, else
 * DK_TCP_CON_FALLBACK_MSS; with a WindowScale entry remote_wscale = the last one's value capped at 14 and local_wscale =
 * window_scale, without one both are 0; local_window = receive_window_size << local_wscale; remote_window = the header
 * window << remote_wscale. The reference passes congestion_control::None::new here (:218): the host chooses the CC row,
 * as it does after a passive open.
 * Frames are the bytes dk_tx_serialize writes for the same descriptor with an empty payload; DK_TX_OFFLOAD_TCP in
 * `flags` writes the TCP checksum as 0, as in the listen section. Source = the row's local address, destination its
 * remote; ip_word is the row's; the link is link[i] when a per-frame link[] is given and link[i] < nlinks
 * (dk_tcp_connect_process only), else the row's.
 *   SYN  62 bytes: flags SYN, seq = local_isn, ack 0, window = receive_window_size, options [MSS(advertised_mss),
 *        WindowScale(window_scale)].
 *   ACK  54 bytes: flags ACK, seq = local_isn + 1, ack = seq_num + 1, window = receive_window_size unscaled, no options.
 * Replies are numbered in the order of the frames that triggered them; reply f owns slot f under dk_tcp_tx_layout's
 * rule; no byte of out outside the frames is written. Ready records follow the order of the frames that made them.
 * status[r], r < nrows: a CONNECTING row reports the first of E_WSCALE, E_LINK, E_SLOT that applies (its frames are
 * SKIP, nothing of it changes); every other row reports OK.
 *
 * dk_tcp_connect_timers is the pop's timeout (:275, :281): every CONNECTING row that passes the checks with deadline_ns
 * <= now_ns takes the EAGAIN step above. Frames and ready records come in ascending row order; frame_seg holds the row,
 * `frame` of the records is DK_TCP_CON_NONE. The per-frame results are not used; status[] as in dk_tcp_connect_process.
 *
 * Capacity is all or nothing and tested on the device, in all three calls: n_frames and n_ready always report the
 * call's need; if n_frames > max_frames, or n_frames * slot_stride > out_bytes, or n_ready > max_ready, then nothing
 * else is written (no frame, record, per-frame result, row field or generator field) and NO_ROOM is reported by the
 * rows that had a frame other than SKIP (process), the rows that were due (timers), the entries that passed their
 * checks (start). There is no host round trip anywhere in a call.
 * The outcome for a row in dk_tcp_connect_process is a function of the index of its first refused / accepted frame, the
 * arrival rank of its EAGAIN frames before that, and syns_left. A count and a 32-bit minimum per row settle the rows
 * with one frame, a second count and minimum the rows with two frames up to that first refused / accepted one; the
 * frames of rows with three or more are compacted in frame order and ranked per row exactly, for any number of frames
 * per row: a wave groups each 64 of them by row, the groups of a row are chained, and a group's base is the sum over
 * the row's groups before it. The memory is a word per row and a few per frame.
 *
 * The calls take their scratch from one per-device pool of the library (the current device's) and are serialised on it
 * as a context's calls are; asynchronous on the caller's stream; the environment is never read. These entry points are
 * additive: DK_RX_ABI_VERSION stays 4.
 * Out of scope: the ephemeral-port allocator and the socket table's Active entry (the host's, before
 * dk_tcp_connect_start) and its removal on failure; ARP resolution before the first SYN (include/dk_arp.h: a resolved dk_arp_query writes the
 * destination MAC into links[], which dk_tcp_connect_start then takes unread by the host); building the rows of the five
 * TCP tables on the device; the closing states (the dk_tcp_close_* section); simultaneous open (the reference has none).
 * ------------------------------------------------------------------------------------------------------------- */
#define DK_TCP_CON_NONE 0xFFFFFFFFu
#define DK_TCP_CON_FALLBACK_MSS 536u         /* FALLBACK_MSS (tcp/constants.rs)                                     */
#define DK_TCP_CON_SYN_BYTES 62u
#define DK_TCP_CON_ACK_BYTES 54u

enum dk_tcp_con_state {
    DK_TCP_CON_IDLE = 0,        /* bound to its addresses, not yet started                                          */
    DK_TCP_CON_CONNECTING = 1,
    DK_TCP_CON_ESTAB = 2,
    DK_TCP_CON_FAILED = 3,      /* err = ECONNREFUSED                                                               */
    DK_TCP_CON_CLOSED = 4       /* written by the host: close() while connecting                                    */
};

/* One connecting socket. Device memory, 16-byte aligned, updated in place (state, err, local_isn, syns_left,
 * deadline_ns). */
typedef struct dk_tcp_connector {
    uint16_t state;                /* enum dk_tcp_con_state                                                        */
    uint16_t err;                  /* 0 or ECONNREFUSED                                                            */
    uint32_t flow_id;              /* its index in the socket table (informational: conn_of_flow is what is used)  */
    uint32_t local_ip;             /* octet order, as dk_rx.h                                                      */
    uint32_t remote_ip;
    uint16_t local_port;
    uint16_t remote_port;
    uint32_t local_isn;            /* written by dk_tcp_connect_start                                              */
    uint16_t receive_window_size;  /* TcpConfig::get_receive_window_size                                           */
    uint16_t advertised_mss;
    uint8_t window_scale;          /* TcpConfig::get_window_scale                                                  */
    uint8_t reserved0;
    uint16_t reserved1;
    uint32_t handshake_retries;    /* SYNs in all                                                                  */
    uint32_t syns_left;            /* SYNs the loop may still send                                                 */
    uint64_t handshake_timeout_ns;
    uint64_t deadline_ns;          /* the pending pop's timeout                                                    */
    uint32_t ip_word;              /* dk_tx_segs.ip_word of the frames                                             */
    uint32_t link;                 /* index into links[]                                                           */
} dk_tcp_connector;                /* 64 bytes */

/* The peer's IsnGenerator. Device memory, 8-byte aligned. */
typedef struct dk_tcp_isn_gen {
    uint32_t nonce;
    uint16_t counter;
    uint16_t reserved;
} dk_tcp_isn_gen;

enum dk_tcp_con_action {
    DK_TCP_CON_SKIP = 0,
    DK_TCP_CON_ESTABLISHED = 1,
    DK_TCP_CON_RETRY_SYN = 2,
    DK_TCP_CON_EXHAUSTED = 3,
    DK_TCP_CON_REFUSED = 4,
    DK_TCP_CON_FORWARD = 5,
    DK_TCP_CON_ORPHANED = 6
};

enum dk_tcp_con_cause { DK_TCP_CON_CAUSE_NONE = 0, DK_TCP_CON_CAUSE_RST = 1, DK_TCP_CON_CAUSE_EXHAUSTED = 2 };

/* A ready record: what EstablishedSocket::new gets (:201-222), or the error connect() returns. An error record carries
 * row, err, cause, frame and snd_nxt; its other fields are 0. */
typedef struct dk_tcp_con_ready {
    uint32_t row;
    uint16_t err;            /* 0 or ECONNREFUSED                                                                  */
    uint16_t cause;          /* enum dk_tcp_con_cause                                                              */
    uint32_t frame;          /* the triggering batch frame; the start[] entry (dk_tcp_connect_start); DK_TCP_CON_NONE
                                from dk_tcp_connect_timers                                                         */
    uint32_t rcv_nxt;        /* seq_num + 1                                                                        */
    uint32_t snd_nxt;        /* local_isn + 1                                                                      */
    uint32_t local_window;   /* receive_window_size << local_wscale                                                */
    uint32_t remote_window;  /* the SYN+ACK's header window << remote_wscale                                       */
    uint32_t mss;
    uint8_t local_wscale;
    uint8_t remote_wscale;
    uint16_t reserved0;
    uint32_t reserved1;
    uint64_t reserved2;
} dk_tcp_con_ready;          /* 48 bytes */

enum dk_tcp_con_status {
    DK_TCP_CON_OK = 0,
    DK_TCP_CON_E_ROW = 1,
    DK_TCP_CON_E_STATE = 2,
    DK_TCP_CON_E_WSCALE = 3,
    DK_TCP_CON_E_LINK = 4,
    DK_TCP_CON_E_SLOT = 5,
    DK_TCP_CON_NO_ROOM = 6
};

/* Outputs (device). Per batch frame, [n] (dk_tcp_connect_process only): action (enum dk_tcp_con_action), row (the
 * connector row for every action but SKIP, else DK_TCP_CON_NONE), reply_frame (its reply's frame index or
 * DK_TCP_CON_NONE). Per reply, [max_frames]: off_out, len_out (a dk_rx_batch over `out`), frame_seg (optional: see each
 * call). ready: [max_ready]. status: [nrows] (dk_tcp_connect_start: [nstart]), enum dk_tcp_con_status. n_frames,
 * n_ready: one word each, the call's need. */
typedef struct dk_tcp_con_results {
    uint8_t* action;
    uint32_t* row;
    uint32_t* reply_frame;
    uint32_t* off_out;
    uint16_t* len_out;
    uint32_t* frame_seg;
    dk_tcp_con_ready* ready;
    uint32_t* status;
    uint32_t* n_frames;
    uint32_t* n_ready;
} dk_tcp_con_results;

/* start[0 .. nstart): device array of row indices. Returns 0, EINVAL (a null required pointer, misaligned rows or
 * isn_gen, nstart >= 2^31, out_bytes > DK_RX_MAX_BLOB, nlinks == 0: all before any GPU work), ENOMEM or EIO. nstart == 0
 * and nrows == 0 are valid calls. */
int dk_tcp_connect_start(dk_tcp_connector* rows, uint32_t nrows, const uint32_t* start, uint32_t nstart,
                         dk_tcp_isn_gen* isn_gen, const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns, uint8_t* out,
                         uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready,
                         uint32_t flags, const dk_tcp_con_results* results, void* stream);

/* rx = the results of the batch's dk_rx_process call (meta, flow_id, tcp_seq, tcp_ack, tcp_win and tcp_opts are
 * required), n its frames; link optional. Returns as dk_tcp_connect_start (n >= 2^31 is EINVAL). n == 0 and nrows == 0
 * are valid calls. */
int dk_tcp_connect_process(const dk_rx_results* rx, uint32_t n, dk_tcp_connector* rows, uint32_t nrows,
                           const uint32_t* conn_of_flow, uint32_t nflows, const uint32_t* link, const dk_tx_link* links,
                           uint32_t nlinks, uint64_t now_ns, uint8_t* out, uint64_t out_bytes,
                           const dk_tcp_tx_layout* layout, uint32_t max_frames, uint32_t max_ready, uint32_t flags,
                           const dk_tcp_con_results* results, void* stream);

/* Returns as dk_tcp_connect_start. results->action, row and reply_frame are not used. */
int dk_tcp_connect_timers(dk_tcp_connector* rows, uint32_t nrows, const dk_tx_link* links, uint32_t nlinks,
                          uint64_t now_ns, uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout,
                          uint32_t max_frames, uint32_t max_ready, uint32_t flags, const dk_tcp_con_results* results,
                          void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Closing a connection: ControlBlock::close with local_close and remote_already_closed (established/ctrlblk.rs:
 * 1039-1119), for every closing connection of a batch at once. A closing connection is a row of dk_tcp_closer in device
 * memory, indexed by flow id like the five TCP tables. Sending the FIN (a zero-length push through dk_tcp_tx_segment,
 * queued by dk_tcp_tx_commit, resent by dk_tcp_retransmit) and receiving one in ESTABLISHED (dk_tcp_rx_process's
 * DK_TCP_FIN, acknowledged by dk_tcp_ack_emit) exist already; this section is the coroutine that pops recv_queue itself
 * once poll() has stopped (:350-372): no window check, no RST or SYN check, no data processing.
 *
 * dk_tcp_close_start is close() up to its first await (:1040-1057). close[0 .. nclose) names connections. Per entry k,
 * the first of these that applies gives status[k] (a rejected entry changes nothing):
 *   E_ROW    close[k] >= nconns
 *   E_ORDER  close[k] <= the maximum of close[0 .. k): the list must be strictly ascending, because the marker list it
 *            yields must have non-decreasing conn
 *   E_STATE  tx_conns[c].state != DK_TCP_ESTABLISHED
 *   E_BADF   the row is not IDLE, or rx_conns[c].state is DK_TCP_NONE ("socket is already closing", EBADF)
 * An accepted entry whose rx state is ESTABLISHED makes the row FIN_WAIT_1 and sets rx_conns[c].state = DK_TCP_CLOSED,
 * as poll() has returned; one whose rx state is CLOSED (a FIN or an RST was received earlier: CloseWait) makes the row
 * LAST_ACK. err = 0, flags = 0, deadline_ns = 0; linger_ns is the caller's input. The accepted connections are written
 * to push_conn[0 .. *n_markers) in order with push_off = push_len = 0; the tail up to nclose is padded with conn =
 * 0xFFFFFFFF, off = len = 0. The three arrays with nbufs = nclose are a valid dk_tcp_tx_push for dk_tcp_tx_segment: the
 * padding reports DK_TCP_TX_E_CONN and sends nothing, so the FIN goes out without the host reading a status. Merging the
 * markers into a call that also carries data stays with the caller.
 *
 * dk_tcp_close_process covers the frames of one dk_rx_process batch with verdict DK_V_OK_TCP whose flow id is below
 * nconns and whose row is in FIN_WAIT_1, FIN_WAIT_2, CLOSING or LAST_ACK (a live row) and passes the row checks; every
 * other frame is SKIP (action 0). Row checks, the first that applies (status[c]; the row's frames are SKIP and nothing of
 * it changes; every row that is not live reports OK):
 *   E_RX_STATE  rx_conns[c].state != DK_TCP_CLOSED
 *   E_STATE     tx_conns[c].state != DK_TCP_ESTABLISHED
 *   E_LINK, E_WSCALE, E_WINDOW, E_SLOT  exactly as dk_tcp_ack_emit states them
 * A live row's frames are taken in arrival order. snd_nxt = tx_conns[c].snd_nxt does not move during a call, so three
 * bits of the frame alone decide: A = ACK set and ack <= snd_nxt (the sign of the wrapping difference), U = ACK set and
 * ack > snd_nxt, F = FIN. Per popped frame, process_ack (:607-650) first: A is Ok, U sends an ACK of ours and is Err, no
 * ACK bit is Err; then, in the local_close loop and also after an Err, process_remote_close (:1003-1026):
 *   state before  A  F  state after  side effects
 *   FIN_WAIT_1    0  0  FIN_WAIT_1   an ACK of ours if U
 *   FIN_WAIT_1    1  0  FIN_WAIT_2   ACK-processed
 *   FIN_WAIT_1    0  1  CLOSING      an ACK if U; FIN consumed
 *   FIN_WAIT_1    1  1  TIME_WAIT    ACK-processed; FIN consumed
 *   FIN_WAIT_2    x  0  FIN_WAIT_2   ACK-processed if A; an ACK if U
 *   FIN_WAIT_2    x  1  TIME_WAIT    as above; FIN consumed
 *   CLOSING       0  0  CLOSING      an ACK if U
 *   CLOSING       1  0  TIME_WAIT    ACK-processed
 *   CLOSING       x  1  FAULT        the deviation below
 *   LAST_ACK      0  x  LAST_ACK     an ACK if U; F ignored
 *   LAST_ACK      1  x  CLOSED       ACK-processed; F ignored
 * Two quirks of the reference are kept: any acceptable ACK takes FIN_WAIT_1 to FIN_WAIT_2, whether or not it covers our
 * FIN; and the FIN's sequence number is not looked at. TIME_WAIT, CLOSED and FAULT end the row's loop: its later frames
 * of the batch are never popped (action UNPROCESSED). "FIN consumed" is RCV.NXT += 1 and one ACK of ours carrying the
 * new RCV.NXT; a consumed frame with U sends two ACKs, the first with the old RCV.NXT. A row changes state at most twice
 * in a call and RCV.NXT moves at most once.
 * One stated deviation: CLOSING + F panics the reference (unreachable!, :1087) after process_remote_close has run its
 * side effects. Here that frame gets action FAULT alone and nothing of it is applied: no ACK, RCV.NXT stays, its
 * ack_action is DK_TCP_UNPROCESSED; the row becomes DK_TCP_CLS_FAULT with err = EPROTO and a done record is appended.
 * Per-frame outputs: action (the DK_TCP_CLS_* bits below), state_after (the row's state after a popped or FAULT frame,
 * its final state for an UNPROCESSED one, 0 for SKIP), reply_frame (the index of the frame's first ACK, or
 * DK_TCP_CLS_NONE), and ack_action in enum dk_tcp_action codes: the array to hand to dk_tcp_cc_ack and
 * dk_tcp_ack_process in place of the receive call's `action`, so that those kernels do the rest of process_ack
 * (on_ack_received, SND.UNA, the send window, the unacknowledged queue with the FIN marker's pop, the RTT sample and the
 * retransmit deadline). A popped frame gets DK_TCP_NO_DATA for A, DK_TCP_ACK_UNSENT for U, DK_TCP_NO_ACK for neither; a
 * frame of a live row that was not popped gets DK_TCP_UNPROCESSED; every other frame copies action_in[i] (that batch's
 * dk_tcp_out.action), or is DK_TCP_SKIP without action_in. dk_tcp_ack_emit keeps getting the original action: the two
 * arrays are distinct. Both of those calls take `action` as a plain input and order the frames from the context's
 * scratch, which holds the frames of CLOSED connections too.
 * ACKs of ours are the 54-byte frame dk_tcp_ack_emit builds: seq = tx_conns[c].snd_nxt, ack = RCV.NXT and window =
 * (buffer_size - (RCV.NXT - reader_next)) >> rcv_wscale as they stood at that moment, DK_TX_OFFLOAD_TCP honoured. They
 * are numbered in the order of the triggering frames, within a frame the U ACK before the FIN ACK; reply f owns slot f
 * under dk_tcp_tx_layout's rule; no byte of out outside the frames is written.
 * Row effects: state and err; deadline_ns = now_ns + linger_ns (wrapping) on entering TIME_WAIT;
 * rx_conns[c].receive_next += 1 on a consumed FIN; dack[c].armed = 0 (when dack is given) for a row that sent any ACK
 * (emit, :761); fin_frame[c] = the frame whose FIN was consumed, else DK_TCP_CLS_NONE, for every row; one done record
 * per row that reached TIME_WAIT, CLOSED or FAULT, in the order of the triggering frames. tx_conns is only read:
 * retiring the connection here would make the dk_tcp_ack_process that follows reject it.
 * A row's loop ends after at most two transitions, and each is "the first frame after index t that triggers one from
 * state s": one classify pass computes row and A / U / F, at most two rounds of a 32-bit minimum per row find the two
 * frames exactly for any number of frames per row, and every frame's state-before follows from comparing its index with
 * them. No sort is needed.
 *
 * dk_tcp_close_timers is TIME-WAIT's end (yield_with_timeout(linger.unwrap_or(2 * MSL)), :1096-1098) and the retiring
 * of closed rows: every TIME_WAIT row with deadline_ns <= now_ns becomes CLOSED; every CLOSED row without
 * DK_TCP_CLS_RETIRED gets it, a done record (frame and fin_frame DK_TCP_CLS_NONE) in ascending row order and, with
 * tx_conns given, tx_conns[c].state = DK_TCP_CLOSED. status[c] is OK, or NO_ROOM for the rows that had a record.
 *
 * Capacity is all or nothing and tested on the device: n_frames and n_done always report the call's need; if n_frames >
 * max_frames, or n_frames * slot_stride > out_bytes, or n_done > max_done, nothing else is written and the rows that had
 * work (a live row with a frame in the batch; a row with a record) report NO_ROOM.
 * The calls take their scratch from a per-device pool of their own and are serialised on it as the connect section's
 * are; asynchronous on the caller's stream; the environment is never read. These entry points are additive:
 * DK_RX_ABI_VERSION stays 4.
 * Out of scope: re-presenting the segments an earlier batch left UNPROCESSED (the reference pops them from recv_queue
 * first; here the host hands them in again); data received in FIN-WAIT (the reference has a TODO there); removing the
 * socket-table entry and the listener's close queue; RST generation.
 * ------------------------------------------------------------------------------------------------------------- */
#define DK_TCP_CLS_NONE 0xFFFFFFFFu
#define DK_TCP_CLS_TIME_WAIT_NS 4000000000ull /* 2 * MSL, MSL = 2 s (runtime/network/consts.rs:25)                  */
#define DK_TCP_CLS_RETIRED 1u                 /* dk_tcp_closer.flags: dk_tcp_close_timers has reported the row      */
#define DK_TCP_CLS_ACK_BYTES 54u

enum dk_tcp_cls_state {
    DK_TCP_CLS_IDLE = 0,
    DK_TCP_CLS_FIN_WAIT_1 = 1,
    DK_TCP_CLS_FIN_WAIT_2 = 2,
    DK_TCP_CLS_CLOSING = 3,
    DK_TCP_CLS_TIME_WAIT = 4,
    DK_TCP_CLS_LAST_ACK = 5,
    DK_TCP_CLS_CLOSED = 6,
    DK_TCP_CLS_FAULT = 7        /* err = EPROTO                                                                      */
};

/* One closing connection. Device memory, 16-byte aligned, updated in place (state, err, flags, deadline_ns). */
typedef struct dk_tcp_closer {
    uint16_t state;        /* enum dk_tcp_cls_state                                                                 */
    uint16_t err;          /* 0 or EPROTO                                                                           */
    uint32_t flags;        /* DK_TCP_CLS_RETIRED                                                                    */
    uint64_t linger_ns;    /* TIME-WAIT's length (input): the socket's linger, else DK_TCP_CLS_TIME_WAIT_NS         */
    uint64_t deadline_ns;  /* TIME-WAIT's end                                                                       */
    uint64_t reserved;
} dk_tcp_closer;           /* 32 bytes */

/* A done record: a row reached TIME_WAIT, CLOSED or FAULT (dk_tcp_close_process), or was retired
 * (dk_tcp_close_timers). */
typedef struct dk_tcp_cls_done {
    uint32_t row;
    uint16_t state;        /* enum dk_tcp_cls_state                                                                 */
    uint16_t err;
    uint32_t frame;        /* the triggering batch frame; DK_TCP_CLS_NONE from dk_tcp_close_timers                  */
    uint32_t fin_frame;    /* the frame whose FIN was consumed in this call, or DK_TCP_CLS_NONE                     */
    uint64_t deadline_ns;  /* the row's, after the call                                                             */
    uint64_t reserved;
} dk_tcp_cls_done;         /* 32 bytes */

/* dk_tcp_cls_results.action, a bit set; 0 is SKIP. */
#define DK_TCP_CLS_POPPED 1u       /* the coroutine popped the frame                                                */
#define DK_TCP_CLS_ACK_OK 2u       /* A: process_ack returned Ok                                                    */
#define DK_TCP_CLS_ACK_UNSENT 4u   /* U: an ACK of ours went out                                                    */
#define DK_TCP_CLS_FIN 8u          /* the frame's FIN was consumed                                                  */
#define DK_TCP_CLS_FAULT_BIT 16u   /* CLOSING + F: nothing of the frame applied, the row is FAULT                   */
#define DK_TCP_CLS_UNPROCESSED 32u /* a live row's frame behind the frame that ended its loop                       */

enum dk_tcp_cls_status {
    DK_TCP_CLS_OK = 0,
    DK_TCP_CLS_E_ROW = 1,
    DK_TCP_CLS_E_ORDER = 2,
    DK_TCP_CLS_E_STATE = 3,
    DK_TCP_CLS_E_BADF = 4,
    DK_TCP_CLS_E_RX_STATE = 5,
    DK_TCP_CLS_E_LINK = 6,
    DK_TCP_CLS_E_WSCALE = 7,
    DK_TCP_CLS_E_WINDOW = 8,
    DK_TCP_CLS_E_SLOT = 9,
    DK_TCP_CLS_NO_ROOM = 10
};

/* Outputs (device). Per batch frame, [n] (dk_tcp_close_process only): action, state_after, ack_action (one byte each),
 * reply_frame. Per reply, [max_frames]: off_out, len_out (a dk_rx_batch over `out`), frame_seg (optional: the batch
 * frame that triggered it). done: [max_done]. Per row, [nconns]: status (enum dk_tcp_cls_status), fin_frame
 * (dk_tcp_close_process only). n_frames, n_done: one word each, the call's need. */
typedef struct dk_tcp_cls_results {
    uint8_t* action;
    uint8_t* state_after;
    uint8_t* ack_action;
    uint32_t* reply_frame;
    uint32_t* off_out;
    uint16_t* len_out;
    uint32_t* frame_seg;
    dk_tcp_cls_done* done;
    uint32_t* status;
    uint32_t* fin_frame;
    uint32_t* n_frames;
    uint32_t* n_done;
} dk_tcp_cls_results;

/* close[0 .. nclose), status[nclose], push_conn / push_off / push_len [nclose] and the word n_markers are device
 * arrays. Returns 0, EINVAL (a null required pointer, rows / rx_conns / tx_conns not 16-byte aligned, nclose >= 2^31:
 * all before any GPU work), ENOMEM or EIO. nclose == 0 and nconns == 0 are valid calls that write n_markers = 0. */
int dk_tcp_close_start(dk_tcp_closer* rows, dk_tcp_conn* rx_conns, const dk_tcp_tx_conn* tx_conns, uint32_t nconns,
                       const uint32_t* close, uint32_t nclose, uint32_t* status, uint32_t* push_conn, uint32_t* push_off,
                       uint32_t* push_len, uint32_t* n_markers, void* stream);

/* rx = the results of the batch's dk_rx_process call (meta, flow_id, tcp_seq and tcp_ack are required), n its frames;
 * dack and action_in optional. Returns 0, EINVAL (a null required pointer, a misaligned table, n >= 2^31, out_bytes >
 * DK_RX_MAX_BLOB, nlinks == 0: all before any GPU work), ENOMEM or EIO. n == 0 and nconns == 0 are valid calls. */
int dk_tcp_close_process(const dk_rx_results* rx, uint32_t n, dk_tcp_closer* rows, dk_tcp_conn* rx_conns,
                         const dk_tcp_tx_conn* tx_conns, dk_tcp_dack_conn* dack, uint32_t nconns,
                         const uint8_t* action_in, const dk_tx_link* links, uint32_t nlinks, uint64_t now_ns,
                         uint8_t* out, uint64_t out_bytes, const dk_tcp_tx_layout* layout, uint32_t max_frames,
                         uint32_t max_done, uint32_t flags, const dk_tcp_cls_results* results, void* stream);

/* tx_conns optional. status: [nconns]. Returns 0, EINVAL (a null required pointer, a misaligned table), ENOMEM or EIO. */
int dk_tcp_close_timers(dk_tcp_closer* rows, dk_tcp_tx_conn* tx_conns, uint32_t nconns, uint64_t now_ns,
                        dk_tcp_cls_done* done, uint32_t max_done, uint32_t* n_done, uint32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DK_TCP_H */
