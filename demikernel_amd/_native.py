"""ctypes binding of include/dk_rx.h (libdk_rx.so, built in-tree for gfx950 by __graft_entry__.build()).

No fallback: if the HIP library is missing, importing the engine raises. The structures below mirror the C header
field for field; tests/test_abi.py checks their sizes and that every function the header declares is exported.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_int, c_int32, c_uint8, c_uint16, c_uint32, c_uint64, c_void_p

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libdk_rx.so")  # tuning builds (tools/variants.sh) are passed as lib_path explicitly

DK_FLOW_NONE = 0xFFFFFFFF
DK_TX_NOT_WRITTEN = 0xFFFF  # dk_tx_checksum_fields: a checksum half the in-place fill leaves untouched
DK_RX_BATCH_ALIGNED16 = 1  # dk_rx_batch.flags
DK_RX_BATCH_DEFER_COUNTS = 2
DK_RX_MAX_DEFERRED_FLOWS = 32768  # flow_counts defer only for tables up to this size (dk_rx.h)
DK_FLOW_TCP_ACTIVE, DK_FLOW_TCP_PASSIVE, DK_FLOW_UDP = 1, 2, 3

# enum dk_verdict (include/dk_rx.h), SURVEY.md Appendix A.
VERDICTS = [
    "OK_TCP", "OK_UDP", "ARP", "ICMP", "IPV6", "ETH_SHORT", "ETH_TYPE", "IP_SHORT", "IP_VERSION", "IP_IHL_SMALL",
    "IP_HDR_TRUNC", "IP_TOTLEN_SMALL", "IP_TOTLEN_BIG", "IP_EVIL", "IP_MF", "IP_FRAGOFF", "IP_TTL", "IP_PROTO",
    "IP_CSUM_FFFF", "IP_CSUM", "IP_DST", "IP_SRC", "TCP_SHORT", "TCP_DOFF_TRUNC", "TCP_DOFF_SMALL", "TCP_CSUM",
    "TCP_OPT", "TCP_OPT_EIO", "TCP_NOSOCK", "UDP_SHORT", "UDP_LEN", "UDP_CSUM", "UDP_NOSOCK", "BAD_DESC",
    "ARP_SHORT", "ARP_UNSUP", "ICMP_SHORT", "ICMP_CSUM", "ICMP_TYPE",
]
V = {name: i for i, name in enumerate(VERDICTS)}
DK_V_COUNT = len(VERDICTS)

# numpy mirror of struct dk_flow (16 bytes).
FLOW_DTYPE = np.dtype([("kind", "<u4"), ("local_ip", "<u4"), ("remote_ip", "<u4"),
                       ("local_port", "<u2"), ("remote_port", "<u2")])
assert FLOW_DTYPE.itemsize == 16


class DkRxCfg(ctypes.Structure):
    _fields_ = [("local_ipv4", c_uint32), ("tcp_rx_checksum_offload", c_uint8),
                ("udp_rx_checksum_offload", c_uint8), ("reserved", c_uint16), ("device", c_int32)]


class DkFlow(ctypes.Structure):
    _fields_ = [("kind", c_uint32), ("local_ip", c_uint32), ("remote_ip", c_uint32),
                ("local_port", c_uint16), ("remote_port", c_uint16)]


class DkRxBatch(ctypes.Structure):
    _fields_ = [("frames", c_void_p), ("frames_bytes", c_uint64), ("off", c_void_p), ("len", c_void_p),
                ("n", c_uint32), ("flags", c_uint32)]


RESULT_FIELDS = ["meta", "src_ip", "dst_ip", "ports", "payload", "flow_id", "tcp_seq", "tcp_ack", "tcp_win",
                 "flow_counts", "verdict_counts", "tcp_opts"]

# numpy mirror of struct dk_tcp_opts (96 bytes): the parsed [TcpOptions2; 5] list of one segment.
TCP_OPT_DTYPE = np.dtype([("kind", "u1"), ("u8", "u1"), ("u16", "<u2"), ("v0", "<u4"), ("v1", "<u4")])
TCP_OPTS_DTYPE = np.dtype([("num", "<u4"), ("opt", TCP_OPT_DTYPE, (5,)), ("sack", "<u4", (4, 2))])
assert TCP_OPT_DTYPE.itemsize == 12 and TCP_OPTS_DTYPE.itemsize == 96
DK_TCPOPT_MSS, DK_TCPOPT_WS, DK_TCPOPT_SACK_OK, DK_TCPOPT_SACK, DK_TCPOPT_TS = 2, 3, 4, 5, 8


class DkTcpOpt(ctypes.Structure):
    _fields_ = [("kind", c_uint8), ("u8", c_uint8), ("u16", c_uint16), ("v0", c_uint32), ("v1", c_uint32)]


class DkTcpOpts(ctypes.Structure):
    _fields_ = [("num", c_uint32), ("opt", DkTcpOpt * 5), ("sack", (c_uint32 * 2) * 4)]


class DkRxResults(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in RESULT_FIELDS]


# dk_tx_serialize (include/dk_rx.h): enum dk_tx_status, the offload flags, struct dk_tx_link and struct dk_tx_segs.
TX_STATUSES = ["OK", "E_PROTO", "E_OPTS", "E_LINK", "E_LEN", "E_RANGE"]
DK_TX_OK, DK_TX_E_PROTO, DK_TX_E_OPTS, DK_TX_E_LINK, DK_TX_E_LEN, DK_TX_E_RANGE = range(6)
DK_TX_OFFLOAD_TCP, DK_TX_OFFLOAD_UDP = 1, 2
TX_LINK_DTYPE = np.dtype([("dst_mac", "u1", (6,)), ("src_mac", "u1", (6,)), ("reserved", "<u4")])
assert TX_LINK_DTYPE.itemsize == 16
TX_SEG_FIELDS = ["payload_off", "payload_len", "meta", "src_ip", "dst_ip", "ports", "tcp_seq", "tcp_ack", "tcp_win",
                 "tcp_opts", "ip_word", "link"]


class DkTxLink(ctypes.Structure):
    _fields_ = [("dst_mac", c_uint8 * 6), ("src_mac", c_uint8 * 6), ("reserved", c_uint32)]


class DkTxSegs(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TX_SEG_FIELDS] + [("n", c_uint32), ("flags", c_uint32)]


# (name, restype, argtypes) of every function include/dk_rx.h declares.
FUNCTIONS = [
    ("dk_rx_ctx_create", c_int, [POINTER(DkRxCfg), POINTER(c_void_p)]),
    ("dk_rx_ctx_destroy", None, [c_void_p]),
    ("dk_rx_flow_table_set", c_int, [c_void_p, c_void_p, c_uint32]),
    ("dk_rx_flow_table_size", c_uint32, [c_void_p]),
    ("dk_rx_process", c_int, [c_void_p, POINTER(DkRxBatch), POINTER(DkRxResults), c_void_p]),
    ("dk_rx_process_host", c_int, [c_void_p, POINTER(DkRxBatch), POINTER(DkRxResults), c_uint32]),
    ("dk_rx_stream_forget", c_int, [c_void_p, c_void_p]),
    ("dk_rx_counts_flush", c_int, [c_void_p, c_void_p]),
    ("dk_rx_flow_counts_allreduce", c_int, [c_void_p, POINTER(DkRxResults), c_void_p, c_void_p]),
    ("dk_rx_flow_counts_allreduce_to", c_int, [c_void_p, POINTER(DkRxResults), c_void_p, c_void_p, c_void_p,
                                               c_void_p]),
    ("dk_tx_checksum", c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_uint32, c_void_p]),
    ("dk_tx_checksum_fields", c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p]),
    ("dk_tx_header_bytes", c_uint32, [c_uint32, c_void_p]),
    ("dk_tx_serialize", c_int, [c_void_p, c_uint64, POINTER(DkTxSegs), c_void_p, c_uint32, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    ("dk_rx_verdict_name", c_char_p, [c_int]),
    ("dk_rx_verdict_errno", c_int, [c_int]),
    ("dk_rx_abi_version", c_uint32, []),
    ("dk_rx_build_id", c_char_p, []),
    ("dk_rx_device_count", c_int, []),
]

# include/dk_ring.h (TPACKET_V3 ring ingest)
RING_FUNCTIONS = [
    ("dk_ring_register", c_int, [c_void_p, c_uint64]),
    ("dk_ring_unregister", c_int, [c_void_p]),
    ("dk_ring_scan_tpacket3", c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32,
                                      POINTER(c_uint32), POINTER(c_uint32)]),
    ("dk_ring_release_tpacket3", c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_uint32]),
    ("dk_rx_process_tpacket3", c_int, [c_void_p, c_void_p, c_uint64, c_uint32, c_uint32, c_uint32,
                                       POINTER(DkRxResults), c_uint32, POINTER(c_uint32), POINTER(c_uint32)]),
]

# include/dk_tcp.h (established-state TCP receive processing)
DK_TCP_OOO_MAX = 16
DK_TCP_DELIV_EXTRA = 18
DK_TCP_REF_EOF = 0xFFFFFFFF
DK_TCP_NONE, DK_TCP_ESTABLISHED, DK_TCP_CLOSED = 0, 1, 2
TCP_ACTIONS = ["SKIP", "DELIVERED", "STORED", "STORE_DUP", "NO_DATA", "FIN", "DUPLICATE", "OUT_OF_WINDOW", "RST",
               "SYN", "NO_ACK", "ACK_UNSENT", "UNPROCESSED"]
A = {name: i for i, name in enumerate(TCP_ACTIONS)}
VIEW_DTYPE = np.dtype([("ref", "<u4"), ("off", "<u4"), ("len", "<u4")])
CONN_DTYPE = np.dtype([("state", "<u4"), ("receive_next", "<u4"), ("reader_next", "<u4"), ("buffer_size", "<u4"),
                       ("send_next", "<u4"), ("fin_pending", "<u4"), ("fin_seq", "<u4"), ("ooo_count", "<u4"),
                       ("ooo_start", "<u4", (DK_TCP_OOO_MAX,)), ("ooo", VIEW_DTYPE, (DK_TCP_OOO_MAX,))])
assert CONN_DTYPE.itemsize == 288


class DkTcpView(ctypes.Structure):
    _fields_ = [("ref", c_uint32), ("off", c_uint32), ("len", c_uint32)]


class DkTcpConn(ctypes.Structure):
    _fields_ = [("state", c_uint32), ("receive_next", c_uint32), ("reader_next", c_uint32),
                ("buffer_size", c_uint32), ("send_next", c_uint32), ("fin_pending", c_uint32), ("fin_seq", c_uint32),
                ("ooo_count", c_uint32), ("ooo_start", c_uint32 * DK_TCP_OOO_MAX),
                ("ooo", DkTcpView * DK_TCP_OOO_MAX)]


class DkTcpOut(ctypes.Structure):
    _fields_ = [("action", c_void_p), ("view", c_void_p), ("deliv", c_void_p), ("deliv_start", c_void_p),
                ("deliv_count", c_void_p)]


TCP_FUNCTIONS = [
    ("dk_tcp_ctx_create", c_int, [c_int32, POINTER(c_void_p)]),
    ("dk_tcp_ctx_destroy", None, [c_void_p]),
    ("dk_tcp_rx_process", c_int, [c_void_p, POINTER(DkRxResults), c_uint32, c_void_p, c_uint32, POINTER(DkTcpOut),
                                  c_void_p]),
]

# include/dk_tcp.h, the sender's reaction to ACKs (dk_tcp_ack_process)
DK_TCP_TX_TIME_NONE = 0xFFFFFFFFFFFFFFFF
TCP_ACK_STATUSES = ["OK", "E_STATE", "E_SND_NXT", "E_FLIGHT", "E_WSCALE", "E_WL2", "E_QUEUE", "E_DRY"]
ACK_CONN_DTYPE = np.dtype([("wl1", "<u4"), ("wl2", "<u4"), ("snd_wscale", "<u4"), ("received_sample", "<u4"),
                           ("q_first", "<u4"), ("q_count", "<u4"), ("rtx_armed", "<u4"), ("reserved", "<u4"),
                           ("srtt", "<f8"), ("rttvar", "<f8"), ("rto", "<f8"), ("rtx_base_ns", "<u8")])
assert ACK_CONN_DTYPE.itemsize == 64
TCP_ACK_OUT_FIELDS = ["acked", "status", "new_acks", "dup_acks", "bytes_acked", "samples"]


class DkTcpAckConn(ctypes.Structure):
    _fields_ = [("wl1", c_uint32), ("wl2", c_uint32), ("snd_wscale", c_uint32), ("received_sample", c_uint32),
                ("q_first", c_uint32), ("q_count", c_uint32), ("rtx_armed", c_uint32), ("reserved", c_uint32),
                ("srtt", ctypes.c_double), ("rttvar", ctypes.c_double), ("rto", ctypes.c_double),
                ("rtx_base_ns", c_uint64)]


class DkTcpUnacked(ctypes.Structure):
    _fields_ = [("off", c_void_p), ("len", c_void_p), ("tx_time", c_void_p)]


class DkTcpAckOut(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_ACK_OUT_FIELDS]


TCP_ACK_FUNCTIONS = [
    ("dk_tcp_ack_process", c_int, [c_void_p, POINTER(DkRxResults), c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_uint32, POINTER(DkTcpUnacked), c_uint32, c_uint64, POINTER(DkTcpAckOut),
                                   c_void_p]),
]

# include/dk_tcp.h, TCP send segmentation (dk_tcp_tx_segment)
TCP_TX_STATUSES = ["SENT", "PARTIAL", "UNSENT", "CLOSED", "E_CONN", "NO_ROOM"]
(DK_TCP_TX_SENT, DK_TCP_TX_PARTIAL, DK_TCP_TX_UNSENT, DK_TCP_TX_CLOSED, DK_TCP_TX_E_CONN,
 DK_TCP_TX_NO_ROOM) = range(6)
TX_CONN_FIELDS = ["state", "snd_una", "snd_nxt", "snd_wnd", "cwnd", "mss", "rcv_nxt", "rcv_wscale", "local_ip",
                  "remote_ip", "ports", "ip_word", "link", "fin_sent"]
TX_CONN_DTYPE = np.dtype([(k, "<u4") for k in TX_CONN_FIELDS] +
                         [("rcv_wnd_hdr", "<u2"), ("reserved0", "<u2"), ("reserved1", "<u4")])
assert TX_CONN_DTYPE.itemsize == 64
TCP_TX_RESULT_FIELDS = ["off_out", "len_out", "frame_buf", "sent", "first_frame", "frame_count", "status", "n_frames"]


class DkTcpTxConn(ctypes.Structure):
    _fields_ = [(k, c_uint32) for k in TX_CONN_FIELDS] + [("rcv_wnd_hdr", c_uint16), ("reserved0", c_uint16),
                                                          ("reserved1", c_uint32)]


class DkTcpTxPush(ctypes.Structure):
    _fields_ = [("conn", c_void_p), ("off", c_void_p), ("len", c_void_p)]


class DkTcpTxLayout(ctypes.Structure):
    _fields_ = [("slot_stride", c_uint32), ("frame_lead", c_uint32)]


class DkTcpTxResults(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_TX_RESULT_FIELDS]


TCP_TX_FUNCTIONS = [
    ("dk_tcp_tx_ctx_create", c_int, [c_int32, POINTER(c_void_p)]),
    ("dk_tcp_tx_ctx_destroy", None, [c_void_p]),
    ("dk_tcp_tx_frame_bound", c_uint64, [c_void_p, c_uint32, c_uint32]),
    ("dk_tcp_tx_segment", c_int, [c_void_p, c_void_p, c_uint64, POINTER(DkTcpTxPush), c_uint32, c_void_p, c_uint32,
                                  c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, POINTER(DkTcpTxLayout), c_uint32,
                                  c_uint32, POINTER(DkTcpTxResults), c_void_p]),
]

# include/dk_tcp.h, retransmission (dk_tcp_retransmit)
DK_TCP_RTX_NONE, DK_TCP_RTX_TIMEOUT, DK_TCP_RTX_FAST = range(3)
TCP_RTX_STATUSES = ["NOT_FIRED", "SENT", "IDLE", "E_FIRE", "E_STATE", "E_QUEUE", "E_RANGE", "E_SLOT", "E_LINK",
                    "E_WINDOW", "NO_ROOM"]
(DK_TCP_RTX_NOT_FIRED, DK_TCP_RTX_SENT, DK_TCP_RTX_IDLE, DK_TCP_RTX_E_FIRE, DK_TCP_RTX_E_STATE, DK_TCP_RTX_E_QUEUE,
 DK_TCP_RTX_E_RANGE, DK_TCP_RTX_E_SLOT, DK_TCP_RTX_E_LINK, DK_TCP_RTX_E_WINDOW, DK_TCP_RTX_NO_ROOM) = range(11)
DK_TCP_RTX_NO_FRAME = 0xFFFFFFFF
TCP_RTX_RESULT_FIELDS = ["off_out", "len_out", "frame_conn", "status", "frame", "n_frames"]


class DkTcpRtxResults(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_RTX_RESULT_FIELDS]


TCP_RTX_FUNCTIONS = [
    ("dk_tcp_retransmit", c_int, [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p,
                                  POINTER(DkTcpUnacked), c_uint32, c_uint64, c_void_p, c_uint32, c_void_p, c_uint64,
                                  POINTER(DkTcpTxLayout), c_uint32, c_uint32, POINTER(DkTcpRtxResults), c_void_p]),
]

# include/dk_tcp.h, the receiver's ACKs (dk_tcp_ack_emit, dk_tcp_ack_timer)
TCP_ACKEMIT_STATUSES = ["OK", "E_STATE", "E_SND_NXT", "E_LINK", "E_WSCALE", "E_WINDOW", "E_SLOT", "NO_ROOM", "NOT_FIRED",
                        "IDLE"]
DK_TCP_ACKEMIT_NO_FRAME = 0xFFFFFFFF
DACK_CONN_DTYPE = np.dtype([("armed", "<u4"), ("reserved", "<u4"), ("delay_ns", "<u8"), ("deadline_ns", "<u8"),
                            ("reserved1", "<u8")])
assert DACK_CONN_DTYPE.itemsize == 32
TCP_ACKEMIT_RESULT_FIELDS = ["off_out", "len_out", "frame_conn", "frame_seg", "ack_frame", "status", "n_acks", "n_frames"]


class DkTcpDackConn(ctypes.Structure):
    _fields_ = [("armed", c_uint32), ("reserved", c_uint32), ("delay_ns", c_uint64), ("deadline_ns", c_uint64),
                ("reserved1", c_uint64)]


class DkTcpAckEmitResults(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_ACKEMIT_RESULT_FIELDS]


TCP_ACKEMIT_FUNCTIONS = [
    ("dk_tcp_ack_emit", c_int, [c_void_p, POINTER(DkRxResults), c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_uint32, c_void_p, c_uint32, c_uint64, c_void_p, c_uint64,
                                POINTER(DkTcpTxLayout), c_uint32, c_uint32, POINTER(DkTcpAckEmitResults), c_void_p]),
    ("dk_tcp_ack_timer", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32,
                                 c_void_p, c_uint64, POINTER(DkTcpTxLayout), c_uint32, c_uint32,
                                 POINTER(DkTcpAckEmitResults), c_void_p]),
]

# include/dk_tcp.h, congestion control and timer expiry (dk_tcp_cc_ack, dk_tcp_timers, dk_tcp_cc_send)
TCP_CC_STATUSES = ["OK", "E_STATE", "E_SND_NXT", "E_MSS", "E_RTO"]
DK_TCP_CC_OK, DK_TCP_CC_E_STATE, DK_TCP_CC_E_SND_NXT, DK_TCP_CC_E_MSS, DK_TCP_CC_E_RTO = range(5)
TCP_CC_FLAGS = {"CUBIC": 1, "FAST_CONVERGENCE": 2, "IN_RECOVERY": 4, "LAST_WAS_RTO": 8, "RETRANSMIT_NOW": 16}
DK_TCP_CC_BEFORE_SEND, DK_TCP_CC_AFTER_SEND = range(2)
CC_CONN_U32 = ["flags", "cwnd", "ssthresh", "w_max", "initial_cwnd", "ltci", "dup_acks", "rpif", "recover", "prev_ack"]
CC_CONN_U64 = ["ca_start_ns", "last_send_ns", "rtt_at_last_send_ns"]
CC_CONN_DTYPE = np.dtype([(k, "<u4") for k in CC_CONN_U32] + [(k, "<u8") for k in CC_CONN_U64])
assert CC_CONN_DTYPE.itemsize == 64
TCP_CC_ACK_OUT_FIELDS = ["status", "new_acks", "dup_acks", "cwnd_after"]
TCP_TIMERS_OUT_FIELDS = ["status", "n_fast", "n_timeout", "n_ack"]


class DkTcpCcConn(ctypes.Structure):
    _fields_ = [(k, c_uint32) for k in CC_CONN_U32] + [(k, c_uint64) for k in CC_CONN_U64]


class DkTcpCcAckOut(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_CC_ACK_OUT_FIELDS]


class DkTcpTimersOut(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_TIMERS_OUT_FIELDS]


TCP_CC_FUNCTIONS = [
    ("dk_tcp_rto_ns", c_uint64, [ctypes.c_double]),
    ("dk_tcp_cc_ack", c_int, [c_void_p, POINTER(DkRxResults), c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_uint32, c_uint64, POINTER(DkTcpCcAckOut), c_void_p]),
    ("dk_tcp_timers", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_uint64, c_void_p,
                              c_void_p, POINTER(DkTcpTimersOut), c_void_p]),
    ("dk_tcp_cc_send", c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, POINTER(DkTcpTxPush),
                               c_uint32, POINTER(DkTcpTxResults), c_uint64, c_void_p, c_void_p]),
]

# include/dk_tcp.h, the send side's bookkeeping (dk_tcp_tx_commit, dk_tcp_rtx_piggyback)
TCP_COMMIT_STATUSES = ["OK", "E_QUEUE", "E_FULL"]
DK_TCP_COMMIT_OK, DK_TCP_COMMIT_E_QUEUE, DK_TCP_COMMIT_E_FULL = range(3)
TCP_COMMIT_OUT_FIELDS = ["status", "appended"]


class DkTcpCommitOut(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_COMMIT_OUT_FIELDS]


TCP_COMMIT_FUNCTIONS = [
    ("dk_tcp_tx_commit", c_int, [c_void_p, POINTER(DkTcpTxPush), c_uint32, POINTER(DkTcpTxResults), c_uint32, c_void_p,
                                 c_uint32, POINTER(DkTcpUnacked), c_uint32, c_uint32, c_void_p, c_uint64,
                                 POINTER(DkTcpCommitOut), c_void_p]),
    ("dk_tcp_rtx_piggyback", c_int, [c_void_p, POINTER(DkTcpRtxResults), c_void_p, c_uint32, c_void_p]),
]

# include/dk_tcp.h, the passive open (dk_tcp_listen_*)
DK_TCP_LSN_NONE = 0xFFFFFFFF
DK_TCP_LSN_NO_WSCALE = 0xFF
DK_TCP_LSN_FALLBACK_MSS = 536
DK_TCP_LSN_MAX_LISTENERS = 65535
DK_TCP_LSN_SYNACK_BYTES, DK_TCP_LSN_RST_BYTES = 62, 54
DK_TCP_LSN_KEY_FREE = 0xFFFFFFFFFFFFFFFF
DK_TCP_LSN_KEY_TOMBSTONE = 0xFFFF << 48
DK_TCP_LSN_CLOSED, DK_TCP_LSN_LISTENING = 0, 1
TCP_LSN_SLOT_STATES = ["FREE", "SYN_RCVD", "ESTAB", "FAILED", "TOMBSTONE"]
TCP_LSN_ACTIONS = ["SKIP", "SYN_ACCEPTED", "ESTABLISHED", "ESTABLISHED_DATA", "BAD_ACK", "FORWARD", "ORPHANED",
                   "RST_FLAGS", "RST_BACKLOG"]
TCP_LSN_STATUSES = ["OK", "E_WSCALE", "E_LINK", "E_SLOT", "E_TABLE", "NO_ROOM"]
LISTENER_DTYPE = np.dtype([("state", "<u4"), ("flow_id", "<u4"), ("local_ip", "<u4"), ("local_port", "<u2"),
                           ("receive_window_size", "<u2"), ("max_backlog", "<u4"), ("nonce", "<u4"),
                           ("advertised_mss", "<u2"), ("window_scale", "u1"), ("reserved0", "u1"),
                           ("handshake_retries", "<u4"), ("handshake_timeout_ns", "<u8"), ("ip_word", "<u4"),
                           ("link", "<u4"), ("inflight", "<u4"), ("isn_counter", "<u2"), ("reserved1", "<u2"),
                           ("reserved2", "<u8")])
LSN_SLOT_DTYPE = np.dtype([("key", "<u8"), ("state", "<u4"), ("err", "<u4"), ("remote_isn", "<u4"),
                           ("local_isn", "<u4"), ("syn_window", "<u2"), ("mss", "<u2"), ("remote_wscale", "u1"),
                           ("reserved0", "u1"), ("reserved1", "<u2"), ("retries_left", "<u4"), ("reserved2", "<u4"),
                           ("deadline_ns", "<u8")])
LSN_READY_DTYPE = np.dtype([("listener", "<u4"), ("remote_ip", "<u4"), ("remote_port", "<u2"), ("err", "<u2"),
                            ("frame", "<u4"), ("rcv_nxt", "<u4"), ("snd_nxt", "<u4"), ("local_window", "<u4"),
                            ("remote_window", "<u4"), ("mss", "<u4"), ("local_wscale", "u1"), ("remote_wscale", "u1"),
                            ("reserved0", "<u2"), ("slot", "<u4"), ("reserved1", "<u4")])
assert LISTENER_DTYPE.itemsize == 64 and LSN_SLOT_DTYPE.itemsize == 48 and LSN_READY_DTYPE.itemsize == 48
TCP_LSN_RESULT_FIELDS = ["action", "slot", "reply_frame", "off_out", "len_out", "frame_seg", "ready", "status",
                         "n_frames", "n_ready"]
_NP_C = {"<u4": c_uint32, "<u2": c_uint16, "u1": c_uint8, "|u1": c_uint8, "<u8": c_uint64}


def _mirror(dtype: np.dtype):
    return [(k, _NP_C[dtype.fields[k][0].str]) for k in dtype.names]


class DkTcpListener(ctypes.Structure):
    _fields_ = _mirror(LISTENER_DTYPE)


class DkTcpLsnSlot(ctypes.Structure):
    _fields_ = _mirror(LSN_SLOT_DTYPE)


class DkTcpLsnReady(ctypes.Structure):
    _fields_ = _mirror(LSN_READY_DTYPE)


class DkTcpLsnResults(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_LSN_RESULT_FIELDS]


TCP_LISTEN_FUNCTIONS = [
    ("dk_tcp_listen_table_create", c_int, [c_int32, c_uint32, POINTER(c_void_p)]),
    ("dk_tcp_listen_table_destroy", None, [c_void_p]),
    ("dk_tcp_listen_table_stats", c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint64)]),
    ("dk_tcp_listen_table_read", c_int, [c_void_p, c_void_p]),
    ("dk_tcp_listen_table_write", c_int, [c_void_p, c_void_p]),
    ("dk_tcp_listen_key", c_uint64, [c_uint32, c_uint32, c_uint16]),
    ("dk_tcp_listen_home", c_uint32, [c_uint32, c_uint64]),
    ("dk_tcp_listen_backlog_fits", c_int, [c_uint32, c_uint64]),
    ("dk_tcp_listen_process", c_int, [c_void_p, POINTER(DkRxResults), c_uint32, c_void_p, c_uint32, c_uint64, c_void_p,
                                      c_uint32, c_void_p, c_void_p, c_uint32, c_uint64, c_void_p, c_uint64,
                                      POINTER(DkTcpTxLayout), c_uint32, c_uint32, c_uint32, POINTER(DkTcpLsnResults),
                                      c_void_p]),
    ("dk_tcp_listen_timers", c_int, [c_void_p, c_void_p, c_uint32, c_uint64, c_void_p, c_uint32, c_uint64, c_void_p,
                                     c_uint64, POINTER(DkTcpTxLayout), c_uint32, c_uint32, c_uint32,
                                     POINTER(DkTcpLsnResults), c_void_p]),
    ("dk_tcp_listen_release", c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p]),
]

# include/dk_tcp.h, the active open (dk_tcp_connect_*)
DK_TCP_CON_NONE = 0xFFFFFFFF
DK_TCP_CON_FALLBACK_MSS = 536
DK_TCP_CON_SYN_BYTES, DK_TCP_CON_ACK_BYTES = 62, 54
TCP_CON_STATES = ["IDLE", "CONNECTING", "ESTAB", "FAILED", "CLOSED"]
TCP_CON_ACTIONS = ["SKIP", "ESTABLISHED", "RETRY_SYN", "EXHAUSTED", "REFUSED", "FORWARD", "ORPHANED"]
TCP_CON_CAUSES = ["CAUSE_NONE", "CAUSE_RST", "CAUSE_EXHAUSTED"]
TCP_CON_STATUSES = ["OK", "E_ROW", "E_STATE", "E_WSCALE", "E_LINK", "E_SLOT", "NO_ROOM"]
CONNECTOR_DTYPE = np.dtype([("state", "<u2"), ("err", "<u2"), ("flow_id", "<u4"), ("local_ip", "<u4"),
                            ("remote_ip", "<u4"), ("local_port", "<u2"), ("remote_port", "<u2"), ("local_isn", "<u4"),
                            ("receive_window_size", "<u2"), ("advertised_mss", "<u2"), ("window_scale", "u1"),
                            ("reserved0", "u1"), ("reserved1", "<u2"), ("handshake_retries", "<u4"),
                            ("syns_left", "<u4"), ("handshake_timeout_ns", "<u8"), ("deadline_ns", "<u8"),
                            ("ip_word", "<u4"), ("link", "<u4")])
ISN_GEN_DTYPE = np.dtype([("nonce", "<u4"), ("counter", "<u2"), ("reserved", "<u2")])
CON_READY_DTYPE = np.dtype([("row", "<u4"), ("err", "<u2"), ("cause", "<u2"), ("frame", "<u4"), ("rcv_nxt", "<u4"),
                            ("snd_nxt", "<u4"), ("local_window", "<u4"), ("remote_window", "<u4"), ("mss", "<u4"),
                            ("local_wscale", "u1"), ("remote_wscale", "u1"), ("reserved0", "<u2"), ("reserved1", "<u4"),
                            ("reserved2", "<u8")])
assert CONNECTOR_DTYPE.itemsize == 64 and ISN_GEN_DTYPE.itemsize == 8 and CON_READY_DTYPE.itemsize == 48
TCP_CON_RESULT_FIELDS = ["action", "row", "reply_frame", "off_out", "len_out", "frame_seg", "ready", "status",
                         "n_frames", "n_ready"]


class DkTcpConnector(ctypes.Structure):
    _fields_ = _mirror(CONNECTOR_DTYPE)


class DkTcpIsnGen(ctypes.Structure):
    _fields_ = _mirror(ISN_GEN_DTYPE)


class DkTcpConReady(ctypes.Structure):
    _fields_ = _mirror(CON_READY_DTYPE)


class DkTcpConResults(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_CON_RESULT_FIELDS]


TCP_CONNECT_FUNCTIONS = [
    ("dk_tcp_connect_start", c_int, [c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, c_uint64,
                                     c_void_p, c_uint64, POINTER(DkTcpTxLayout), c_uint32, c_uint32, c_uint32,
                                     POINTER(DkTcpConResults), c_void_p]),
    ("dk_tcp_connect_process", c_int, [POINTER(DkRxResults), c_uint32, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p,
                                       c_void_p, c_uint32, c_uint64, c_void_p, c_uint64, POINTER(DkTcpTxLayout), c_uint32,
                                       c_uint32, c_uint32, POINTER(DkTcpConResults), c_void_p]),
    ("dk_tcp_connect_timers", c_int, [c_void_p, c_uint32, c_void_p, c_uint32, c_uint64, c_void_p, c_uint64,
                                      POINTER(DkTcpTxLayout), c_uint32, c_uint32, c_uint32, POINTER(DkTcpConResults),
                                      c_void_p]),
]

# include/dk_tcp.h, closing a connection (dk_tcp_close_*)
DK_TCP_CLS_NONE = 0xFFFFFFFF
DK_TCP_CLS_TIME_WAIT_NS = 4_000_000_000
DK_TCP_CLS_RETIRED = 1
DK_TCP_CLS_ACK_BYTES = 54
TCP_CLS_STATES = ["IDLE", "FIN_WAIT_1", "FIN_WAIT_2", "CLOSING", "TIME_WAIT", "LAST_ACK", "CLOSED", "FAULT"]
TCP_CLS_ACTION_BITS = {"POPPED": 1, "ACK_OK": 2, "ACK_UNSENT": 4, "FIN": 8, "FAULT_BIT": 16, "UNPROCESSED": 32}
TCP_CLS_STATUSES = ["OK", "E_ROW", "E_ORDER", "E_STATE", "E_BADF", "E_RX_STATE", "E_LINK", "E_WSCALE", "E_WINDOW",
                    "E_SLOT", "NO_ROOM"]
CLOSER_DTYPE = np.dtype([("state", "<u2"), ("err", "<u2"), ("flags", "<u4"), ("linger_ns", "<u8"),
                         ("deadline_ns", "<u8"), ("reserved", "<u8")])
CLS_DONE_DTYPE = np.dtype([("row", "<u4"), ("state", "<u2"), ("err", "<u2"), ("frame", "<u4"), ("fin_frame", "<u4"),
                           ("deadline_ns", "<u8"), ("reserved", "<u8")])
assert CLOSER_DTYPE.itemsize == 32 and CLS_DONE_DTYPE.itemsize == 32
TCP_CLS_RESULT_FIELDS = ["action", "state_after", "ack_action", "reply_frame", "off_out", "len_out", "frame_seg", "done",
                         "status", "fin_frame", "n_frames", "n_done"]


class DkTcpCloser(ctypes.Structure):
    _fields_ = _mirror(CLOSER_DTYPE)


class DkTcpClsDone(ctypes.Structure):
    _fields_ = _mirror(CLS_DONE_DTYPE)


class DkTcpClsResults(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in TCP_CLS_RESULT_FIELDS]


TCP_CLOSE_FUNCTIONS = [
    ("dk_tcp_close_start", c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    ("dk_tcp_close_process", c_int, [POINTER(DkRxResults), c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32,
                                     c_void_p, c_void_p, c_uint32, c_uint64, c_void_p, c_uint64, POINTER(DkTcpTxLayout),
                                     c_uint32, c_uint32, c_uint32, POINTER(DkTcpClsResults), c_void_p]),
    ("dk_tcp_close_timers", c_int, [c_void_p, c_void_p, c_uint32, c_uint64, c_void_p, c_uint32, c_void_p, c_void_p,
                                    c_void_p]),
]

# include/dk_arp.h, the ARP peer (dk_arp_*)
DK_ARP_NONE = 0xFFFFFFFF
DK_ARP_NO_LINK = 0xFFFFFFFF
DK_ARP_FRAME_BYTES = 42
DK_ARP_DISABLED = 1
DK_ARP_MAX_RETRIES = 65534
ARP_ACTION_BITS = {"HIT": 1, "INSERTED": 2, "REPLY": 4, "LEARNED": 8, "DROPPED": 16}
ARP_SLOT_STATES = ["FREE", "LIVE", "TOMBSTONE"]
ARP_QUERY_STATES = ["IDLE", "WAITING", "RESOLVED", "FAILED"]
ARP_STATUSES = ["OK", "E_ROW", "E_STATE", "E_LINK", "E_SLOT", "NO_ROOM"]
ARP_CFG_DTYPE = np.dtype([("local_ip", "<u4"), ("local_mac", "u1", (6,)), ("reserved0", "<u2"), ("flags", "<u4"),
                          ("retry_count", "<u4"), ("reserved1", "<u4"), ("cache_ttl_ns", "<u8"), ("request_timeout_ns", "<u8")])
ARP_SLOT_DTYPE = np.dtype([("ip", "<u4"), ("state", "<u4"), ("mac", "u1", (6,)), ("reserved", "<u2"),
                           ("expiration_ns", "<u8")])
ARP_QUERY_DTYPE = np.dtype([("ip", "<u4"), ("link", "<u4"), ("tag", "<u4"), ("state", "<u2"), ("err", "<u2"),
                            ("deadline_ns", "<u8"), ("mac", "u1", (6,)), ("sent", "<u2")])
ARP_READY_DTYPE = np.dtype([("row", "<u4"), ("tag", "<u4"), ("ip", "<u4"), ("frame", "<u4"), ("mac", "u1", (6,)),
                            ("err", "<u2")])
assert (ARP_CFG_DTYPE.itemsize, ARP_SLOT_DTYPE.itemsize, ARP_QUERY_DTYPE.itemsize,
        ARP_READY_DTYPE.itemsize) == (40, 24, 32, 24)
ARP_RESULT_FIELDS = ["action", "reply_frame", "off_out", "len_out", "frame_seg", "ready", "status", "n_frames",
                     "n_ready", "n_entries"]


def _mirror_arp(dtype: np.dtype):
    return [(k, c_uint8 * 6 if dtype.fields[k][0].shape == (6,) else _NP_C[dtype.fields[k][0].str]) for k in dtype.names]


class DkArpCfg(ctypes.Structure):
    _fields_ = _mirror_arp(ARP_CFG_DTYPE)


class DkArpSlot(ctypes.Structure):
    _fields_ = _mirror_arp(ARP_SLOT_DTYPE)


class DkArpQuery(ctypes.Structure):
    _fields_ = _mirror_arp(ARP_QUERY_DTYPE)


class DkArpReady(ctypes.Structure):
    _fields_ = _mirror_arp(ARP_READY_DTYPE)


class DkArpResults(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in ARP_RESULT_FIELDS]


ARP_FUNCTIONS = [
    ("dk_arp_home", c_uint32, [c_uint32, c_uint32]),
    ("dk_arp_fits", c_int, [c_uint32, c_uint64]),
    ("dk_arp_table_create", c_int, [c_int32, c_uint32, POINTER(DkArpCfg), POINTER(c_void_p)]),
    ("dk_arp_table_destroy", None, [c_void_p]),
    ("dk_arp_table_stats", c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint64)]),
    ("dk_arp_table_read", c_int, [c_void_p, c_void_p]),
    ("dk_arp_table_write", c_int, [c_void_p, c_void_p]),
    ("dk_arp_table_insert", c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_uint64]),
    ("dk_arp_process", c_int, [c_void_p, POINTER(DkRxBatch), POINTER(DkRxResults), c_uint32, c_void_p, c_uint32,
                               c_void_p, c_uint32, c_uint64, c_void_p, c_uint64, POINTER(DkTcpTxLayout), c_uint32,
                               c_uint32, POINTER(DkArpResults), c_void_p]),
    ("dk_arp_query_start", c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_uint32, c_uint64,
                                   c_void_p, c_uint64, POINTER(DkTcpTxLayout), c_uint32, c_uint32,
                                   POINTER(DkArpResults), c_void_p]),
    ("dk_arp_timers", c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_uint64, c_void_p, c_uint64,
                              POINTER(DkTcpTxLayout), c_uint32, c_uint32, POINTER(DkArpResults), c_void_p]),
    ("dk_arp_lookup", c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p,
                              c_void_p]),
]

# include/dk_diag.h (diagnostics, not the receive ABI)
# include/dk_demi.h: delivered frames as demi_sgarray_t (host-side, no GPU work)
class DemiSgaseg(ctypes.Structure):
    _pack_ = 1
    _fields_ = [("sgaseg_buf", c_void_p), ("sgaseg_len", c_uint32)]


class SockaddrIn(ctypes.Structure):
    _fields_ = [("sin_family", ctypes.c_uint16), ("sin_port", ctypes.c_uint16), ("sin_addr", c_uint32),
                ("sin_zero", ctypes.c_uint8 * 8)]


class DemiSgarray(ctypes.Structure):
    _pack_ = 1
    _fields_ = [("sga_buf", c_void_p), ("sga_numsegs", c_uint32), ("sga_segs", DemiSgaseg * 1),
                ("sga_addr", SockaddrIn)]


DEMI_FUNCTIONS = [
    ("dk_rx_into_sgarrays", c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    POINTER(DemiSgarray), c_void_p, c_uint32, POINTER(c_uint32)]),
    ("dk_tcp_into_sgarrays", c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, POINTER(DemiSgarray),
                                     c_uint32, POINTER(c_uint32)]),
]

# include/dk_comm.h: RCCL communicator bootstrap (the receive path's one collective is dk_rx_flow_counts_allreduce)
DK_COMM_ID_BYTES = 128
COMM_FUNCTIONS = [
    ("dk_comm_unique_id", c_int, [c_void_p]),
    ("dk_comm_init_rank", c_int, [POINTER(c_void_p), c_int32, c_void_p, c_int32, c_int32]),
    ("dk_comm_init_all", c_int, [c_void_p, c_int32, c_void_p]),
    ("dk_comm_count", c_int, [c_void_p, POINTER(c_int32)]),
    ("dk_comm_destroy", c_int, [c_void_p]),
]

DIAG_FUNCTIONS = [
    ("dk_diag_read_probe", c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_int, c_void_p]),
    ("dk_diag_rw_probe", c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p]),
    ("dk_diag_patch_probe", c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_uint32, c_void_p, c_uint32, c_void_p]),
    ("dk_diag_path_stats_enable", c_int, [c_void_p, c_int]),
    ("dk_diag_path_stats_read", c_int, [c_void_p, c_void_p]),
    ("dk_diag_rx_set_tuning", c_int, [c_void_p, c_void_p, c_uint32]),
    ("dk_diag_tx_set_tuning", c_int, [c_int32, c_int32, c_int32]),
    ("dk_diag_tx_serialize_set_grid", c_int, [c_int32]),
    ("dk_diag_tcp_tx_set_grid", c_int, [c_int32]),
    ("dk_diag_tcp_set_walk", c_int, [c_void_p, c_int32, c_int32]),
    ("dk_diag_tcp_last_walk", c_int, [c_void_p]),
    ("dk_diag_tcp_set_sort", c_int, [c_void_p, c_int32]),
    ("dk_diag_tcp_last_sort", c_int, [c_void_p]),
    ("dk_diag_tcp_ack_set_form", c_int, [c_void_p, c_int32]),
    ("dk_diag_tcp_ack_last_form", c_int, [c_void_p]),
    ("dk_diag_tcp_ack_emit_set_form", c_int, [c_void_p, c_int32]),
    ("dk_diag_tcp_ack_emit_last_form", c_int, [c_void_p]),
    ("dk_diag_tcp_cc_cbrt", c_int, [c_void_p, c_void_p, c_uint32, c_void_p]),
    ("dk_diag_tcp_commit_set_form", c_int, [c_void_p, c_int32]),
    ("dk_diag_tcp_commit_last_form", c_int, [c_void_p]),
]
DK_DIAG_RX_KNOBS = ["stage", "split", "small", "sched", "grid", "grid_per_cu", "debug", "lds_table", "tail", "udp_table",
                    "host_zc"]
DK_TCP_WALKS = {"lane": 0, "wave": 1, "relay": 2, "scan": 3}
DK_TCP_SORTS = {"counting": 0, "radix": 1}
DK_TCP_ACK_FORMS = {"lane": 0, "wave": 1, "chip": 2}
DK_TCP_ACK_EMIT_FORMS = {"lane": 0, "scan": 1}
DK_TCP_COMMIT_FORMS = {"conn": 0, "chip": 1}

ALL_FUNCTIONS = (FUNCTIONS + RING_FUNCTIONS + TCP_FUNCTIONS + TCP_ACK_FUNCTIONS + TCP_TX_FUNCTIONS + TCP_RTX_FUNCTIONS +
                 TCP_ACKEMIT_FUNCTIONS + TCP_CC_FUNCTIONS + TCP_COMMIT_FUNCTIONS + TCP_LISTEN_FUNCTIONS +
                 TCP_CONNECT_FUNCTIONS + TCP_CLOSE_FUNCTIONS +
                 DIAG_FUNCTIONS +
                 DEMI_FUNCTIONS + COMM_FUNCTIONS)

# include/dk_arp.h is a header of its own: its functions are bound beside the list above (tests/test_arp_abi.py checks
# them against that header, as tests/test_abi.py checks ALL_FUNCTIONS against the others).
BOUND_FUNCTIONS = ALL_FUNCTIONS + ARP_FUNCTIONS

_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libdk_rx.so (fails loudly: there is no CPU fallback for the product path)."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    # One HIP runtime per process: torch ships its own libamdhip64 (SONAME libamdhip64.so.7, NEEDED as
    # "libamdhip64.so"). Loaded first, it also satisfies our NEEDED libamdhip64.so.7; loaded after us, it would be a
    # second runtime and device pointers/streams would not be shared.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    for name, restype, argtypes in BOUND_FUNCTIONS:
        fn = getattr(lib, name, None)
        if fn is None:
            if path != LIB_PATH:
                continue  # tuning builds (older sources) may predate a function
            raise ImportError(f"{path}: missing {name}")
        fn.restype = restype
        fn.argtypes = argtypes
    if path == LIB_PATH:
        _lib = lib
    return lib
