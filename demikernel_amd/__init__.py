"""demikernel_amd — MI355X-native receive path for Demikernel's inetstack.

One hot path, rebuilt for gfx950: per-frame Ethernet/IPv4/TCP/UDP parse, the one's-complement Internet checksums and
the 4-tuple socket demux, run as hand-written HIP kernels over HBM-resident frame batches behind a C ABI
(include/dk_rx.h, libdk_rx.so). See DESIGN.md and INTEGRATION.md.
"""
from .rx import (  # noqa: F401
    Comm,
    Config,
    Fail,
    FrameBatch,
    RxEngine,
    RxResults,
    SocketId,
    V,
    VERDICTS,
    flow_array,
    ipv4,
    ipv4_str,
    raise_for_verdict,
    tx_tuning,
)
from .tx import TxSegments, tx_header_bytes, tx_links, tx_serialize  # noqa: F401
from .tcp_tx import PushList, TcpSender, TcpTxResults, tx_conn_table  # noqa: F401
from .tcp_ack import TcpAcker, TcpAckOut, UnackedQueue, ack_conn_table, sync_send_next  # noqa: F401
from .tcp_rtx import RtxResults, retransmit, retransmit_batch  # noqa: F401
from .tcp_ackemit import AckEmitResults, ack_emit, ack_emit_batch, ack_timer, dack_conn_table  # noqa: F401
from .tcp_cc import CcAckOut, TimersOut, cc_ack, cc_conn_table, cc_send, timers  # noqa: F401
from .tcp_commit import CommitOut, rtx_piggyback, tx_commit  # noqa: F401
from .tcp_listen import ListenResults, ListenTable, listen_process, listen_release, listen_timers, listener_table  # noqa: F401
from .tcp_connect import (ConnectResults, conn_of_flow, conn_rows_from_connect_ready, connect_process, connect_start,  # noqa: F401
                          connect_timers, connector_table)
from .tcp_close import CloseResults, close_process, close_start, close_timers, closer_table  # noqa: F401
from .arp import ArpResults, ArpTable, arp_cfg, arp_lookup, arp_process, arp_query_start, arp_timers, query_table  # noqa: F401

__all__ = ["ArpResults", "ArpTable", "arp_cfg", "arp_lookup", "arp_process", "arp_query_start", "arp_timers", "query_table",
           "CloseResults", "close_process", "close_start", "close_timers", "closer_table",
           "ConnectResults", "conn_of_flow", "conn_rows_from_connect_ready", "connect_process", "connect_start",
           "connect_timers", "connector_table",
           "ListenResults", "ListenTable", "listen_process", "listen_release", "listen_timers", "listener_table",
           "CommitOut", "rtx_piggyback", "tx_commit", "CcAckOut", "TimersOut", "cc_ack", "cc_conn_table", "cc_send", "timers", "AckEmitResults", "ack_emit", "ack_emit_batch", "ack_timer", "dack_conn_table", "RtxResults", "retransmit", "retransmit_batch", "TcpAcker", "TcpAckOut", "UnackedQueue", "ack_conn_table", "sync_send_next", "PushList", "TcpSender", "TcpTxResults", "tx_conn_table","Comm", "Config", "Fail", "FrameBatch", "RxEngine", "RxResults", "SocketId", "V", "VERDICTS", "flow_array",
           "ipv4", "ipv4_str", "raise_for_verdict", "tx_tuning", "TxSegments", "tx_header_bytes", "tx_links",
           "tx_serialize"]
