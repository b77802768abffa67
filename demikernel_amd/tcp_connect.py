"""The active open on the GPU (include/dk_tcp.h, the dk_tcp_connect_* section).

What TcpPeer::connect and SharedActiveOpenSocket do for a connecting socket (tcp/peer.rs, tcp/active_open.rs): the
ISN, the SYN with its options and its retries, process_ack's three tests on the answer, the handshake ACK, the window
and MSS negotiation, and the arguments of EstablishedSocket::new, for every connector-bound frame of one
RxEngine.receive_batch call at once. The connecting sockets are rows of CONNECTOR_DTYPE in device memory; a ready
record carries what EstablishedSocket::new receives, and conn_rows_from_connect_ready turns one into rows of the
established-state tables.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import RxResults, _check, _ptr
from .tcp_listen import _stream, to_device  # noqa: F401

CONNECTOR_DTYPE, ISN_GEN_DTYPE, READY_DTYPE = N.CONNECTOR_DTYPE, N.ISN_GEN_DTYPE, N.CON_READY_DTYPE
STATES, ACTIONS, CAUSES, STATUSES = N.TCP_CON_STATES, N.TCP_CON_ACTIONS, N.TCP_CON_CAUSES, N.TCP_CON_STATUSES
IDLE, CONNECTING, ESTAB, FAILED, CLOSED = range(5)
SKIP, ESTABLISHED, RETRY_SYN, EXHAUSTED, REFUSED, FORWARD, ORPHANED = range(7)
CAUSE_NONE, CAUSE_RST, CAUSE_EXHAUSTED = range(3)
OK, E_ROW, E_STATE, E_WSCALE, E_LINK, E_SLOT, NO_ROOM = range(7)
NONE = N.DK_TCP_CON_NONE
FALLBACK_MSS = N.DK_TCP_CON_FALLBACK_MSS
SYN_BYTES, ACK_BYTES = N.DK_TCP_CON_SYN_BYTES, N.DK_TCP_CON_ACK_BYTES


def connector_table(nrows: int, **fields) -> np.ndarray:
    """Host table (CONNECTOR_DTYPE, 64-byte items), IDLE, the reference's defaults (receive window 0xFFFF, window scale
    0, advertised MSS 1450, 5 SYNs 3 s apart, ttl 255); scalars or per-row arrays override."""
    t = np.zeros(nrows, CONNECTOR_DTYPE)
    t["receive_window_size"], t["advertised_mss"] = 0xFFFF, 1450
    t["handshake_retries"], t["handshake_timeout_ns"] = 5, 3_000_000_000
    t["ip_word"] = 0x00FF0000
    for k, v in fields.items():
        t[k] = np.asarray(v).astype(CONNECTOR_DTYPE.fields[k][0])
    return t


def isn_gen(nonce: int = 0, counter: int = 0) -> np.ndarray:
    """The peer's IsnGenerator as a one-row ISN_GEN_DTYPE array."""
    g = np.zeros(1, ISN_GEN_DTYPE)
    g["nonce"], g["counter"] = nonce & 0xFFFFFFFF, counter & 0xFFFF
    return g


def conn_of_flow(nflows: int, rows: np.ndarray) -> np.ndarray:
    """The flow_id -> connector row map from the rows' flow_id field; NONE for every other flow."""
    m = np.full(max(nflows, 1), NONE, np.uint32)
    m[rows["flow_id"]] = np.arange(len(rows), dtype=np.uint32)
    return m[:nflows] if nflows else m[:0]


def rows_to_host(dev) -> np.ndarray:
    return dev.cpu().numpy().view(CONNECTOR_DTYPE).copy()


def isn_gen_to_host(dev) -> np.ndarray:
    return dev.cpu().numpy().view(ISN_GEN_DTYPE).copy()


class ConnectResults:
    """Device outputs of one dk_tcp_connect_start / _process / _timers call (dk_tcp_con_results) for n batch frames, up
    to max_frames frames and max_ready ready records, nstatus status words (rows; start[] entries); every array starts
    as `fill` bytes."""

    def __init__(self, n: int, max_frames: int, max_ready: int, nstatus: int, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.n, self.max_frames, self.max_ready, self.nstatus = n, max_frames, max_ready, nstatus
        u8 = lambda k: torch.full((max(k, 4),), fill, dtype=torch.uint8, device=dev)  # noqa: E731
        self.action = u8(n)
        self.row, self.reply_frame = u8(4 * n), u8(4 * n)
        self.off_out, self.len_out, self.frame_seg = u8(4 * max_frames), u8(2 * max_frames), u8(4 * max_frames)
        self.ready = u8(READY_DTYPE.itemsize * max_ready)
        self.status = u8(4 * nstatus)
        self.n_frames, self.n_ready = u8(4), u8(4)

    def c_struct(self) -> N.DkTcpConResults:
        return N.DkTcpConResults(*[_ptr(getattr(self, k)) for k in N.TCP_CON_RESULT_FIELDS])

    def raw(self) -> dict:
        """Every array whole, as bytes (for canary comparisons)."""
        return {k: getattr(self, k).cpu().numpy().copy() for k in N.TCP_CON_RESULT_FIELDS}

    def to_numpy(self) -> dict:
        r = self.raw()
        u32 = lambda k, m: r[k][:4 * m].view(np.uint32)  # noqa: E731
        return {"action": r["action"][:self.n], "row": u32("row", self.n), "reply_frame": u32("reply_frame", self.n),
                "off_out": u32("off_out", self.max_frames), "len_out": r["len_out"][:2 * self.max_frames].view(np.uint16),
                "frame_seg": u32("frame_seg", self.max_frames),
                "ready": r["ready"][:READY_DTYPE.itemsize * self.max_ready].view(READY_DTYPE),
                "status": u32("status", self.nstatus), "n_frames": int(u32("n_frames", 1)[0]),
                "n_ready": int(u32("n_ready", 1)[0])}


def _nrows(rows) -> int:
    return rows.numel() // CONNECTOR_DTYPE.itemsize


def connect_start(rows, start, gen, links, now_ns: int, out, res: ConnectResults, *, slot_stride: int,
                  frame_lead: int = 0, flags: int = 0, nstart: Optional[int] = None, out_bytes=None, max_frames=None,
                  max_ready=None, device: int = 0, stream=None) -> None:
    """dk_tcp_connect_start: rows a uint8 device tensor of CONNECTOR_DTYPE rows (updated in place), start the int32 /
    uint32 device array of row indices in connect-call order, gen the device ISN_GEN_DTYPE row (updated in place).
    Asynchronous on `stream` (default: the current stream), as connect_process and connect_timers are; the wrappers make
    no tensor of their own. Everything the caller passes in, `res` included, must be ready on `stream`: tensors made or
    filled on another stream need that stream waited for before the call."""
    s = _stream(stream, device)
    o = res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(N.load_library().dk_tcp_connect_start(
        _ptr(rows), _nrows(rows), _ptr(start), start.numel() if nstart is None else nstart, _ptr(gen), _ptr(links),
        links.numel() // N.TX_LINK_DTYPE.itemsize, now_ns, _ptr(out), out.numel() if out_bytes is None else out_bytes,
        ctypes.byref(lay), res.max_frames if max_frames is None else max_frames,
        res.max_ready if max_ready is None else max_ready, flags, ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)),
        "dk_tcp_connect_start")


def connect_process(rx: RxResults, rows, con_map, links, now_ns: int, out, res: ConnectResults, *, slot_stride: int,
                    frame_lead: int = 0, flags: int = 0, link=None, n: Optional[int] = None, out_bytes=None,
                    max_frames=None, max_ready=None, device: int = 0, stream=None) -> None:
    """dk_tcp_connect_process: `rx` are the results of the batch's receive_batch call (tcp_fields and tcp_opts on),
    con_map the int32 / uint32 device map flow_id -> connector row."""
    s = _stream(stream, device)
    r, o = rx.c_struct(), res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(N.load_library().dk_tcp_connect_process(
        ctypes.byref(r), rx.n if n is None else n, _ptr(rows), _nrows(rows), _ptr(con_map), con_map.numel(), _ptr(link),
        _ptr(links), links.numel() // N.TX_LINK_DTYPE.itemsize, now_ns, _ptr(out),
        out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
        res.max_frames if max_frames is None else max_frames, res.max_ready if max_ready is None else max_ready, flags,
        ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_tcp_connect_process")


def connect_timers(rows, links, now_ns: int, out, res: ConnectResults, *, slot_stride: int, frame_lead: int = 0,
                   flags: int = 0, out_bytes=None, max_frames=None, max_ready=None, device: int = 0,
                   stream=None) -> None:
    """dk_tcp_connect_timers: the handshake timeout over every row."""
    s = _stream(stream, device)
    o = res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(N.load_library().dk_tcp_connect_timers(
        _ptr(rows), _nrows(rows), _ptr(links), links.numel() // N.TX_LINK_DTYPE.itemsize, now_ns, _ptr(out),
        out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
        res.max_frames if max_frames is None else max_frames, res.max_ready if max_ready is None else max_ready, flags,
        ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_tcp_connect_timers")


def conn_rows_from_connect_ready(rec, connector_row, *, buffer_size: Optional[int] = None, link: Optional[int] = None):
    """The dk_tcp_conn (CONN_DTYPE) and dk_tcp_tx_conn (TX_CONN_DTYPE) rows of the connection a successful ready
    record describes, as EstablishedSocket::new sets them up: RCV.NXT = reader_next = rcv_nxt, SND.UNA = SND.NXT =
    snd_nxt, the send window = remote_window, the receive buffer = local_window unless given."""
    assert int(rec["err"]) == 0
    rx = np.zeros(1, N.CONN_DTYPE)
    rx["state"] = N.DK_TCP_ESTABLISHED
    rx["receive_next"] = rx["reader_next"] = rec["rcv_nxt"]
    rx["buffer_size"] = int(rec["local_window"]) if buffer_size is None else buffer_size
    rx["send_next"] = rec["snd_nxt"]
    tx = np.zeros(1, N.TX_CONN_DTYPE)
    tx["state"] = N.DK_TCP_ESTABLISHED
    tx["snd_una"] = tx["snd_nxt"] = rec["snd_nxt"]
    tx["snd_wnd"], tx["cwnd"], tx["mss"] = rec["remote_window"], 0xFFFFFFFF, rec["mss"]
    tx["rcv_nxt"], tx["rcv_wscale"] = rec["rcv_nxt"], rec["local_wscale"]
    tx["local_ip"], tx["remote_ip"] = connector_row["local_ip"], connector_row["remote_ip"]
    tx["ports"] = int(connector_row["local_port"]) | int(connector_row["remote_port"]) << 16
    tx["ip_word"] = connector_row["ip_word"]
    tx["link"] = connector_row["link"] if link is None else link
    tx["rcv_wnd_hdr"] = min(int(rx["buffer_size"][0]) >> int(rec["local_wscale"]), 0xFFFF)
    return rx, tx
