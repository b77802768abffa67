"""Closing a connection on the GPU (include/dk_tcp.h, the dk_tcp_close_* section).

What ControlBlock::close does with local_close and remote_already_closed (tcp/established/ctrlblk.rs:1039-1119): the
state a close() call enters and the FIN marker it pushes, the close coroutine's loop over the segments that arrive
after poll() has returned (FIN-WAIT-1/2, CLOSING, LAST-ACK), the ACKs it sends and TIME-WAIT's end, for every closing
connection of one RxEngine.receive_batch call at once. The closing connections are rows of CLOSER_DTYPE in device
memory, indexed by flow id like the other TCP tables.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import RxResults, _check, _ptr
from .tcp_listen import _stream, to_device  # noqa: F401
from .tcp_tx import PushList

CLOSER_DTYPE, DONE_DTYPE = N.CLOSER_DTYPE, N.CLS_DONE_DTYPE
STATES, STATUSES, ACTION_BITS = N.TCP_CLS_STATES, N.TCP_CLS_STATUSES, N.TCP_CLS_ACTION_BITS
IDLE, FIN_WAIT_1, FIN_WAIT_2, CLOSING, TIME_WAIT, LAST_ACK, CLOSED, FAULT = range(8)
POPPED, ACK_OK, ACK_UNSENT, FIN, FAULT_BIT, UNPROCESSED = 1, 2, 4, 8, 16, 32
OK, E_ROW, E_ORDER, E_STATE, E_BADF, E_RX_STATE, E_LINK, E_WSCALE, E_WINDOW, E_SLOT, NO_ROOM = range(11)
NONE = N.DK_TCP_CLS_NONE
TIME_WAIT_NS = N.DK_TCP_CLS_TIME_WAIT_NS
RETIRED = N.DK_TCP_CLS_RETIRED
ACK_BYTES = N.DK_TCP_CLS_ACK_BYTES


def closer_table(nconns: int, **fields) -> np.ndarray:
    """Host table (CLOSER_DTYPE, 32-byte items), IDLE, linger_ns = 2 * MSL; scalars or per-row arrays override."""
    t = np.zeros(nconns, CLOSER_DTYPE)
    t["linger_ns"] = TIME_WAIT_NS
    for k, v in fields.items():
        t[k] = np.asarray(v).astype(CLOSER_DTYPE.fields[k][0])
    return t


def rows_to_host(dev) -> np.ndarray:
    return dev.cpu().numpy().view(CLOSER_DTYPE).copy()


class CloseResults:
    """Device outputs of one dk_tcp_close_process call (dk_tcp_cls_results) for n batch frames, up to max_frames ACKs
    and max_done done records, nconns rows; every array starts as `fill` bytes. dk_tcp_close_timers uses done, status
    and n_done of it."""

    def __init__(self, n: int, max_frames: int, max_done: int, nconns: int, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.n, self.max_frames, self.max_done, self.nconns = n, max_frames, max_done, nconns
        u8 = lambda k: torch.full((max(k, 4),), fill, dtype=torch.uint8, device=dev)  # noqa: E731
        self.action, self.state_after, self.ack_action = u8(n), u8(n), u8(n)
        self.reply_frame = u8(4 * n)
        self.off_out, self.len_out, self.frame_seg = u8(4 * max_frames), u8(2 * max_frames), u8(4 * max_frames)
        self.done = u8(DONE_DTYPE.itemsize * max_done)
        self.status, self.fin_frame = u8(4 * nconns), u8(4 * nconns)
        self.n_frames, self.n_done = u8(4), u8(4)

    def c_struct(self) -> N.DkTcpClsResults:
        return N.DkTcpClsResults(*[_ptr(getattr(self, k)) for k in N.TCP_CLS_RESULT_FIELDS])

    def raw(self) -> dict:
        """Every array whole, as bytes (for canary comparisons)."""
        return {k: getattr(self, k).cpu().numpy().copy() for k in N.TCP_CLS_RESULT_FIELDS}

    def to_numpy(self) -> dict:
        r = self.raw()
        u32 = lambda k, m: r[k][:4 * m].view(np.uint32)  # noqa: E731
        return {"action": r["action"][:self.n], "state_after": r["state_after"][:self.n],
                "ack_action": r["ack_action"][:self.n], "reply_frame": u32("reply_frame", self.n),
                "off_out": u32("off_out", self.max_frames), "len_out": r["len_out"][:2 * self.max_frames].view(np.uint16),
                "frame_seg": u32("frame_seg", self.max_frames),
                "done": r["done"][:DONE_DTYPE.itemsize * self.max_done].view(DONE_DTYPE),
                "status": u32("status", self.nconns), "fin_frame": u32("fin_frame", self.nconns),
                "n_frames": int(u32("n_frames", 1)[0]), "n_done": int(u32("n_done", 1)[0])}


def _nconns(rows) -> int:
    return rows.numel() // CLOSER_DTYPE.itemsize


class CloseStart:
    """What dk_tcp_close_start left: status per close[] entry, the padded marker list (a PushList for
    TcpSender.segment) and the word n_markers, all on the device."""

    def __init__(self, status, markers: PushList, n_markers):
        self.status, self.markers, self.n_markers = status, markers, n_markers

    def to_numpy(self) -> dict:
        u = lambda t: t.cpu().numpy().view(np.uint32).copy()  # noqa: E731
        return {"status": u(self.status), "conn": u(self.markers.conn), "off": u(self.markers.off),
                "len": u(self.markers.len), "n_markers": int(u(self.n_markers)[0])}


def close_start(rows, rx_conns, tx_conns, close, *, nclose: Optional[int] = None, fill: int = 0, device: int = 0,
                stream=None) -> CloseStart:
    """dk_tcp_close_start: rows / rx_conns / tx_conns uint8 device tensors of CLOSER_DTYPE / CONN_DTYPE / TX_CONN_DTYPE
    rows (the first two updated in place), close the int32 / uint32 device array of connections, strictly ascending.
    Returns the statuses and the marker list; nothing is read back. The returned tensors are made and filled on
    `stream` (default: the current stream), the stream the call runs on: a reader on another stream waits for `stream`
    first. What the caller passes in (here and in close_process / close_timers, their result objects included) must be
    ready on `stream`: tensors made or filled on another stream need that stream waited for before the call."""
    import torch

    s = _stream(stream, device)
    k = close.numel() if nclose is None else nclose
    i32 = lambda m: torch.full((4 * max(m, 1),), fill, dtype=torch.uint8,  # noqa: E731
                               device=torch.device("cuda", device)).view(torch.int32)
    with torch.cuda.stream(s):  # the fills are ordered before the call's stores, and the allocator knows the stream
        status, conn, off, lens, nm = i32(k), i32(k), i32(k), i32(k), i32(1)
    _check(N.load_library().dk_tcp_close_start(
        _ptr(rows), _ptr(rx_conns), _ptr(tx_conns), _nconns(rows), _ptr(close), k, _ptr(status), _ptr(conn), _ptr(off),
        _ptr(lens), _ptr(nm), ctypes.c_void_p(s.cuda_stream)), "dk_tcp_close_start")
    return CloseStart(status, PushList(conn, off, lens), nm)


def close_process(rx: RxResults, rows, rx_conns, tx_conns, links, now_ns: int, out, res: CloseResults, *,
                  slot_stride: int, frame_lead: int = 0, flags: int = 0, dack=None, action_in=None,
                  n: Optional[int] = None, out_bytes=None, max_frames=None, max_done=None, device: int = 0,
                  stream=None) -> None:
    """dk_tcp_close_process: `rx` are the results of the batch's receive_batch call (tcp_fields on), action_in that
    batch's dk_tcp_rx_process actions (optional), dack the DACK_CONN_DTYPE table (optional). res.ack_action is what
    dk_tcp_cc_ack and dk_tcp_ack_process take in place of those actions."""
    s = _stream(stream, device)
    r, o = rx.c_struct(), res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(N.load_library().dk_tcp_close_process(
        ctypes.byref(r), rx.n if n is None else n, _ptr(rows), _ptr(rx_conns), _ptr(tx_conns), _ptr(dack),
        _nconns(rows), _ptr(action_in), _ptr(links), links.numel() // N.TX_LINK_DTYPE.itemsize, now_ns, _ptr(out),
        out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
        res.max_frames if max_frames is None else max_frames, res.max_done if max_done is None else max_done, flags,
        ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_tcp_close_process")


def close_timers(rows, now_ns: int, res: CloseResults, *, tx_conns=None, max_done=None, device: int = 0,
                 stream=None) -> None:
    """dk_tcp_close_timers: TIME-WAIT's end and the retiring of closed rows; writes res.done, res.status, res.n_done."""
    s = _stream(stream, device)
    _check(N.load_library().dk_tcp_close_timers(
        _ptr(rows), _ptr(tx_conns), _nconns(rows), now_ns, _ptr(res.done),
        res.max_done if max_done is None else max_done, _ptr(res.n_done), _ptr(res.status),
        ctypes.c_void_p(s.cuda_stream)), "dk_tcp_close_timers")
