"""The receiver's ACKs on the GPU (include/dk_tcp.h, dk_tcp_ack_emit and dk_tcp_ack_timer).

What ControlBlock::process_packet decides per segment (tcp/established/ctrlblk.rs:403-440: an ACK at once, an ACK only
if one is already owed, or none, and what becomes of the delayed-ACK deadline) and ControlBlock::send_ack sends
(:712-720), for every connection of a batch at once: pure ACK frames of 54 bytes that carry RCV.NXT and the window as
they stood at the segment that triggered them. ack_emit follows TcpReceiver.process on the same batch, like
TcpAcker.process, in either order with it; ack_timer is the acknowledger's expiry for the connections the host names.
With them two endpoints run a whole transfer against each other with no frame built on the host.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import FrameBatch, RxResults, _check, _ptr
from .tcp import TcpOut, TcpReceiver
from .tcp_tx import TX_CONN_DTYPE, TcpSender

DACK_CONN_DTYPE = N.DACK_CONN_DTYPE
STATUSES = N.TCP_ACKEMIT_STATUSES
OK, E_STATE, E_SND_NXT, E_LINK, E_WSCALE, E_WINDOW, E_SLOT, NO_ROOM, NOT_FIRED, IDLE = range(10)
NO_FRAME = N.DK_TCP_ACKEMIT_NO_FRAME
ACK_FRAME_BYTES = 54
FORMS = N.DK_TCP_ACK_EMIT_FORMS


def dack_conn_table(nconns: int, *, delay_ns=40_000_000, armed=0, deadline_ns=0) -> np.ndarray:
    """Host table (DACK_CONN_DTYPE, 32-byte items): the delayed-ACK timer disarmed unless given, delay_ns =
    receive_ack_delay_timeout_secs. Scalars or per-connection arrays."""
    t = np.zeros(nconns, DACK_CONN_DTYPE)
    t["armed"] = np.asarray(armed, np.int64).astype(np.uint32)
    t["delay_ns"] = np.asarray(delay_ns, np.uint64)
    t["deadline_ns"] = np.asarray(deadline_ns, np.uint64)
    return t


def dack_to_device(table: np.ndarray, device: int = 0):
    import torch

    t = np.ascontiguousarray(table, DACK_CONN_DTYPE)
    return torch.from_numpy(t.view(np.uint8).copy()).to(torch.device("cuda", device))


def dack_to_host(dev) -> np.ndarray:
    return dev.cpu().numpy().view(DACK_CONN_DTYPE).copy()


class AckEmitResults:
    """Device outputs of one dk_tcp_ack_emit or dk_tcp_ack_timer call (dk_tcp_ackemit_results) for up to max_frames
    frames, nconns connections and n items (dk_tcp_ack_emit: the batch's frames; dk_tcp_ack_timer: the connections)."""

    def __init__(self, max_frames: int, nconns: int, n: Optional[int] = None, frame_conn: bool = True,
                 frame_seg: bool = True, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.max_frames, self.nconns, self.n = max_frames, nconns, nconns if n is None else n
        i32 = lambda k: torch.full((max(k, 1),), fill, dtype=torch.int32, device=dev)  # noqa: E731
        self.off_out = i32(max_frames)
        self.len_out = torch.full((max(max_frames, 1),), ((fill & 0xFFFF) ^ 0x8000) - 0x8000, dtype=torch.int16,
                                  device=dev)
        self.frame_conn = i32(max_frames) if frame_conn else None
        self.frame_seg = i32(max_frames) if frame_seg else None
        self.ack_frame = i32(self.n)
        self.status, self.n_acks = i32(nconns), i32(nconns)
        self.n_frames = i32(1)

    def c_struct(self) -> N.DkTcpAckEmitResults:
        return N.DkTcpAckEmitResults(*[_ptr(getattr(self, k)) for k in N.TCP_ACKEMIT_RESULT_FIELDS])

    def to_numpy(self) -> dict:
        """Host copies (synchronises). Per-frame arrays are cut to the frames written (none when the call ran out of
        room); n_frames is the call's need."""
        need = int(self.n_frames.cpu().numpy().view(np.uint32)[0])
        st = self.status.cpu().numpy().view(np.uint32)[:self.nconns]
        wrote = need if need <= self.max_frames and not (st == NO_ROOM).any() else 0
        h = {"n_frames": need, "frames_written": wrote, "status": st,
             "n_acks": self.n_acks.cpu().numpy().view(np.uint32)[:self.nconns],
             "ack_frame": self.ack_frame.cpu().numpy().view(np.uint32)[:self.n],
             "off_out": self.off_out.cpu().numpy().view(np.uint32)[:wrote],
             "len_out": self.len_out.cpu().numpy().view(np.uint16)[:wrote]}
        for k in ("frame_conn", "frame_seg"):
            if getattr(self, k) is not None:
                h[k] = getattr(self, k).cpu().numpy().view(np.uint32)[:wrote]
        return h


def ack_emit(receiver: TcpReceiver, rx: RxResults, tcp_out: TcpOut, rx_conns, tx_conns, dack, links, now_ns: int, out,
             res: AckEmitResults, *, slot_stride: int, frame_lead: int = 0, flags: int = 0, stream=None,
             form: Optional[str] = None, n: Optional[int] = None, out_bytes=None, max_frames=None) -> None:
    """dk_tcp_ack_emit on `receiver`'s context, after receiver.process(rx, rx_conns, tcp_out) on the same batch: the
    ACKs that batch's segments trigger as frames in `out` (frame f at f * slot_stride + frame_lead, numbered in the
    order of the batch frames that triggered them), asynchronously on `stream` (default: the current stream). rx_conns
    (CONN_DTYPE) and tx_conns (TX_CONN_DTYPE) are only read; dack (DACK_CONN_DTYPE, uint8 device tensor) is updated in
    place. form: a diagnostic override ("lane", "scan"; None = the engine's rule). Raises Fail(EINVAL) when it is not
    that call's turn."""
    import torch

    nconns = dack.numel() // DACK_CONN_DTYPE.itemsize
    assert tx_conns.numel() == nconns * TX_CONN_DTYPE.itemsize and rx_conns.numel() == nconns * N.CONN_DTYPE.itemsize
    n = rx.n if n is None else n
    assert res.n >= n and res.nconns >= nconns
    lib = receiver.lib
    _check(lib.dk_diag_tcp_ack_emit_set_form(receiver._ctx, FORMS[form] if form else -1), "dk_diag_tcp_ack_emit_set_form")
    s = stream if stream is not None else torch.cuda.current_stream(receiver.device)
    r, o = rx.c_struct(), res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(lib.dk_tcp_ack_emit(receiver._ctx, ctypes.byref(r), n, _ptr(tcp_out.action), _ptr(tcp_out.view),
                               _ptr(rx_conns), _ptr(tx_conns), _ptr(dack), nconns, _ptr(links),
                               links.numel() // N.TX_LINK_DTYPE.itemsize, now_ns, _ptr(out),
                               out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
                               res.max_frames if max_frames is None else max_frames, flags, ctypes.byref(o),
                               ctypes.c_void_p(s.cuda_stream)), "dk_tcp_ack_emit")


def last_form(receiver: TcpReceiver) -> Optional[str]:
    """The form the receiver's last ack_emit call ran (dk_diag_tcp_ack_emit_last_form)."""
    f = receiver.lib.dk_diag_tcp_ack_emit_last_form(receiver._ctx)
    return {v: k for k, v in FORMS.items()}.get(f)


def _batch(out, res: AckEmitResults, kw: dict, device) -> FrameBatch:
    import torch

    stream = kw.get("stream")
    (stream if stream is not None else torch.cuda.current_stream(device)).synchronize()
    need = int(res.n_frames.cpu().numpy().view(np.uint32)[0])
    cap = res.max_frames if kw.get("max_frames") is None else kw["max_frames"]
    ob = out.numel() if kw.get("out_bytes") is None else kw["out_bytes"]
    n = need if need <= cap and need * kw["slot_stride"] <= ob else 0
    batch = FrameBatch(out, res.off_out[:n], res.len_out[:n])
    batch.results = res
    return batch


def ack_emit_batch(receiver: TcpReceiver, rx: RxResults, tcp_out: TcpOut, rx_conns, tx_conns, dack, links, now_ns: int,
                   out, res: AckEmitResults, **kw) -> FrameBatch:
    """ack_emit(), then the frames it wrote as a FrameBatch over `out`, ready for the peer's RxEngine.receive_batch or
    a NIC ring. Reads n_frames back, so it waits for the call; an empty batch when the call ran out of room (res then
    says how many frames it needs)."""
    ack_emit(receiver, rx, tcp_out, rx_conns, tx_conns, dack, links, now_ns, out, res, **kw)
    return _batch(out, res, kw, receiver.device)


def ack_timer(sender: TcpSender, fire, tx_conns, rx_conns, dack, links, out, res: AckEmitResults, *, slot_stride: int,
              frame_lead: int = 0, flags: int = 0, stream=None, out_bytes=None, max_frames=None) -> None:
    """dk_tcp_ack_timer on `sender`'s context: for every connection c with fire[c] != 0 (uint8 device tensor; the host
    compares deadline_ns with its clock) whose delayed ACK is armed, one ACK from the tables as they stand, in
    connection order; armed becomes 0. res.ack_frame holds each connection's frame index."""
    import torch

    assert fire.dtype == torch.uint8 and fire.is_contiguous()
    nconns = fire.numel()
    assert tx_conns.numel() == nconns * TX_CONN_DTYPE.itemsize and rx_conns.numel() == nconns * N.CONN_DTYPE.itemsize
    assert dack.numel() == nconns * DACK_CONN_DTYPE.itemsize and res.nconns >= nconns and res.n >= nconns
    s = stream if stream is not None else torch.cuda.current_stream(sender.device)
    o = res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(sender.lib.dk_tcp_ack_timer(sender._ctx, _ptr(fire), _ptr(tx_conns), _ptr(rx_conns), _ptr(dack), nconns,
                                       _ptr(links), links.numel() // N.TX_LINK_DTYPE.itemsize, _ptr(out),
                                       out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
                                       res.max_frames if max_frames is None else max_frames, flags, ctypes.byref(o),
                                       ctypes.c_void_p(s.cuda_stream)), "dk_tcp_ack_timer")


def ack_timer_batch(sender: TcpSender, fire, tx_conns, rx_conns, dack, links, out, res: AckEmitResults,
                    **kw) -> FrameBatch:
    """ack_timer(), then the frames it wrote as a FrameBatch over `out` (waits for the call)."""
    ack_timer(sender, fire, tx_conns, rx_conns, dack, links, out, res, **kw)
    return _batch(out, res, kw, sender.device)
