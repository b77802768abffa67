"""Retransmission on the GPU (include/dk_tcp.h, dk_tcp_retransmit).

Sender::retransmit (tcp/established/sender.rs:375-403) and the timeout branch of background_retransmitter
(sender.rs:347-364, RtoCalculator::back_off) for every connection of a table at once: the front entry of each fired
connection's unacknowledged queue goes out again under fresh headers at SND.UNA, copied from the source blob and summed
in one pass; its tx_time becomes NONE (Karn), and a timeout doubles rto and restarts the timer at now_ns. The host names
who fires (`fire`: TIMEOUT for an expired deadline rtx_base_ns + rto, FAST for a connection its congestion control
flagged) and keeps congestion control; no payload byte comes back to it. With it the loop TcpSender.segment ->
UnackedQueue.append_frames -> TcpReceiver.process -> TcpAcker.process -> retransmit runs a lossy transfer on one stream.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .rx import FrameBatch, _check, _ptr
from .tcp_ack import ACK_CONN_DTYPE, UnackedQueue
from .tcp_tx import TX_CONN_DTYPE, TcpSender

STATUSES = N.TCP_RTX_STATUSES
NOT_FIRED, SENT, IDLE, E_FIRE, E_STATE, E_QUEUE, E_RANGE, E_SLOT, E_LINK, E_WINDOW, NO_ROOM = range(11)
FIRE_NONE, FIRE_TIMEOUT, FIRE_FAST = N.DK_TCP_RTX_NONE, N.DK_TCP_RTX_TIMEOUT, N.DK_TCP_RTX_FAST
NO_FRAME = N.DK_TCP_RTX_NO_FRAME


class RtxResults:
    """Device outputs of one dk_tcp_retransmit call (dk_tcp_rtx_results) for up to max_frames frames and nconns
    connections."""

    def __init__(self, max_frames: int, nconns: int, frame_conn: bool = True, device: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.max_frames, self.nconns = max_frames, nconns
        i32 = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=dev)  # noqa: E731
        self.off_out = i32(max_frames)
        self.len_out = torch.zeros(max(max_frames, 1), dtype=torch.int16, device=dev)
        self.frame_conn = i32(max_frames) if frame_conn else None
        self.status, self.frame = i32(nconns), i32(nconns)
        self.n_frames = i32(1)

    def c_struct(self) -> N.DkTcpRtxResults:
        return N.DkTcpRtxResults(*[_ptr(getattr(self, k)) for k in N.TCP_RTX_RESULT_FIELDS])

    def to_numpy(self) -> dict:
        """Host copies (synchronises). Per-frame arrays are cut to the frames written (none when the call ran out of
        room); n_frames is the call's need."""
        need = int(self.n_frames.cpu().numpy().view(np.uint32)[0])
        st = self.status.cpu().numpy().view(np.uint32)[:self.nconns]
        wrote = need if need <= self.max_frames and not (st == NO_ROOM).any() else 0
        h = {"n_frames": need, "frames_written": wrote, "status": st,
             "frame": self.frame.cpu().numpy().view(np.uint32)[:self.nconns],
             "off_out": self.off_out.cpu().numpy().view(np.uint32)[:wrote],
             "len_out": self.len_out.cpu().numpy().view(np.uint16)[:wrote]}
        if self.frame_conn is not None:
            h["frame_conn"] = self.frame_conn.cpu().numpy().view(np.uint32)[:wrote]
        return h


def fire_to_device(fire, device: int = 0):
    """A host array of dk_tcp_rtx_fire values as the uint8 device tensor dk_tcp_retransmit reads."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(fire, np.uint8).copy()).to(torch.device("cuda", device))


def retransmit(sender: TcpSender, src, fire, tx_conns, ack_conns, queue: UnackedQueue, now_ns: int, links, out,
               res: RtxResults, *, rx_conns=None, slot_stride: int, frame_lead: int = 0, flags: int = 0, stream=None,
               src_bytes=None, out_bytes=None, max_frames=None) -> None:
    """dk_tcp_retransmit on `sender`'s context: for every connection c with fire[c] != 0 (uint8 device tensor, one per
    connection) the front of its queue as a frame in `out` (frame f at f * slot_stride + frame_lead, in connection
    order), asynchronously on `stream` (default: the current stream). tx_conns (TX_CONN_DTYPE) and rx_conns (optional,
    CONN_DTYPE: ack number and window are then read from it) are only read; ack_conns (ACK_CONN_DTYPE) and the pool's
    tx_time are updated in place. flags: DK_TX_OFFLOAD_TCP writes the TCP checksum as 0. Results land in `res`."""
    import torch

    assert fire.dtype == torch.uint8 and fire.is_contiguous()
    nconns = fire.numel()
    assert tx_conns.numel() == nconns * TX_CONN_DTYPE.itemsize and ack_conns.numel() == nconns * ACK_CONN_DTYPE.itemsize
    assert rx_conns is None or rx_conns.numel() == nconns * N.CONN_DTYPE.itemsize
    assert res.nconns >= nconns
    s = stream if stream is not None else torch.cuda.current_stream(sender.device)
    q, r = queue.c_struct(), res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(sender.lib.dk_tcp_retransmit(
        sender._ctx, _ptr(src), src.numel() if src_bytes is None else src_bytes, _ptr(fire), _ptr(tx_conns),
        _ptr(ack_conns), nconns, _ptr(rx_conns), ctypes.byref(q), queue.nq, now_ns, _ptr(links),
        links.numel() // N.TX_LINK_DTYPE.itemsize, _ptr(out), out.numel() if out_bytes is None else out_bytes,
        ctypes.byref(lay), res.max_frames if max_frames is None else max_frames, flags, ctypes.byref(r),
        ctypes.c_void_p(s.cuda_stream)), "dk_tcp_retransmit")


def retransmit_batch(sender: TcpSender, src, fire, tx_conns, ack_conns, queue: UnackedQueue, now_ns: int, links, out,
                     res: RtxResults, **kw) -> FrameBatch:
    """retransmit(), then the frames it wrote as a FrameBatch over `out`, ready for RxEngine.receive_batch or a NIC
    ring. Reads n_frames back, so it waits for the call; an empty batch when the call ran out of room (res then says
    how many frames it needs)."""
    import torch

    retransmit(sender, src, fire, tx_conns, ack_conns, queue, now_ns, links, out, res, **kw)
    stream = kw.get("stream")
    (stream if stream is not None else torch.cuda.current_stream(sender.device)).synchronize()
    need = int(res.n_frames.cpu().numpy().view(np.uint32)[0])
    cap = res.max_frames if kw.get("max_frames") is None else kw["max_frames"]
    ob = out.numel() if kw.get("out_bytes") is None else kw["out_bytes"]
    n = need if need <= cap and need * kw["slot_stride"] <= ob else 0
    batch = FrameBatch(out, res.off_out[:n], res.len_out[:n])
    batch.results = res
    return batch
