"""The send side's bookkeeping on the GPU (include/dk_tcp.h: dk_tcp_tx_commit, dk_tcp_rtx_piggyback).

The "post-send operations" of Sender::send_segment (tcp/established/sender.rs:195-206) and ControlBlock::emit
(ctrlblk.rs:761) for every connection of one TcpSender.segment call at once: each frame the call sent is pushed onto
its connection's unacknowledged queue with its transmit time, a disarmed retransmit timer is armed, and the delayed-ACK
deadline of a connection that sent anything is cancelled. tx_commit follows sender.segment on the same stream and
reads nothing back: n_frames stays on the device. rtx_piggyback is the same cancel after retransmit.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import _check, _ptr
from .tcp_ack import ACK_CONN_DTYPE, UnackedQueue
from .tcp_rtx import RtxResults
from .tcp_tx import PushList, TcpSender, TcpTxResults

STATUSES = N.TCP_COMMIT_STATUSES
OK, E_QUEUE, E_FULL = range(3)
FORMS = N.DK_TCP_COMMIT_FORMS


class CommitOut:
    """Device outputs of one dk_tcp_tx_commit call (dk_tcp_commit_out): status and appended per connection."""

    def __init__(self, nconns: int, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.nconns = nconns
        self.status = torch.full((max(nconns, 1),), fill, dtype=torch.int32, device=dev)
        self.appended = torch.full((max(nconns, 1),), fill, dtype=torch.int32, device=dev)

    def c_struct(self) -> N.DkTcpCommitOut:
        return N.DkTcpCommitOut(_ptr(self.status), _ptr(self.appended))

    def to_numpy(self) -> dict:
        return {k: getattr(self, k).cpu().numpy().view(np.uint32)[:self.nconns] for k in N.TCP_COMMIT_OUT_FIELDS}


def last_form(sender: TcpSender) -> Optional[str]:
    """The form the sender's last tx_commit ran ("conn", "chip"; None: none yet, or a call with no table rows)."""
    f = sender.lib.dk_diag_tcp_commit_last_form(sender._ctx)
    return {v: k for k, v in FORMS.items()}.get(f)


def tx_commit(sender: TcpSender, push: PushList, res: TcpTxResults, ack_conns, queue: UnackedQueue, now_ns: int,
              out: CommitOut, dack=None, form: Optional[str] = None, *, stream=None, nbufs: Optional[int] = None,
              max_frames: Optional[int] = None, nconns: Optional[int] = None) -> None:
    """dk_tcp_tx_commit on `sender`'s context, after sender.segment(.., push, .., res) on the same stream: the frames
    that call sent are appended to `queue` (connection c's region is [c * queue.capacity, (c + 1) * queue.capacity)),
    ack_conns (ACK_CONN_DTYPE, uint8 device tensor) gets q_first / q_count and a disarmed timer armed at now_ns, and
    with dack (DACK_CONN_DTYPE) armed is cleared for every connection that sent. form: a diagnostic override ("conn",
    "chip"; None = the engine's rule). Raises Fail(EINVAL) when it is not the call's turn."""
    import torch

    assert res.frame_buf is not None, "tx_commit needs TcpTxResults(frame_buf=True)"
    nc = ack_conns.numel() // ACK_CONN_DTYPE.itemsize if nconns is None else nconns
    assert dack is None or dack.numel() >= nc * N.DACK_CONN_DTYPE.itemsize
    assert out.nconns >= nc
    _check(sender.lib.dk_diag_tcp_commit_set_form(sender._ctx, FORMS[form] if form else -1),
           "dk_diag_tcp_commit_set_form")
    s = stream if stream is not None else torch.cuda.current_stream(sender.device)
    p, r, q, o = push.c_struct(), res.c_struct(), queue.c_struct(), out.c_struct()
    _check(sender.lib.dk_tcp_tx_commit(sender._ctx, ctypes.byref(p), push.n if nbufs is None else nbufs, ctypes.byref(r),
                                       res.max_frames if max_frames is None else max_frames, _ptr(ack_conns), nc,
                                       ctypes.byref(q), queue.nq, queue.capacity, _ptr(dack), now_ns, ctypes.byref(o),
                                       ctypes.c_void_p(s.cuda_stream)), "dk_tcp_tx_commit")


def rtx_piggyback(sender: TcpSender, rres: RtxResults, dack, *, stream=None) -> None:
    """dk_tcp_rtx_piggyback on `sender`'s context: dack[c].armed = 0 for every connection the retransmit call behind
    `rres` built a frame for (status SENT). Idempotent."""
    import torch

    nconns = dack.numel() // N.DACK_CONN_DTYPE.itemsize
    assert rres.nconns >= nconns
    s = stream if stream is not None else torch.cuda.current_stream(sender.device)
    r = rres.c_struct()
    _check(sender.lib.dk_tcp_rtx_piggyback(sender._ctx, ctypes.byref(r), _ptr(dack), nconns,
                                           ctypes.c_void_p(s.cuda_stream)), "dk_tcp_rtx_piggyback")
