"""Congestion control and timer expiry on the GPU (include/dk_tcp.h: dk_tcp_cc_ack, dk_tcp_timers, dk_tcp_cc_send).

CUBIC as tcp/established/congestion_control/cubic.rs states it, for every connection of a table at once: cc_ack is
on_ack_received over a batch (it follows TcpReceiver.process and precedes TcpAcker.process on the same batch), timers
names the connections whose retransmit deadline or fast-retransmit flag fires (running on_rto / on_fast_retransmit) and
whose delayed ACK is due, and cc_send is the pair of hooks around TcpSender.segment. With them a lossy transfer runs
cc_send(before) -> segment -> tx_commit (tcp_commit.py) -> cc_send(after) -> rx -> cc_ack -> ack_process -> ack_emit
-> timers -> retransmit / ack_timer with the host advancing only its clock: it fills no fire[] and no cwnd.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import RxResults, _check, _ptr
from .tcp import TcpOut, TcpReceiver
from .tcp_tx import PushList, TcpSender, TcpTxResults

CC_CONN_DTYPE = N.CC_CONN_DTYPE
STATUSES = N.TCP_CC_STATUSES
OK, E_STATE, E_SND_NXT, E_MSS, E_RTO = range(5)
CUBIC, FAST_CONVERGENCE, IN_RECOVERY, LAST_WAS_RTO, RETRANSMIT_NOW = 1, 2, 4, 8, 16
BEFORE_SEND, AFTER_SEND = N.DK_TCP_CC_BEFORE_SEND, N.DK_TCP_CC_AFTER_SEND


def cc_conn_table(nconns: int, *, mss, seq_no=0, now_ns=0, cubic=True, fast_convergence=True) -> np.ndarray:
    """Host table (CC_CONN_DTYPE, 64-byte items) as Cubic::new leaves it (cubic.rs:66-100): cwnd = initial_cwnd = 4 / 3 /
    2 x mss (mss <= 1095 / <= 2190 / above), ssthresh 0xFFFFFFFF, w_max 0, rtt_at_last_send 1 s, recover = prev_ack =
    seq_no (the initial send sequence number), ca_start = last_send = now_ns. cubic=False gives the algorithm None: a
    zero row. Scalars or per-connection arrays."""
    t = np.zeros(nconns, CC_CONN_DTYPE)
    mss = np.broadcast_to(np.asarray(mss, np.int64), (nconns,))
    on = np.broadcast_to(np.asarray(cubic, bool), (nconns,))
    fc = np.broadcast_to(np.asarray(fast_convergence, bool), (nconns,))
    init = (np.where(mss <= 1095, 4, np.where(mss <= 2190, 3, 2)) * mss).astype(np.uint32)
    seq = np.broadcast_to(np.asarray(seq_no, np.int64).astype(np.uint32), (nconns,))
    t["flags"] = np.where(on, CUBIC | np.where(fc, FAST_CONVERGENCE, 0), 0)
    t["cwnd"] = t["initial_cwnd"] = np.where(on, init, 0)
    t["ssthresh"] = np.where(on, 0xFFFFFFFF, 0)
    t["recover"] = t["prev_ack"] = np.where(on, seq, 0)
    t["ca_start_ns"] = t["last_send_ns"] = np.where(on, np.asarray(now_ns, np.uint64), 0)
    t["rtt_at_last_send_ns"] = np.where(on, 10**9, 0)
    return t


def cc_to_device(table: np.ndarray, device: int = 0):
    import torch

    t = np.ascontiguousarray(table, CC_CONN_DTYPE)
    return torch.from_numpy(t.view(np.uint8).copy()).to(torch.device("cuda", device))


def cc_to_host(dev) -> np.ndarray:
    return dev.cpu().numpy().view(CC_CONN_DTYPE).copy()


def rto_ns(rto: float) -> int:
    """dk_tcp_rto_ns: Duration::from_secs_f64(rto) in nanoseconds, the code the kernels run, on the host."""
    return int(N.load_library().dk_tcp_rto_ns(rto))


class CcAckOut:
    """Device outputs of one dk_tcp_cc_ack call (dk_tcp_cc_ack_out)."""

    def __init__(self, n: int, nconns: int, cwnd_after: bool = True, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.n, self.nconns = n, nconns
        i32 = lambda k: torch.full((max(k, 1),), fill, dtype=torch.int32, device=dev)  # noqa: E731
        self.status, self.new_acks, self.dup_acks = i32(nconns), i32(nconns), i32(nconns)
        self.cwnd_after = i32(n) if cwnd_after else None

    def c_struct(self) -> N.DkTcpCcAckOut:
        return N.DkTcpCcAckOut(*[_ptr(getattr(self, k)) for k in N.TCP_CC_ACK_OUT_FIELDS])

    def to_numpy(self) -> dict:
        h = {k: getattr(self, k).cpu().numpy().view(np.uint32)[:self.nconns] for k in N.TCP_CC_ACK_OUT_FIELDS[:3]}
        if self.cwnd_after is not None:
            h["cwnd_after"] = self.cwnd_after.cpu().numpy().view(np.uint32)[:self.n]
        return h


class TimersOut:
    """Device outputs of one dk_tcp_timers call: rtx_fire / ack_fire (uint8, the fire[] of retransmit / ack_timer),
    status, and the three counts."""

    def __init__(self, nconns: int, ack_fire: bool = True, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.nconns = nconns
        self.rtx_fire = torch.full((max(nconns, 1),), fill & 0xFF, dtype=torch.uint8, device=dev)[:nconns]
        self.ack_fire = torch.full((max(nconns, 1),), fill & 0xFF, dtype=torch.uint8, device=dev)[:nconns] if ack_fire else None
        self.status = torch.full((max(nconns, 1),), fill, dtype=torch.int32, device=dev)
        self.counts = torch.full((3,), fill, dtype=torch.int32, device=dev)  # n_fast, n_timeout, n_ack

    def c_struct(self) -> N.DkTcpTimersOut:
        base, p = self.counts.data_ptr(), ctypes.c_void_p
        return N.DkTcpTimersOut(_ptr(self.status), p(base), p(base + 4), p(base + 8))

    def to_numpy(self) -> dict:
        n_fast, n_timeout, n_ack = (int(v) for v in self.counts.cpu().numpy().view(np.uint32))
        h = {"status": self.status.cpu().numpy().view(np.uint32)[:self.nconns], "rtx_fire": self.rtx_fire.cpu().numpy(),
             "n_fast": n_fast, "n_timeout": n_timeout, "n_ack": n_ack}
        if self.ack_fire is not None:
            h["ack_fire"] = self.ack_fire.cpu().numpy()
        return h


def _nconns(cc, tx_conns, ack_conns) -> int:
    nconns = cc.numel() // CC_CONN_DTYPE.itemsize
    assert tx_conns.numel() == nconns * N.TX_CONN_DTYPE.itemsize and ack_conns.numel() == nconns * N.ACK_CONN_DTYPE.itemsize
    return nconns


def cc_ack(receiver: TcpReceiver, rx: RxResults, tcp_out: TcpOut, rx_conns, tx_conns, ack_conns, cc, now_ns: int,
           out: CcAckOut, *, stream=None, n: Optional[int] = None) -> None:
    """dk_tcp_cc_ack on `receiver`'s context, after receiver.process(rx, rx_conns, tcp_out) and before TcpAcker.process
    on the same batch: on_ack_received for every segment that reaches process_ack, per connection in arrival order.
    cc (CC_CONN_DTYPE, uint8 device tensor) and tx_conns' cwnd are updated in place; rx_conns and ack_conns are only
    read. Raises Fail(EINVAL) when it is not that call's turn."""
    import torch

    nconns = _nconns(cc, tx_conns, ack_conns)
    assert rx_conns.numel() == nconns * N.CONN_DTYPE.itemsize
    n = rx.n if n is None else n
    assert out.n >= n and out.nconns >= nconns
    s = stream if stream is not None else torch.cuda.current_stream(receiver.device)
    r, o = rx.c_struct(), out.c_struct()
    _check(receiver.lib.dk_tcp_cc_ack(receiver._ctx, ctypes.byref(r), n, _ptr(tcp_out.action), _ptr(rx_conns),
                                      _ptr(tx_conns), _ptr(ack_conns), _ptr(cc), nconns, now_ns, ctypes.byref(o),
                                      ctypes.c_void_p(s.cuda_stream)), "dk_tcp_cc_ack")


def timers(sender: TcpSender, tx_conns, ack_conns, cc, now_ns: int, out: TimersOut, *, dack=None, stream=None) -> None:
    """dk_tcp_timers on `sender`'s context: out.rtx_fire[c] = FAST for a connection whose fast_retransmit_now flag is
    set (cleared), TIMEOUT for one whose armed retransmit deadline rtx_base_ns + rto has passed (on_rto runs), else 0:
    the fire[] of retransmit, which follows on the same stream. With dack (DACK_CONN_DTYPE, only read) out.ack_fire is
    the fire[] of ack_timer. The counts let the host skip those calls."""
    import torch

    nconns = _nconns(cc, tx_conns, ack_conns)
    assert out.nconns >= nconns and (dack is None or out.ack_fire is not None)
    assert dack is None or dack.numel() == nconns * N.DACK_CONN_DTYPE.itemsize
    s = stream if stream is not None else torch.cuda.current_stream(sender.device)
    o = out.c_struct()
    _check(sender.lib.dk_tcp_timers(sender._ctx, _ptr(tx_conns), _ptr(ack_conns), _ptr(cc), _ptr(dack), nconns, now_ns,
                                    _ptr(out.rtx_fire), _ptr(out.ack_fire) if dack is not None else None,
                                    ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_tcp_timers")


def cc_send(sender: TcpSender, phase: int, tx_conns, ack_conns, cc, now_ns: int, status, *,
            push: Optional[PushList] = None, res: Optional[TcpTxResults] = None, stream=None) -> None:
    """dk_tcp_cc_send on `sender`'s context. phase BEFORE_SEND: the idle restart of on_cwnd_check_before_send, then
    tx_conns' cwnd refreshed, before sender.segment. phase AFTER_SEND, with that segment call's push and res: on_send
    for every frame it sent. status: int32 device tensor [nconns]."""
    import torch

    nconns = _nconns(cc, tx_conns, ack_conns)
    assert status.dtype == torch.int32 and status.numel() >= nconns
    assert phase == BEFORE_SEND or (push is not None and res is not None)
    s = stream if stream is not None else torch.cuda.current_stream(sender.device)
    p = push.c_struct() if push is not None else None
    r = res.c_struct() if res is not None else None
    _check(sender.lib.dk_tcp_cc_send(sender._ctx, phase, _ptr(tx_conns), _ptr(ack_conns), _ptr(cc), nconns,
                                     ctypes.byref(p) if p is not None else None, push.n if push is not None else 0,
                                     ctypes.byref(r) if r is not None else None, now_ns, _ptr(status),
                                     ctypes.c_void_p(s.cuda_stream)), "dk_tcp_cc_send")


def device_cbrt(x: np.ndarray, device: int = 0) -> np.ndarray:
    """The device's correctly rounded f32 cube root (dk_diag_tcp_cc_cbrt) of a float32 array."""
    import torch

    dev = torch.device("cuda", device)
    a = torch.from_numpy(np.ascontiguousarray(x, np.float32).copy()).to(dev)
    b = torch.zeros_like(a)
    s = torch.cuda.current_stream(dev)
    _check(N.load_library().dk_diag_tcp_cc_cbrt(_ptr(a), _ptr(b), a.numel(), ctypes.c_void_p(s.cuda_stream)),
           "dk_diag_tcp_cc_cbrt")
    return b.cpu().numpy()
