"""The sender's reaction to ACKs on the GPU (include/dk_tcp.h, dk_tcp_ack_process).

What ControlBlock::process_ack hands to Sender::process_ack (tcp/established/ctrlblk.rs:607-650, sender.rs:406-508,
rto.rs:40-79) for every connection of a batch at once: SND.UNA and the send window move, the unacknowledged queue is
popped, its entries' transmit times feed the RTT estimate (f64, bit for bit), and the retransmit deadline follows the
queue's front. It follows TcpReceiver.process on the same batch and reuses that call's order by connection, so a
transfer's steady state is RxEngine.receive_batch -> TcpReceiver.process -> TcpAcker.process -> TcpSender.segment on
one stream with no per-segment array read by the host. Congestion control stays with the host: TcpAckOut.acked in
arrival order with new_acks / dup_acks is what on_ack_received needs.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import RxResults, _check, _ptr
from .tcp import TcpOut, TcpReceiver
from .tcp_tx import PushList, TcpTxResults

ACK_CONN_DTYPE = N.ACK_CONN_DTYPE
STATUSES = N.TCP_ACK_STATUSES
OK, E_STATE, E_SND_NXT, E_FLIGHT, E_WSCALE, E_WL2, E_QUEUE, E_DRY = range(8)
TX_TIME_NONE = N.DK_TCP_TX_TIME_NONE
TCP_HEADERS = 54  # Ethernet + IPv4 + TCP without options: what dk_tcp_tx_segment puts in front of a payload


def ack_conn_table(nconns: int, *, wl1=0, wl2=0, snd_wscale=0, q_first=0, q_count=0) -> np.ndarray:
    """Host table (ACK_CONN_DTYPE, 64-byte items): RtoCalculator::new() (srtt 1.0, rttvar 0.0, rto 1.0, no sample
    yet), the retransmit timer disarmed, empty queues unless given. Scalars or per-connection arrays."""
    t = np.zeros(nconns, ACK_CONN_DTYPE)
    u32 = lambda v: np.asarray(v, np.int64).astype(np.uint32)  # noqa: E731
    for k, v in (("wl1", wl1), ("wl2", wl2), ("snd_wscale", snd_wscale), ("q_first", q_first), ("q_count", q_count)):
        t[k] = u32(v)
    t["srtt"], t["rttvar"], t["rto"] = 1.0, 0.0, 1.0
    return t


def sync_send_next(rx_conns, tx_conns) -> None:
    """Copy snd_nxt of the TX table (TX_CONN_DTYPE, uint8 device tensor) into send_next of the RX table (CONN_DTYPE)
    on the device: dk_tcp_rx_process judges ack <= SND.NXT against the latter."""
    import torch

    rx = rx_conns.view(torch.int32).view(-1, N.CONN_DTYPE.itemsize // 4)
    tx = tx_conns.view(torch.int32).view(-1, N.TX_CONN_DTYPE.itemsize // 4)
    assert rx.shape[0] == tx.shape[0]
    rx[:, N.CONN_DTYPE.fields["send_next"][1] // 4] = tx[:, N.TX_CONN_DTYPE.fields["snd_nxt"][1] // 4]


class UnackedQueue:
    """The pool of unacknowledged-queue entries on the device (dk_tcp_unacked): `capacity` entries per connection,
    connection c's in pool[c * capacity, (c + 1) * capacity). Its live entries are pool[q_first, q_first + q_count) of
    the connection's dk_tcp_ack_conn."""

    def __init__(self, nconns: int, capacity: int, device: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.nconns, self.capacity, self.nq = nconns, capacity, nconns * capacity
        self.off = torch.zeros(max(self.nq, 1), dtype=torch.int32, device=dev)
        self.len = torch.zeros(max(self.nq, 1), dtype=torch.int32, device=dev)
        self.tx_time = torch.zeros(max(self.nq, 1), dtype=torch.int64, device=dev)

    @classmethod
    def from_numpy(cls, off, lens, tx_time, device: int = 0) -> "UnackedQueue":
        """A pool given whole (tests): one region, the tables' q_first index it directly."""
        import torch

        q = cls(1, len(off), device)
        dev = q.off.device
        if len(off):
            q.off = torch.from_numpy(np.ascontiguousarray(off, np.uint32).view(np.int32).copy()).to(dev)
            q.len = torch.from_numpy(np.ascontiguousarray(lens, np.uint32).view(np.int32).copy()).to(dev)
            q.tx_time = torch.from_numpy(np.ascontiguousarray(tx_time, np.uint64).view(np.int64).copy()).to(dev)
        return q

    def c_struct(self) -> N.DkTcpUnacked:
        return N.DkTcpUnacked(_ptr(self.off), _ptr(self.len), _ptr(self.tx_time))

    def to_numpy(self) -> dict:
        return {"off": self.off.cpu().numpy().view(np.uint32)[:self.nq],
                "len": self.len.cpu().numpy().view(np.uint32)[:self.nq],
                "tx_time": self.tx_time.cpu().numpy().view(np.uint64)[:self.nq]}

    def append_frames(self, ack_conns, res: TcpTxResults, push: PushList, now_ns: int, n_frames: int) -> None:
        """One entry per frame the TcpSender.segment call behind `res` sent (its first n_frames frames, e.g. the
        FrameBatch.n segment_batch returned), as Sender::send_segment pushes them (sender.rs:196-206): {the frame's
        bytes in the source blob, transmit time now_ns}; a FIN frame becomes the end-of-send marker (len 0); a disarmed
        retransmit timer is armed at now_ns. Every connection's live entries first move to the start of its region.
        Torch ops on the current stream; plumbing, not the hot path."""
        import torch

        assert res.frame_buf is not None, "append_frames needs TcpTxResults(frame_buf=True)"
        cap, nc = self.capacity, self.nconns
        ak = ack_conns.view(torch.int32).view(nc, ACK_CONN_DTYPE.itemsize // 4)
        col = lambda k: ACK_CONN_DTYPE.fields[k][1] // 4  # noqa: E731
        qf, qc = ak[:, col("q_first")].long(), ak[:, col("q_count")].long()
        dev = self.off.device
        # compact: entry j of connection c to c * cap + j
        j = torch.arange(cap, device=dev)[None, :]
        live = j < qc[:, None]
        src = (qf[:, None] + j).clamp_(max=max(self.nq - 1, 0))
        for name in ("off", "len", "tx_time"):
            t = getattr(self, name)
            moved = torch.where(live, t[src], torch.zeros((), dtype=t.dtype, device=dev))
            setattr(self, name, moved.reshape(-1).contiguous())
        f = torch.arange(n_frames, device=dev)
        buf = res.frame_buf[:n_frames].long()
        conn = push.conn.long()[buf]
        flen = (res.len_out[:n_frames].int() & 0xFFFF).long() - TCP_HEADERS
        first = res.first_frame.long()[buf]  # the buffer's first frame: its frames are consecutive
        before = torch.cumsum(flen, 0) - flen  # payload bytes of the frames before f
        within = before - before[first] if n_frames else before
        cnt = torch.bincount(conn, minlength=nc)
        start = torch.cumsum(cnt, 0) - cnt  # a connection's frames are consecutive too
        assert bool((qc + cnt <= cap).all()), "UnackedQueue: a connection's entries exceed its capacity"
        pos = conn * cap + qc[conn] + (f - start[conn])
        self.off[pos] = ((push.off.long()[buf] & 0xFFFFFFFF) + within).int()
        self.len[pos] = flen.int()
        self.tx_time[pos] = now_ns
        ak[:, col("q_first")] = (torch.arange(nc, device=dev) * cap).int()
        ak[:, col("q_count")] = (qc + cnt).int()
        arm = (ak[:, col("rtx_armed")] == 0) & (cnt > 0)
        ak[:, col("rtx_armed")] |= arm.int()
        base = ack_conns.view(torch.int64).view(nc, ACK_CONN_DTYPE.itemsize // 8)[:, ACK_CONN_DTYPE.fields["rtx_base_ns"][1] // 8]
        base[arm] = now_ns


class TcpAckOut:
    """Device outputs of one dk_tcp_ack_process call (dk_tcp_ack_out)."""

    def __init__(self, n: int, nconns: int, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.n, self.nconns = n, nconns
        self.acked = torch.full((max(n, 1),), fill, dtype=torch.int32, device=dev)
        for k in N.TCP_ACK_OUT_FIELDS[1:]:
            setattr(self, k, torch.full((max(nconns, 1),), fill, dtype=torch.int32, device=dev))

    def c_struct(self) -> N.DkTcpAckOut:
        return N.DkTcpAckOut(*[_ptr(getattr(self, k)) for k in N.TCP_ACK_OUT_FIELDS])

    def to_numpy(self) -> dict:
        h = {"acked": self.acked.cpu().numpy().view(np.uint32)[:self.n]}
        for k in N.TCP_ACK_OUT_FIELDS[1:]:
            h[k] = getattr(self, k).cpu().numpy().view(np.uint32)[:self.nconns]
        return h


class TcpAcker:
    """dk_tcp_ack_process over the context of a TcpReceiver: call process() right after receiver.process() on the
    same batch."""

    def __init__(self, form: Optional[str] = None):
        """form: a diagnostic override of the form ("lane", "wave", "chip"; None = the engine's rule), set
        through dk_diag_tcp_ack_set_form on the receiver's context at each call."""
        self.form = form

    @staticmethod
    def conns_to_device(table: np.ndarray, device: int = 0):
        import torch

        t = np.ascontiguousarray(table, ACK_CONN_DTYPE)
        return torch.from_numpy(t.view(np.uint8).copy()).to(torch.device("cuda", device))

    @staticmethod
    def conns_to_host(dev) -> np.ndarray:
        return dev.cpu().numpy().view(ACK_CONN_DTYPE).copy()

    @staticmethod
    def last_form(receiver: TcpReceiver) -> Optional[str]:
        f = receiver.lib.dk_diag_tcp_ack_last_form(receiver._ctx)
        return {v: k for k, v in N.DK_TCP_ACK_FORMS.items()}.get(f)

    def process(self, receiver: TcpReceiver, rx: RxResults, tcp_out: TcpOut, rx_conns, tx_conns, ack_conns,
                queue: UnackedQueue, now_ns: int, out: TcpAckOut, stream=None, n: Optional[int] = None) -> None:
        """The ACKs of the batch receiver.process(rx, rx_conns, tcp_out) just ran, applied to tx_conns (TX_CONN_DTYPE),
        ack_conns (ACK_CONN_DTYPE) and `queue`, all uint8 device tensors updated in place. Asynchronous on `stream`
        (default: the current stream). Raises Fail(EINVAL) when it is not that call's turn."""
        import torch

        nconns = ack_conns.numel() // ACK_CONN_DTYPE.itemsize
        assert tx_conns.numel() == nconns * N.TX_CONN_DTYPE.itemsize
        assert rx_conns.numel() == nconns * N.CONN_DTYPE.itemsize
        n = rx.n if n is None else n
        assert out.n >= n and out.nconns == nconns
        lib = receiver.lib
        _check(lib.dk_diag_tcp_ack_set_form(receiver._ctx, N.DK_TCP_ACK_FORMS[self.form] if self.form else -1),
               "dk_diag_tcp_ack_set_form")
        s = stream if stream is not None else torch.cuda.current_stream(receiver.device)
        r, o, q = rx.c_struct(), out.c_struct(), queue.c_struct()
        _check(lib.dk_tcp_ack_process(receiver._ctx, ctypes.byref(r), n, _ptr(tcp_out.action), _ptr(rx_conns),
                                      _ptr(tx_conns), _ptr(ack_conns), nconns, ctypes.byref(q), queue.nq, now_ns,
                                      ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_tcp_ack_process")
