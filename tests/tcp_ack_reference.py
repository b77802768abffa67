"""TEST INFRASTRUCTURE ONLY: a plain-Python restatement of the sender's reaction to ACKs, for the dk_tcp_ack_process
tests to compare against bit for bit.

    ControlBlock::process_ack                       layer4/tcp/established/ctrlblk.rs:607-650
    Sender::process_ack                             layer4/tcp/established/sender.rs:406-474
    update_retransmit_deadline, update_send_window  sender.rs:476-488, :490-508
    RtoCalculator::add_sample, update_rto           layer4/tcp/established/rto.rs:40-79
    SeqNumber comparisons                           sequence_number.rs (sign of the wrapping difference)

`ack_process` is literally that code, one segment at a time per connection: a deque for the unacknowledged queue,
Python floats (IEEE f64, no contraction) for the RTO state, u32 wrapping written out; plus dk_tcp_ack_process's batch
contract (include/dk_tcp.h): which segments get there, the connection-level failures, the outputs, the one deviation.
tests/test_tcp_ack_model.py pins this module against answers derived by hand.
"""
from __future__ import annotations

from collections import deque

import numpy as np

M32 = 0xFFFFFFFF
NONE = 0xFFFFFFFFFFFFFFFF  # DK_TCP_TX_TIME_NONE
ESTABLISHED = 1
OK, E_STATE, E_SND_NXT, E_FLIGHT, E_WSCALE, E_WL2, E_QUEUE, E_DRY = range(8)
# enum dk_tcp_action: the segments process_packet hands to process_ack and that pass its ack_num <= SND.NXT test
DELIVERED, STORED, STORE_DUP, NO_DATA, FIN = 1, 2, 3, 4, 5
PROCESSED = (DELIVERED, STORED, STORE_DUP, NO_DATA, FIN)


def seq_lt(a: int, b: int) -> bool:
    """SeqNumber a < b: the wrapping difference a - b, as i32, is negative."""
    return ((a - b) & M32) >= 0x80000000


def seq_le(a: int, b: int) -> bool:
    return a == b or seq_lt(a, b)


class Rto:
    """RtoCalculator (rto.rs)."""

    def __init__(self, srtt=1.0, rttvar=0.0, rto=1.0, received_sample=False):
        self.srtt, self.rttvar, self.rto, self.received_sample = float(srtt), float(rttvar), float(rto), bool(received_sample)

    def add_sample_ns(self, d: int) -> None:
        self.add_sample((d // 1000000000) + (d % 1000000000) / 1e9)  # Duration::as_secs_f64

    def add_sample(self, rtt: float) -> None:
        if not self.received_sample:
            self.srtt = rtt
            self.rttvar = rtt / 2.0
            self.received_sample = True
        else:
            self.rttvar = (1.0 - 0.25) * self.rttvar + 0.25 * abs(self.srtt - rtt)
            self.srtt = (1.0 - 0.125) * self.srtt + 0.125 * rtt
        rto = self.srtt + max(0.001, 4.0 * self.rttvar)
        self.rto = min(max(rto, 0.1), 60.0)


class Dry(Exception):
    """The queue ran dry with acknowledged bytes left: the reference spins there in release builds."""


class Sender:
    """The parts of Sender that process_ack touches. queue: deque of [off, len, tx_time]."""

    def __init__(self, una, nxt, wnd, wl1, wl2, wscale, rto: Rto, queue, armed, base):
        self.una, self.nxt, self.wnd, self.wl1, self.wl2, self.wscale = una, nxt, wnd, wl1, wl2, wscale
        self.rto, self.queue, self.armed, self.base = rto, queue, armed, base
        self.popped = self.samples = self.new_acks = self.dup_acks = 0

    def process_ack(self, seq: int, ack: int, win: int, now: int) -> int:
        """One segment (sender.rs:406-474); returns ctrlblk.rs:638's nbytes = ack - SND.UNA (wrapping)."""
        nbytes = (ack - self.una) & M32
        if ack == self.una:
            self.dup_acks += 1
        new = seq_lt(self.una, ack)
        if new and nbytes == 0x80000000 and self.una == self.nxt:
            new = False  # the deviation: the reference would spin on the empty queue
        if not new:
            return nbytes
        self.new_acks += 1
        remaining = nbytes
        while remaining != 0:
            if not self.queue:
                raise Dry()
            e = self.queue.popleft()
            self.popped += 1
            if e[2] != NONE:
                self.rto.add_sample_ns(max(now - e[2], 0))
                self.samples += 1
            if e[1] > remaining:
                e[0], e[1], e[2] = (e[0] + remaining) & M32, e[1] - remaining, NONE
                self.queue.appendleft(e)
                self.popped -= 1
                break
            if e[1] == 0:
                remaining = 0  # the end-of-send marker
            remaining -= e[1]
        self.una = ack
        if seq_lt(self.wl1, seq) or (self.wl1 == seq and seq_le(self.wl2, ack)):  # update_send_window
            self.wnd = (win << self.wscale) & M32
            self.wl1, self.wl2 = seq, ack
        if self.queue:  # update_retransmit_deadline: the host adds rto
            self.armed, self.base = 1, (self.queue[0][2] if self.queue[0][2] != NONE else now)
        else:
            self.armed, self.base = 0, 0
        return nbytes


def conn_status(tx, ak, rx, nq: int) -> int:
    una, nxt = int(tx["snd_una"]), int(tx["snd_nxt"])
    if int(tx["state"]) != ESTABLISHED:
        return E_STATE
    if int(rx["send_next"]) != nxt:
        return E_SND_NXT
    if ((nxt - una) & M32) >= 0x80000000:
        return E_FLIGHT
    if int(ak["snd_wscale"]) > 14:
        return E_WSCALE
    if 0 < ((int(ak["wl2"]) - una) & M32) < 0x80000000:
        return E_WL2
    if int(ak["q_first"]) + int(ak["q_count"]) > nq:
        return E_QUEUE
    return OK


def ack_process(flow_id, action, seq, ack, tcp_win, rx_conns, tx_conns, ack_conns, pool: dict, now_ns: int) -> dict:
    """dk_tcp_ack_process over host arrays. flow_id / action / seq / ack / tcp_win: [n], the batch's dk_rx results and
    dk_tcp_rx_process actions. pool: {"off", "len", "tx_time"} arrays. Returns copies of the tables and the pool as
    the call leaves them, and every output array."""
    n, nc = len(action), len(tx_conns)
    tx, ak = np.array(tx_conns, copy=True), np.array(ack_conns, copy=True)
    pool = {k: np.array(v, copy=True) for k, v in pool.items()}
    nq = len(pool["off"])
    acked = np.zeros(n, np.uint32)
    status, new_acks, dup_acks, bytes_acked, samples = (np.zeros(nc, np.uint32) for _ in range(5))
    segs = [[] for _ in range(nc)]
    for i in range(n):
        if int(action[i]) in PROCESSED:
            segs[int(flow_id[i])].append(i)
    for c in range(nc):
        status[c] = conn_status(tx[c], ak[c], rx_conns[c], nq)
        if status[c] != OK:
            continue
        a = ak[c]
        qf, qc = int(a["q_first"]), int(a["q_count"])
        queue = deque([int(pool["off"][e]), int(pool["len"][e]), int(pool["tx_time"][e])] for e in range(qf, qf + qc))
        rto = Rto(a["srtt"], a["rttvar"], a["rto"], a["received_sample"])
        s = Sender(int(tx[c]["snd_una"]), int(tx[c]["snd_nxt"]), int(tx[c]["snd_wnd"]), int(a["wl1"]), int(a["wl2"]),
                   int(a["snd_wscale"]), rto, queue, int(a["rtx_armed"]), int(a["rtx_base_ns"]))
        got = {}
        try:
            for i in segs[c]:
                got[i] = s.process_ack(int(seq[i]), int(ack[i]), int(tcp_win[i]) & 0xFFFF, now_ns)
        except Dry:
            status[c] = E_DRY
            continue
        for i, v in got.items():
            acked[i] = v
        new_acks[c], dup_acks[c], samples[c] = s.new_acks, s.dup_acks, s.samples
        bytes_acked[c] = (s.una - int(tx[c]["snd_una"])) & M32
        for t, fields in ((tx, dict(snd_una=s.una, snd_wnd=s.wnd)),
                          (ak, dict(wl1=s.wl1, wl2=s.wl2, received_sample=int(rto.received_sample), srtt=rto.srtt,
                                    rttvar=rto.rttvar, rto=rto.rto, q_first=qf + s.popped, q_count=len(queue),
                                    rtx_armed=s.armed, rtx_base_ns=s.base))):
            for k, v in fields.items():
                t[k][c] = v
        if queue:
            e = qf + s.popped
            pool["off"][e], pool["len"][e], pool["tx_time"][e] = queue[0]
    return {"tx_conns": tx, "ack_conns": ak, "pool": pool, "acked": acked, "status": status, "new_acks": new_acks,
            "dup_acks": dup_acks, "bytes_acked": bytes_acked, "samples": samples}
