"""A connection's end as a closed loop on the MI355X: two endpoints on the device, each side's output blob the other
side's receive batch. No frame is built or parsed on the host to drive the loop: the host advances the clock, chooses
which batches are lost, and reads the frames back afterwards for the trace. Per received batch:
dk_rx_process, dk_tcp_rx_process, dk_tcp_close_process, then dk_tcp_cc_ack and dk_tcp_ack_process with the close call's
ack_action, and dk_tcp_ack_emit with the receive call's own action; close() is dk_tcp_close_start, whose marker list goes
to dk_tcp_tx_segment and dk_tcp_tx_commit unread; the clocks run dk_tcp_timers, dk_tcp_retransmit, dk_tcp_ack_timer and
dk_tcp_close_timers.

  (a) 1,000 bytes from A to B, then A closes (FIN_WAIT_1, FIN_WAIT_2, TIME_WAIT) and B, which met the FIN in
      ESTABLISHED, closes through LAST_ACK.
  (b) the simultaneous close of close-simultaneous.pkt: B's pure ACK of A's FIN is lost, so B's own FIN, which
      acknowledges A's, finds A in FIN_WAIT_1 and takes it to TIME_WAIT in one frame. (Two FINs that cross with neither
      acknowledging the other leave both ends in TIME_WAIT with their FIN unacknowledged, in the reference as here: no
      coroutine pops recv_queue any more. That ending cannot meet the conditions below and is not a scenario.)
  (c) as (a), with A's first FIN lost and resent by the retransmission timer.
Each ends with both rows CLOSED after dk_tcp_close_timers, both unacknowledged queues empty, the retransmit timers
disarmed, both tx states DK_TCP_CLOSED, and the frame trace the one the reference's behaviour gives (the expected traces
below are written out by hand from ctrlblk.rs, in the scripts' notation, relative to the two initial sequence numbers)."""
import numpy as np
import pytest

import tx_segment_reference as M
from demikernel_amd import (AckEmitResults, CcAckOut, CommitOut, Config, FrameBatch, PushList, RxEngine, SocketId, TcpAcker,
                            TcpAckOut, TcpSender, TcpTxResults, TimersOut, UnackedQueue, ack_conn_table, ack_emit_batch,
                            cc_ack, cc_conn_table, dack_conn_table, flow_array, sync_send_next, synth, timers, tx_commit)
from demikernel_amd import _native as N
from demikernel_amd import tcp_close as TCL
from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table
from demikernel_amd.tcp_ackemit import ack_timer_batch, dack_to_device
from demikernel_amd.tcp_cc import cc_to_device
from demikernel_amd.tcp_rtx import RtxResults, retransmit_batch

pytestmark = pytest.mark.gpu

NC, MSS, BUFFER, DELAY, LINGER = 2, 1000, 60000, 40_000_000, 3_000_000_000
A_IP, B_IP, B_PORT = synth.ALICE_IPV4, synth.BOB_IPV4, 12345
FIN, PSH, ACK = 0x01, 0x08, 0x10
STRIDE = 1088


class Actions:
    """What dk_tcp_cc_ack and dk_tcp_ack_process take in place of the receive call's outputs: only `action` is read."""

    def __init__(self, action):
        self.action = action


class Endpoint:
    def __init__(self, name, ip, flows_here, flows_there, snd, rcv, link, now):
        import torch

        self.name, self.dev = name, torch.device("cuda", 0)
        self.snd, self.eng, self.tcp, self.acker = TcpSender(0), RxEngine(Config(ip), device=0), TcpReceiver(0), TcpAcker()
        self.eng.set_sockets(flows_here)
        self.d_tx = self.snd.conns_to_device(M.conns_toward(flows_there, snd_nxt=snd, snd_una=snd, rcv_nxt=rcv,
                                                            snd_wnd=65535, mss=MSS, link=link, rcv_wscale=0))
        self.d_ak = TcpAcker.conns_to_device(ack_conn_table(NC, wl1=rcv, wl2=snd))
        self.d_rx = self.tcp.conns_to_device(conn_table(NC, receive_next=rcv, send_next=snd, buffer_size=BUFFER))
        self.d_cc = cc_to_device(cc_conn_table(NC, mss=MSS, seq_no=snd, now_ns=now))
        self.d_dack = dack_to_device(dack_conn_table(NC, delay_ns=DELAY))
        self.d_cls = TCL.to_device(TCL.closer_table(NC, linger_ns=LINGER))
        self.queue = UnackedQueue(NC, 4)
        self.d_links = torch.from_numpy(np.ascontiguousarray(M.links_table()).view(np.uint8).copy()).to(self.dev)
        self.d_src = torch.arange(4096, dtype=torch.int32, device=self.dev).to(torch.uint8)
        self.sent = []  # every frame this end put on the wire, as (blob, offsets, lengths) still on the device

    def close_all(self):
        for o in (self.snd, self.eng, self.tcp):
            o.close()

    def blob(self, slots, stride=64):
        import torch

        return torch.zeros(max(slots, 1) * stride, dtype=torch.uint8, device=self.dev)

    def put(self, batch):
        if batch.n:
            self.sent.append(batch)
        return batch

    def push(self, push, now):
        """dk_tcp_tx_segment and dk_tcp_tx_commit over a push list that is already on the device."""
        res = TcpTxResults(push.n, push.n)
        batch = self.snd.segment_batch(self.d_src, push, self.d_tx, self.d_links, self.blob(push.n, STRIDE), res,
                                       slot_stride=STRIDE, rx_conns=self.d_rx)
        cout = CommitOut(NC)
        tx_commit(self.snd, push, res, self.d_ak, self.queue, now, cout, dack=self.d_dack)
        assert not cout.to_numpy()["status"].any()
        return self.put(batch)

    def close(self, now):
        """close() on every connection: the marker list goes from dk_tcp_close_start to the send path unread."""
        import torch

        conns = torch.arange(NC, dtype=torch.int32, device=self.dev)
        s = TCL.close_start(self.d_cls, self.d_rx, self.d_tx, conns)
        batch = self.push(s.markers, now)
        assert list(s.to_numpy()["status"]) == [TCL.OK] * NC and batch.n == NC
        return batch

    def receive(self, batch, now):
        """One received batch through every call of the loop -> (dk_tcp_ack_emit's ACKs, dk_tcp_close_process's ACKs)."""
        import torch

        n = batch.n
        sync_send_next(self.d_rx, self.d_tx)
        r = self.eng.results(n, tcp_fields=True)
        self.eng.receive_batch(batch, r)
        out = TcpOut(n, NC)
        self.tcp.process(r, self.d_rx, out)
        cres = TCL.CloseResults(n, 2 * n, n, NC)
        cblob = self.blob(2 * n)
        TCL.close_process(r, self.d_cls, self.d_rx, self.d_tx, self.d_links, now, cblob, cres, slot_stride=64,
                          dack=self.d_dack, action_in=out.action)
        handed = Actions(cres.ack_action)
        cout, aout = CcAckOut(n, NC), TcpAckOut(n, NC)
        cc_ack(self.tcp, r, handed, self.d_rx, self.d_tx, self.d_ak, self.d_cc, now, cout)
        self.acker.process(self.tcp, r, handed, self.d_rx, self.d_tx, self.d_ak, self.queue, now, aout)
        ares = AckEmitResults(n, NC, n)
        acks = ack_emit_batch(self.tcp, r, out, self.d_rx, self.d_tx, self.d_dack, self.d_links, now, self.blob(n), ares,
                              slot_stride=64)
        torch.cuda.synchronize()
        c = cres.to_numpy()
        assert not c["status"].any() and not cout.to_numpy()["status"].any() and not aout.to_numpy()["status"].any()
        assert not ares.to_numpy()["status"].any()
        nf = c["n_frames"]
        closing = FrameBatch(cblob, cres.off_out.view(torch.int32)[:nf], cres.len_out.view(torch.int16)[:nf])
        self.last = c
        return self.put(acks), self.put(closing)

    def clock(self, now):
        """dk_tcp_timers, then dk_tcp_retransmit and dk_tcp_ack_timer as its counts say -> (resent frames, ACKs)."""
        tout = TimersOut(NC)
        timers(self.snd, self.d_tx, self.d_ak, self.d_cc, now, tout, dack=self.d_dack)
        t = tout.to_numpy()
        assert not t["status"].any()
        rtx = acks = None
        if t["n_fast"] + t["n_timeout"]:
            rtx = self.put(retransmit_batch(self.snd, self.d_src, tout.rtx_fire, self.d_tx, self.d_ak, self.queue, now,
                                            self.d_links, self.blob(NC, STRIDE), RtxResults(NC, NC), rx_conns=self.d_rx,
                                            slot_stride=STRIDE))
        if t["n_ack"]:
            acks = self.put(ack_timer_batch(self.snd, tout.ack_fire, self.d_tx, self.d_rx, self.d_dack, self.d_links,
                                            self.blob(NC), AckEmitResults(NC, NC), slot_stride=64))
        return rtx, acks

    def close_timers(self, now):
        res = TCL.CloseResults(0, 0, NC, NC)
        TCL.close_timers(self.d_cls, now, res, tx_conns=self.d_tx)
        return res.to_numpy()

    def rows(self):
        return [int(s) for s in TCL.rows_to_host(self.d_cls)["state"]]

    def trace(self, conn_port):
        """The frames this end sent on the connection whose local or remote port is conn_port, in order, read back."""
        out = []
        for b in self.sent:
            blob, off, ln = b.blob.cpu().numpy(), b.off.cpu().numpy().view(np.uint32), b.len.cpu().numpy().view(np.uint16)
            for o, l in zip(off, ln):
                f = blob[int(o):int(o) + int(l)].tobytes()
                if conn_port in (int.from_bytes(f[34:36], "big"), int.from_bytes(f[36:38], "big")):
                    out.append((f[47], int.from_bytes(f[38:42], "big"), int.from_bytes(f[42:46], "big"), int(l) - 54,
                                int.from_bytes(f[48:50], "big")))
        return out


@pytest.fixture
def ends():
    rng = np.random.default_rng(5)
    a_port = [40000 + c for c in range(NC)]
    flows_b = flow_array([SocketId.Active((B_IP, B_PORT), (A_IP, a_port[c])) for c in range(NC)])  # at B
    flows_a = flow_array([SocketId.Active((A_IP, a_port[c]), (B_IP, B_PORT)) for c in range(NC)])  # at A
    ia = np.array([0xFFFFFE00, int(rng.integers(0, 1 << 32))], np.uint32)  # connection 0's sequence numbers wrap
    ib = np.array([0xFFFFFFFF, int(rng.integers(0, 1 << 32))], np.uint32)
    now = 10**9
    a = Endpoint("A", A_IP, flows_a, flows_b, ia, ib, 0, now)
    b = Endpoint("B", B_IP, flows_b, flows_a, ib, ia, 1, now)
    yield a, b, ia, ib, a_port
    a.close_all()
    b.close_all()


def finish(a, b, now, ia, ib, a_port, expect_a, expect_b):
    """The end every scenario shares: LAST_ACK's end is retired at once, TIME-WAIT after the linger; then the four
    conditions and the trace."""
    assert a.rows() == [TCL.TIME_WAIT] * NC and b.rows() == [TCL.CLOSED] * NC
    tw = now
    yb = b.close_timers(now)
    assert yb["n_done"] == NC and b.close_timers(now)["n_done"] == 0  # retired exactly once
    assert a.close_timers(tw + LINGER - 1)["n_done"] == 0 and a.rows() == [TCL.TIME_WAIT] * NC
    ya = a.close_timers(tw + LINGER)
    assert ya["n_done"] == NC and a.rows() == [TCL.CLOSED] * NC and b.rows() == [TCL.CLOSED] * NC
    for e in (a, b):
        ak = TcpAcker.conns_to_host(e.d_ak)
        tx = e.snd.conns_to_host(e.d_tx)
        assert not ak["q_count"].any() and not ak["rtx_armed"].any(), e.name
        assert (tx["state"] == N.DK_TCP_CLOSED).all() and (tx["snd_una"] == tx["snd_nxt"]).all(), e.name
    M32 = 0xFFFFFFFF
    for c in range(NC):
        A0, B0 = int(ia[c]), int(ib[c])
        rel = lambda tr, s0, r0: [(fl, (s - s0) & M32, (k - r0) & M32, ln, w) for fl, s, k, ln, w in tr]  # noqa: E731
        assert rel(a.trace(a_port[c]), A0, B0) == expect_a, (c, rel(a.trace(a_port[c]), A0, B0))
        assert rel(b.trace(a_port[c]), B0, A0) == expect_b, (c, rel(b.trace(a_port[c]), B0, A0))


def transfer_then_close(a, b, now, lose_first_fin):
    """(a) and (c) up to B's close()."""
    data = a.push(PushList.from_numpy(np.arange(NC), np.zeros(NC, np.int64), np.full(NC, 1000)), now)
    now += 1_000_000
    acks, closing = b.receive(data, now)
    assert acks.n == 0 and closing.n == 0  # delivered; the ACK is delayed
    now += DELAY
    rtx, acks = b.clock(now)
    assert rtx is None and acks.n == NC
    a.receive(acks, now)
    fins = a.close(now)
    assert a.rows() == [TCL.FIN_WAIT_1] * NC
    if lose_first_fin:
        assert b.clock(now) == (None, None)
        now += 1_100_000_000  # the initial RTO is one second
        fins, none = a.clock(now)
        assert fins.n == NC and none is None
    now += 1_000_000
    acks, closing = b.receive(fins, now)  # the FIN in ESTABLISHED: dk_tcp_rx_process and dk_tcp_ack_emit
    assert acks.n == NC and closing.n == 0 and b.rows() == [TCL.IDLE] * NC
    return now, acks


def test_active_and_passive_close(ends):
    a, b, ia, ib, a_port = ends
    now, acks = transfer_then_close(a, b, 10**9, False)
    x, y = a.receive(acks, now)
    assert x.n == 0 and y.n == 0 and a.rows() == [TCL.FIN_WAIT_2] * NC
    assert list(a.last["ack_action"]) == [N.A["NO_DATA"]] * NC
    fins = b.close(now)
    assert b.rows() == [TCL.LAST_ACK] * NC
    x, last = a.receive(fins, now + 1_000_000)
    assert x.n == 0 and last.n == NC
    tw = now + 1_000_000
    x, y = b.receive(last, tw)
    assert x.n == 0 and y.n == 0
    assert a.clock(tw + 5 * 10**9) == (None, None) and b.clock(tw + 5 * 10**9) == (None, None)  # nothing is armed
    W = BUFFER
    finish(a, b, tw, ia, ib, a_port,
           [(PSH | ACK, 0, 0, 1000, W), (FIN | ACK, 1000, 0, 0, W), (ACK, 1001, 1, 0, W - 1)],
           [(ACK, 0, 1000, 0, W - 1000), (ACK, 0, 1001, 0, W - 1001), (FIN | ACK, 0, 1001, 0, W - 1001)])


def test_close_with_a_lost_fin(ends):
    a, b, ia, ib, a_port = ends
    now, acks = transfer_then_close(a, b, 10**9, True)
    x, y = a.receive(acks, now)
    assert a.rows() == [TCL.FIN_WAIT_2] * NC
    fins = b.close(now)
    x, last = a.receive(fins, now + 1_000_000)
    tw = now + 1_000_000
    b.receive(last, tw)
    W = BUFFER
    finish(a, b, tw, ia, ib, a_port,
           [(PSH | ACK, 0, 0, 1000, W), (FIN | ACK, 1000, 0, 0, W), (FIN | ACK, 1000, 0, 0, W), (ACK, 1001, 1, 0, W - 1)],
           [(ACK, 0, 1000, 0, W - 1000), (ACK, 0, 1001, 0, W - 1001), (FIN | ACK, 0, 1001, 0, W - 1001)])


def test_simultaneous_close(ends):
    a, b, ia, ib, a_port = ends
    now = 10**9
    fins_a = a.close(now)
    now += 1_000_000
    acks, closing = b.receive(fins_a, now)
    assert acks.n == NC and closing.n == 0
    fins_b = b.close(now)  # B's FIN acknowledges A's; its pure ACK is lost
    assert a.rows() == [TCL.FIN_WAIT_1] * NC and b.rows() == [TCL.LAST_ACK] * NC
    now += 1_000_000
    x, last = a.receive(fins_b, now)
    assert x.n == 0 and last.n == NC
    assert list(a.last["action"]) == [TCL.POPPED | TCL.ACK_OK | TCL.FIN] * NC  # FIN_WAIT_1 to TIME_WAIT in one frame
    b.receive(last, now)
    W = BUFFER
    finish(a, b, now, ia, ib, a_port,
           [(FIN | ACK, 0, 0, 0, W), (ACK, 1, 1, 0, W - 1)],
           [(ACK, 0, 1, 0, W - 1), (FIN | ACK, 0, 1, 0, W - 1)])
