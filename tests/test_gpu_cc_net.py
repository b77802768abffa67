"""A lossy transfer between two endpoints on one MI355X with the congestion window and the timers on the device: A moves
16 KiB on each of 4 connections to B through the network of tests/stream_net.py (frames dropped, duplicated and locally
reordered while the lossy phase lasts, plus two losses placed by hand so that the run meets a fast retransmit and a
timeout). Per round: cc_send(before) -> dk_tcp_tx_segment -> cc_send(after) -> B: dk_rx_process, dk_tcp_rx_process,
dk_tcp_ack_emit -> A: dk_rx_process, dk_tcp_rx_process, dk_tcp_cc_ack, dk_tcp_ack_process -> dk_tcp_timers on both ends
-> dk_tcp_retransmit / dk_tcp_ack_timer. The host advances the clock and applies the loss; it fills no fire[] and no
cwnd. tests/tcp_cc_reference.py runs beside every congestion-control call, from the tables as that call finds them, and
must agree on every row after it."""
from types import SimpleNamespace

import numpy as np
import pytest

import stream_net as SN
import tcp_cc_reference as R
import tx_segment_reference as M
from tcp_cc_cases import segs_by_conn
from demikernel_amd import (AckEmitResults, Config, FrameBatch, PushList, RxEngine, SocketId, TcpAcker, TcpAckOut,
                            TcpSender, TcpTxResults, UnackedQueue, ack_conn_table, ack_emit_batch, dack_conn_table,
                            flow_array, sync_send_next, synth)
from demikernel_amd import _native as N
from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table
from demikernel_amd.tcp_ackemit import ack_timer_batch, dack_to_device
from demikernel_amd.tcp_cc import (AFTER_SEND, BEFORE_SEND, CcAckOut, TimersOut, cc_ack, cc_conn_table, cc_send,
                                   cc_to_device, cc_to_host, timers)
from demikernel_amd.tcp_rtx import RtxResults, retransmit_batch

pytestmark = pytest.mark.gpu

NC, TOTAL, MSS = 4, 16384, 1000
A_IP, B_IP, B_PORT = synth.ALICE_IPV4, synth.BOB_IPV4, 12345
WSCALE, BUFFER, DELAY = 6, 1 << 20, 40_000_000
LOSSY_ROUNDS, STEP = 6, 10_000_000  # one network leg takes 10 ms
NET = SimpleNamespace(loss=0.1, dup=0.1, span=3)


class Beside:
    """The restatement's congestion-control table, run beside the device's."""

    def __init__(self, cc, d_cc, d_tx, d_ak):
        self.cc, self.d_cc, self.d_tx, self.d_ak = cc.copy(), d_cc, d_tx, d_ak
        self.steps = 0
        self.entered, self.left, self.was_in = set(), set(), set()

    def tables(self):
        return TcpSender.conns_to_host(self.d_tx), TcpAcker.conns_to_host(self.d_ak)

    def check(self, tx_exp, what: str):
        got_cc, got_tx = cc_to_host(self.d_cc), TcpSender.conns_to_host(self.d_tx)
        rows = [c for c in range(NC) if got_cc[c].tobytes() != self.cc[c].tobytes()]
        assert not rows, f"{what}: rows {rows}: device {got_cc[rows]} restatement {self.cc[rows]}"
        assert np.array_equal(got_tx["cwnd"], tx_exp["cwnd"]), (what, got_tx["cwnd"], tx_exp["cwnd"])
        now_in = {c for c in range(NC) if self.cc["flags"][c] & R.IN_RECOVERY}
        self.left |= {c for c in self.entered if c not in now_in and c in self.was_in}
        self.entered |= now_in
        self.was_in = now_in
        self.steps += 1


def test_lossy_transfer_under_cubic():
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    a_port = [40000 + c for c in range(NC)]
    flows_b = flow_array([SocketId.Active((B_IP, B_PORT), (A_IP, a_port[c])) for c in range(NC)])
    flows_a = flow_array([SocketId.Active((A_IP, a_port[c]), (B_IP, B_PORT)) for c in range(NC)])
    isn = rng.integers(0, 1 << 32, NC, dtype=np.uint64).astype(np.uint32)
    isn[0] = (1 << 32) - 9000  # one stream wraps
    irs = rng.integers(0, 1 << 32, NC, dtype=np.uint64).astype(np.uint32)
    d_links = torch.from_numpy(np.ascontiguousarray(M.links_table()).view(np.uint8).copy()).to(dev)
    now = 10**9

    # A: the sender
    sender, eng_a, tcp_a, acker = TcpSender(0), RxEngine(Config(A_IP), device=0), TcpReceiver(0), TcpAcker()
    eng_a.set_sockets(flows_a)
    tx_a = M.conns_toward(flows_b, snd_nxt=isn, rcv_nxt=irs, snd_wnd=65535, cwnd=0, mss=MSS, link=0)
    d_tx_a = sender.conns_to_device(tx_a)
    d_ak = TcpAcker.conns_to_device(ack_conn_table(NC, wl1=irs, wl2=isn, snd_wscale=WSCALE))
    cc0 = cc_conn_table(NC, mss=MSS, seq_no=isn, now_ns=now, fast_convergence=[True, True, False, True])
    d_cc = cc_to_device(cc0)
    queue = UnackedQueue(NC, 32)
    d_rx_a = tcp_a.conns_to_device(conn_table(NC, receive_next=irs, send_next=isn))
    status = torch.zeros(NC, dtype=torch.int32, device=dev)
    beside = Beside(cc0, d_cc, d_tx_a, d_ak)
    # B: the receiver; its timers run on rows of the algorithm None with nothing armed to retransmit
    eng_b, tcp_b, timer_b = RxEngine(Config(B_IP), device=0), TcpReceiver(0), TcpSender(0)
    eng_b.set_sockets(flows_b)
    rx_b = conn_table(NC, receive_next=isn, send_next=irs, buffer_size=BUFFER)
    d_tx_b = timer_b.conns_to_device(M.conns_toward(flows_a, snd_nxt=irs, rcv_wscale=WSCALE, link=1))
    d_dack = dack_to_device(dack_conn_table(NC, delay_ns=DELAY))
    d_ak_b = TcpAcker.conns_to_device(ack_conn_table(NC))
    d_cc_b = cc_to_device(cc_conn_table(NC, mss=MSS, cubic=False))

    src = rng.integers(0, 256, NC * TOTAL, dtype=np.uint8)
    d_src = torch.from_numpy(src).to(dev)
    stride, cap = 1100, 24 * NC
    d_out = torch.zeros(cap * stride, dtype=torch.uint8, device=dev)    # A's new frames
    d_rtx = torch.zeros(NC * stride, dtype=torch.uint8, device=dev)     # A's retransmissions
    d_acks = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)       # B's ACKs
    d_tacks = torch.zeros(NC * 64, dtype=torch.uint8, device=dev)       # B's delayed ACKs
    pushed = np.zeros(NC, np.int64)
    received = [bytearray() for _ in range(NC)]
    kept = []  # every frame B has seen, by global number: stored segments are delivered from a later call
    want_una = ((isn.astype(np.int64) + TOTAL) & 0xFFFFFFFF).astype(np.uint32)
    seen = dict(fast=0, timeout=0, ack_timer=0, dropped=0, rounds=0)

    def network(batch, conn, lossy, forced=()):
        """The frames of `batch` as they arrive: stream_net's network, minus the frames dropped by hand."""
        conn = np.asarray(conn)
        rank = np.zeros(len(conn), np.int64)
        for c in range(NC):
            rank[conn == c] = np.arange((conn == c).sum())
        idx = SN.network(conn, rank, lossy, NET, rng)
        idx = np.array([i for i in idx if (int(conn[i]), int(rank[i])) not in forced], np.int64)
        seen["dropped"] += len(conn) - len(set(idx.tolist()))
        t = torch.from_numpy(idx).to(dev)
        return FrameBatch(batch.blob, batch.off[t].contiguous(), batch.len[t].contiguous())

    def into_b(batch):
        """B receives, delivers and acknowledges; returns its ACK frames and the connection of each."""
        nonlocal rx_b
        if batch.n == 0:
            return None, []
        r = eng_b.results(batch.n, tcp_fields=True)
        eng_b.receive_batch(batch, r)
        out_b = TcpOut(batch.n, NC)
        d_rx_b = tcp_b.conns_to_device(rx_b)
        tcp_b.process(r, d_rx_b, out_b)
        ares = AckEmitResults(cap, NC, batch.n)
        acks = ack_emit_batch(tcp_b, r, out_b, d_rx_b, d_tx_b, d_dack, d_links, now, d_acks, ares, slot_stride=64)
        hb, blob = out_b.to_numpy(), batch.blob.cpu().numpy()
        off, ln = batch.off.cpu().numpy().view(np.uint32), batch.len.cpu().numpy().view(np.uint16)
        base = len(kept)
        kept.extend(blob[int(o):int(o) + int(k)].tobytes() for o, k in zip(off, ln))
        assert (ares.to_numpy()["status"] == 0).all()
        for c in range(NC):
            for v in out_b.delivered(c, hb):
                ref = int(v["ref"])
                if ref == N.DK_TCP_REF_EOF:
                    continue
                frame = kept[ref & ~SN.HANDLE] if ref & SN.HANDLE else kept[base + ref]
                received[c] += frame[int(v["off"]):int(v["off"]) + int(v["len"])]
        rx_b = tcp_b.conns_to_host(d_rx_b)
        SN.carry_refs(rx_b, base + np.arange(batch.n, dtype=np.uint32))
        return acks, ares.to_numpy()["frame_conn"]

    def into_a(batch):
        """B's ACK frames through A's receive path, congestion control, then ACK processing."""
        if batch is None or batch.n == 0:
            return
        sync_send_next(d_rx_a, d_tx_a)
        ra = eng_a.results(batch.n, tcp_fields=True)
        eng_a.receive_batch(batch, ra)
        out_a, aout, cout = TcpOut(batch.n, NC), TcpAckOut(batch.n, NC), CcAckOut(batch.n, NC)
        tcp_a.process(ra, d_rx_a, out_a)
        tx, ak = beside.tables()
        cc_ack(tcp_a, ra, out_a, d_rx_a, d_tx_a, d_ak, d_cc, now, cout)
        acker.process(tcp_a, ra, out_a, d_rx_a, d_tx_a, d_ak, queue, now, aout)
        torch.cuda.synchronize()
        ha, act = ra.to_numpy(), out_a.to_numpy()["action"]
        exp = R.cc_ack(segs_by_conn(ha["flow_id"], act, ha["tcp_ack"], NC), tcp_a.conns_to_host(d_rx_a), tx, ak,
                       beside.cc, now, batch.n)
        got = cout.to_numpy()
        for k in ("status", "new_acks", "dup_acks", "cwnd_after"):
            assert np.array_equal(got[k], exp[k]), (k, got[k], exp[k])
        assert (got["status"] == 0).all() and (aout.to_numpy()["status"] == 0).all(), (got["status"], aout.to_numpy()["status"])
        beside.check(tx, f"round {seen['rounds']} cc_ack")

    rtx_batch, rtx_conn = None, []
    for rnd in range(400):
        una = sender.conns_to_host(d_tx_a)["snd_una"]
        if (una == want_una).all():
            break
        seen["rounds"] += 1
        lossy = 1 <= rnd <= LOSSY_ROUNDS  # round 0 loses only what is dropped by hand, below
        progress = False
        # A sends: the idle restart and the window, the frames, on_send
        tx, ak = beside.tables()
        cc_send(sender, BEFORE_SEND, d_tx_a, d_ak, d_cc, now, status)
        assert (R.cc_send_before(tx, beside.cc, now) == 0).all()
        beside.check(tx, f"round {rnd} before send")
        pc = [c for c in range(NC) if pushed[c] < TOTAL]
        data, dconn = None, []
        if pc:
            push = PushList.from_numpy(pc, [c * TOTAL + pushed[c] for c in pc], [TOTAL - pushed[c] for c in pc])
            res = TcpTxResults(cap, len(pc))
            data = sender.segment_batch(d_src, push, d_tx_a, d_links, d_out, res, slot_stride=stride)
            h = res.to_numpy()
            for b, c in enumerate(pc):
                pushed[c] += int(h["sent"][b])
            queue.append_frames(d_ak, res, push, now, data.n)
            dconn = [pc[int(b)] for b in h["frame_buf"]]
            frames = [[int(h["len_out"][f]) - 54 for f in range(data.n) if dconn[f] == c] for c in range(NC)]
            tx, ak = beside.tables()
            cc_send(sender, AFTER_SEND, d_tx_a, d_ak, d_cc, now, status, push=push, res=res)
            assert (R.cc_send_after(tx, ak, beside.cc, now, frames) == 0).all()
            beside.check(tx, f"round {rnd} after send")
            progress |= data.n > 0
        now += STEP
        # the network; by hand: connection 1 loses the first frame of its first flight (three duplicates follow: a
        # fast retransmit), connection 2 its whole first flight (nothing comes back: a timeout)
        forced = {(1, 0), (2, 0), (2, 1), (2, 2), (2, 3)} if rnd == 0 else ()
        arrivals = []
        if rtx_batch is not None and rtx_batch.n:
            arrivals.append((rtx_batch, rtx_conn, ()))
        if data is not None and data.n:
            arrivals.append((data, dconn, forced))
        for batch, conn, drop in arrivals:
            acks, aconn = into_b(network(batch, conn, lossy, drop))
            if acks is not None and acks.n:  # straight back: B's ACK buffer is reused by its next call
                progress = True
                into_a(network(acks, aconn, lossy))
        now += STEP
        # the timers of both ends
        tout = TimersOut(NC, ack_fire=False)
        tx, ak = beside.tables()
        timers(sender, d_tx_a, d_ak, d_cc, now, tout)
        exp = R.timers(tx, ak, beside.cc, now)
        got = tout.to_numpy()
        assert np.array_equal(got["rtx_fire"], exp["rtx_fire"]) and (got["status"] == 0).all()
        assert (got["n_fast"], got["n_timeout"]) == (exp["n_fast"], exp["n_timeout"])
        beside.check(tx, f"round {rnd} timers")
        seen["fast"] += got["n_fast"]
        seen["timeout"] += got["n_timeout"]
        rtx_batch, rtx_conn = None, []
        if got["n_fast"] + got["n_timeout"]:  # the counts: no array is read to decide this
            rres = RtxResults(NC, NC)
            rtx_batch = retransmit_batch(sender, d_src, tout.rtx_fire, d_tx_a, d_ak, queue, now, d_links, d_rtx, rres,
                                         slot_stride=stride)
            rtx_conn = rres.to_numpy()["frame_conn"]
            progress = True
        tb = TimersOut(NC)
        timers(timer_b, d_tx_b, d_ak_b, d_cc_b, now, tb, dack=d_dack)
        gb = tb.to_numpy()
        assert gb["n_fast"] == gb["n_timeout"] == 0 and (gb["status"] == 0).all()
        if gb["n_ack"]:
            ares = AckEmitResults(NC, NC)
            d_rx_b = tcp_b.conns_to_device(rx_b)
            tacks = ack_timer_batch(timer_b, tb.ack_fire, d_tx_b, d_rx_b, d_dack, d_links, d_tacks, ares, slot_stride=64)
            assert tacks.n == gb["n_ack"]
            seen["ack_timer"] += tacks.n
            into_a(network(tacks, ares.to_numpy()["frame_conn"], lossy))
            progress = True
        if not progress:
            now += 200_000_000  # nothing moved: the clock runs on to the next deadline
    torch.cuda.synchronize()
    print(seen, "checked steps", beside.steps, "entered", beside.entered, "left", beside.left)
    tx_end, ak_end = sender.conns_to_host(d_tx_a), TcpAcker.conns_to_host(d_ak)
    for c in range(NC):
        assert bytes(received[c]) == src[c * TOTAL:(c + 1) * TOTAL].tobytes(), f"connection {c}'s stream"
    assert np.array_equal(tx_end["snd_una"], want_una) and np.array_equal(tx_end["snd_una"], tx_end["snd_nxt"])
    assert (ak_end["q_count"] == 0).all() and (ak_end["rtx_armed"] == 0).all(), ak_end
    assert seen["fast"] >= 1 and seen["timeout"] >= 1 and seen["dropped"] >= 5, seen
    assert beside.left, "no connection entered and left fast recovery"
    assert beside.cc.tobytes() == cc_to_host(d_cc).tobytes()
    for o in (sender, eng_a, tcp_a, eng_b, tcp_b, timer_b):
        o.close()
