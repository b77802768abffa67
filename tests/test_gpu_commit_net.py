"""The loop closed on the MI355X with no step outside dk_tcp.h: the replay of tests/test_gpu_rtx_net.py (the recorder of
tests/ack_net.py: a lossy network, retransmissions by dk_tcp_retransmit) with UnackedQueue.append_frames replaced by
dk_tcp_tx_commit, and dk_tcp_rtx_piggyback after each retransmit call. The regions are as small as the recording
allows (the largest queue any connection ever holds), so the live entries have to move during the transfer, which is
asserted. Every commit is compared with the numpy model on the tables it started from; before and after every ACK call
the live queues, q_count, rtx_armed / rtx_base_ns and the rest of the ACK table are compared with the recorder's
tables (q_first legitimately differs: append_frames always compacts), the TX table and dk_tcp_ack_process's outputs as
bytes; the transfer completes with every byte delivered.

The second test has two endpoints: B owes A a delayed ACK on two connections and then sends data of its own on one.
With dack passed to B's commit that connection's armed is 0 afterwards and dk_tcp_timers reports n_ack == 1 (the other
connection); without it, 2. B's data frame carries the ACK: it moves A's SND.UNA."""
import numpy as np
import pytest

import ack_net as AN
import tcp_commit_reference as C
import tx_segment_reference as M
from demikernel_amd import (AckEmitResults, CommitOut, Config, FrameBatch, PushList, RxEngine, SocketId, TcpAcker,
                            TcpAckOut, TcpSender, TcpTxResults, TimersOut, UnackedQueue, ack_conn_table, ack_emit_batch,
                            cc_conn_table, dack_conn_table, flow_array, rtx_piggyback, sync_send_next, synth, timers,
                            tx_commit)
from demikernel_amd import _native as N
from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table
from demikernel_amd.tcp_ackemit import dack_to_device, dack_to_host
from demikernel_amd.tcp_cc import cc_to_device
from demikernel_amd.tcp_commit import last_form
from demikernel_amd.tcp_rtx import RtxResults, fire_to_device, retransmit_batch
from test_gpu_tcp import assert_same
from test_gpu_tcp_ack import CANARY, OUT_KEYS

pytestmark = pytest.mark.gpu


def tight_cap(tr) -> int:
    """The largest queue any connection holds right after an append, over the whole recording."""
    qc, most = np.zeros(len(tr.tx0), np.int64), 1
    for r in tr.rounds:
        if r.sends is not None:
            qc += np.bincount(r.sends[0], minlength=len(qc))
            most = max(most, int(qc.max()))
        if r.ack is not None:
            qc = r.ack.exp["ack_conns"]["q_count"].astype(np.int64)
    return most


def same_queues(ak, pool, q_cap, rec_ak, rec_pool, ctx):
    """The device's tables against the recorder's: everything but q_first, and the live entries."""
    a, b = ak.copy(), rec_ak.copy()
    a["q_first"] = b["q_first"] = 0
    rows = [c for c in range(len(a)) if a[c].tobytes() != b[c].tobytes()]
    assert not rows, f"{ctx}: ACK rows {rows}: got {ak[rows]} recorded {rec_ak[rows]}"
    for c in range(len(ak)):
        f, g, n = int(ak["q_first"][c]), int(rec_ak["q_first"][c]), int(ak["q_count"][c])
        assert n == 0 or (c * q_cap <= f and f + n <= (c + 1) * q_cap), f"{ctx}: connection {c}'s queue [{f}, +{n})"
        for k in pool:
            assert np.array_equal(pool[k][f:f + n], rec_pool[k][g:g + n]), f"{ctx}: connection {c}'s live {k}"


def replay(name: str, form) -> dict:
    import torch

    tr = AN.trace(name)
    rows, dev, q_cap = len(tr.tx0), torch.device("cuda", 0), tight_cap(tr)
    sender, tcp, acker = TcpSender(0), TcpReceiver(0), TcpAcker(None)
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    try:
        eng.set_sockets(tr.flows)
        d_tx, d_ak = sender.conns_to_device(tr.tx0), TcpAcker.conns_to_device(tr.ak0)
        queue = UnackedQueue(rows, q_cap)
        d_src = torch.from_numpy(tr.src).to(dev)
        d_links = torch.from_numpy(tr.links.view(np.uint8).copy()).to(dev)
        d_out = torch.zeros(tr.max_frames * tr.stride, dtype=torch.uint8, device=dev)
        d_rtx = torch.zeros(rows * tr.stride, dtype=torch.uint8, device=dev)
        owed = dack_conn_table(rows, armed=1, deadline_ns=5)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        tx32 = d_tx.view(torch.int32).view(rows, N.TX_CONN_DTYPE.itemsize // 4)
        rx = tr.rx0.copy()
        seen = dict(moved_back=0, in_place=0, rtx=0, forms=set())
        for rnd, r in enumerate(tr.rounds):
            ctx = f"{name} round {rnd}"
            tx32[:, N.TX_CONN_DTYPE.fields["mss"][1] // 4] = up(r.mss.astype(np.uint32).view(np.int32))
            if len(r.rtx):
                fire = np.zeros(rows, np.uint8)
                fire[r.rtx] = N.DK_TCP_RTX_FAST
                fire[r.rto_set[0]] = N.DK_TCP_RTX_TIMEOUT
                res = RtxResults(rows, rows)
                batch = retransmit_batch(sender, d_src, fire_to_device(fire), d_tx, d_ak, queue, r.t_send, d_links,
                                         d_rtx, res, slot_stride=tr.stride)
                assert batch.n == len(r.rtx), f"{ctx}: {batch.n} retransmissions"
                d_dack = dack_to_device(owed)
                rtx_piggyback(sender, res, d_dack)
                want = owed.copy()
                want["armed"][r.rtx] = 0
                assert dack_to_host(d_dack).tobytes() == want.tobytes(), f"{ctx}: dk_tcp_rtx_piggyback"
                seen["rtx"] += len(r.rtx)
            if r.push is not None:
                push = PushList.from_numpy(*r.push)
                res = TcpTxResults(tr.max_frames, push.n)
                sender.segment(d_src, push, d_tx, d_links, d_out, res, slot_stride=tr.stride)
                ak0, pool0 = TcpAcker.conns_to_host(d_ak), queue.to_numpy()
                cout = CommitOut(rows, fill=CANARY)
                tx_commit(sender, push, res, d_ak, queue, r.t_send, cout, form=form)  # no n_frames read between them
                torch.cuda.synchronize()
                seen["forms"].add(last_form(sender))
                h, e = res.to_numpy(), r.seg
                assert h["frames_written"] == len(e["off_out"]), f"{ctx}: {h['frames_written']} frames"
                for f in ("off_out", "len_out", "frame_buf", "first_frame", "sent", "status"):
                    assert np.array_equal(h[f], e[f]), f"{ctx}: dk_tcp_tx_segment's {f}"
                ln = e["len_out"].astype(np.int64)  # the frames' own bytes: the rest of a slot is not the call's
                at_b = np.repeat(e["off_out"].astype(np.int64) - np.cumsum(ln) + ln, ln) + np.arange(ln.sum())
                bad = np.nonzero(d_out[:len(ln) * tr.stride].cpu().numpy()[at_b] != e["out"][at_b])[0]
                assert not len(bad), f"{ctx}: frame {at_b[bad[0]] // tr.stride} is not the recorded one"
                exp = C.tx_commit(r.push[0], r.push[1], h, ak0, pool0, q_cap, r.t_send)
                ak1, pool1, co = TcpAcker.conns_to_host(d_ak), queue.to_numpy(), cout.to_numpy()
                assert np.array_equal(co["status"], exp["status"]) and not co["status"].any(), f"{ctx}: {co['status']}"
                assert np.array_equal(co["appended"], exp["appended"]), ctx
                assert ak1.tobytes() == exp["ack_conns"].tobytes(), f"{ctx}: the ACK table after the commit"
                mask = C.live_mask(exp, q_cap, rows * q_cap)
                assert all(np.array_equal(pool1[k][mask], exp["pool"][k][mask]) for k in pool1), f"{ctx}: the pool"
                sent = exp["appended"] > 0
                back = sent & (ak0["q_count"] > 0) & (ak1["q_first"] < ak0["q_first"])
                seen["moved_back"] += int(back.sum())
                seen["in_place"] += int((sent & (ak0["q_count"] > 0) & (ak1["q_first"] == ak0["q_first"])).sum())
            a = r.ack
            if a is None:
                continue
            same_queues(TcpAcker.conns_to_host(d_ak), queue.to_numpy(), q_cap, a.start["ak"], a.start["pool"],
                        f"{ctx}, before the ACKs")
            n = len(a.off)
            d_rx = tcp.conns_to_device(rx)
            sync_send_next(d_rx, d_tx)
            res_rx = eng.results(n, tcp_fields=True)
            eng.receive_batch(FrameBatch.from_numpy(a.blob, a.off, a.lens, device=0), res_rx)
            out, aout = TcpOut(n, rows), TcpAckOut(n, rows, fill=CANARY)
            tcp.process(res_rx, d_rx, out)
            acker.process(tcp, res_rx, out, d_rx, d_tx, d_ak, queue, a.now, aout)
            torch.cuda.synchronize()
            got_rx, got_out = tcp.conns_to_host(d_rx), out.to_numpy()
            assert_same(got_rx, got_out, a.rx_after, a.rx_out, ctx)
            got = aout.to_numpy()
            for k in OUT_KEYS:
                assert np.array_equal(got[k], a.exp[k]), f"{ctx}: dk_tcp_ack_process's {k}"
            tx_now, ak_now = sender.conns_to_host(d_tx), TcpAcker.conns_to_host(d_ak)
            assert tx_now.tobytes() == a.exp["tx_conns"].tobytes(), f"{ctx}: the TX table"
            same_queues(ak_now, queue.to_numpy(), q_cap, a.exp["ack_conns"], a.exp["pool"], f"{ctx}, after the ACKs")
            AN.carry_refs(got_rx, a.base)
            rx = got_rx
        nc, L = tr.case.nconns, tr.case.stream
        final = ((tr.isn[:nc].astype(np.int64) + L + 1) & AN.M32).astype(np.uint32)
        assert tr.done and (tx_now["snd_una"][:nc] == final).all() and (tx_now["snd_nxt"][:nc] == final).all()
        assert not ak_now["q_count"][:nc].any() and not ak_now["rtx_armed"][:nc].any(), "a queue or a timer is left"
        for c in range(nc):  # the frames were the recorded ones byte for byte: B got what the recording says
            assert tr.peer_fin[c] and np.array_equal(tr.peer_got[c], AN.SN.stream_bytes(c, np.arange(L))), c
        seen["q_cap"] = q_cap
        return seen
    finally:
        for o in (sender, tcp, eng):
            o.close()


@pytest.mark.parametrize("name", list(AN.CASES))
def test_lossy_transfer_with_device_commits(name):
    tr = AN.trace(name)
    seen = replay(name, None)
    print(name, seen)
    assert seen["moved_back"] > 0, "no queue ever moved back to its region's start"
    assert seen["in_place"] > 0, "no append ever went in place behind a live queue"
    assert seen["rtx"] == tr.stats["timer_rtx"] + tr.stats["fast_rtx"]


@pytest.mark.parametrize("form", ["conn", "chip"])
@pytest.mark.parametrize("name", ["one_long", "many"])
def test_lossy_transfer_forced_form(name, form):
    seen = replay(name, form)
    assert seen["forms"] == {form} and seen["moved_back"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# two endpoints: a data frame carries the ACK
# ---------------------------------------------------------------------------------------------------------------------
NC, MSS, WSCALE, BUFFER, DELAY = 2, 1000, 6, 1 << 20, 40_000_000
A_IP, B_IP, B_PORT = synth.ALICE_IPV4, synth.BOB_IPV4, 12345


@pytest.mark.parametrize("piggyback", [True, False])
def test_data_frames_cancel_the_delayed_ack(piggyback):
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    a_port = [40000 + c for c in range(NC)]
    flows_b = flow_array([SocketId.Active((B_IP, B_PORT), (A_IP, a_port[c])) for c in range(NC)])  # at B
    flows_a = flow_array([SocketId.Active((A_IP, a_port[c]), (B_IP, B_PORT)) for c in range(NC)])  # at A
    isn, irs = (rng.integers(0, 1 << 32, NC, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    d_links = torch.from_numpy(np.ascontiguousarray(M.links_table()).view(np.uint8).copy()).to(dev)
    stride, cap = 1088, 4
    # A: sends first, and takes B's frames in
    snd_a, eng_a, tcp_a, acker = TcpSender(0), RxEngine(Config(A_IP), device=0), TcpReceiver(0), TcpAcker()
    eng_a.set_sockets(flows_a)
    d_tx_a = snd_a.conns_to_device(M.conns_toward(flows_b, snd_nxt=isn, rcv_nxt=irs, snd_wnd=65535, mss=MSS, link=0))
    d_ak_a = TcpAcker.conns_to_device(ack_conn_table(NC, wl1=irs, wl2=isn, snd_wscale=WSCALE))
    queue_a = UnackedQueue(NC, cap)
    d_rx_a = tcp_a.conns_to_device(conn_table(NC, receive_next=irs, send_next=isn, buffer_size=BUFFER))
    # B: receives, owes the ACK, then sends data of its own
    snd_b, eng_b, tcp_b = TcpSender(0), RxEngine(Config(B_IP), device=0), TcpReceiver(0)
    eng_b.set_sockets(flows_b)
    d_rx_b = tcp_b.conns_to_device(conn_table(NC, receive_next=isn, send_next=irs, buffer_size=BUFFER))
    d_tx_b = snd_b.conns_to_device(M.conns_toward(flows_a, snd_nxt=irs, rcv_wscale=WSCALE, snd_wnd=65535, mss=MSS,
                                                  link=1))
    d_ak_b = TcpAcker.conns_to_device(ack_conn_table(NC, wl1=isn, wl2=irs))
    d_cc_b = cc_to_device(cc_conn_table(NC, mss=MSS, now_ns=10**9))
    queue_b = UnackedQueue(NC, cap)
    d_dack = dack_to_device(dack_conn_table(NC, delay_ns=DELAY))
    d_src = torch.from_numpy(rng.integers(0, 256, 4096, dtype=np.uint8)).to(dev)
    d_out_a = torch.zeros(cap * stride, dtype=torch.uint8, device=dev)
    d_out_b = torch.zeros(cap * stride, dtype=torch.uint8, device=dev)
    d_acks = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
    now = 10**9
    try:
        # A -> B: one segment on each connection, queued by the commit
        push = PushList.from_numpy([0, 1], [0, 1000], [1000, 1000])
        res = TcpTxResults(cap, 2)
        batch = snd_a.segment_batch(d_src, push, d_tx_a, d_links, d_out_a, res, slot_stride=stride)
        cout = CommitOut(NC)
        tx_commit(snd_a, push, res, d_ak_a, queue_a, now, cout)
        assert batch.n == 2 and cout.to_numpy()["appended"].tolist() == [1, 1]
        # B takes them in: both ACKs are delayed
        now += 500_000
        r = eng_b.results(2, tcp_fields=True)
        eng_b.receive_batch(batch, r)
        out_b = TcpOut(2, NC)
        tcp_b.process(r, d_rx_b, out_b)
        ares = AckEmitResults(cap, NC, 2)
        acks = ack_emit_batch(tcp_b, r, out_b, d_rx_b, d_tx_b, d_dack, d_links, now, d_acks, ares, slot_stride=64)
        dk = dack_to_host(d_dack)
        assert acks.n == 0 and (out_b.to_numpy()["action"] == N.A["DELIVERED"]).all() and dk["armed"].tolist() == [1, 1]
        deadline = now + DELAY
        assert dk["deadline_ns"].tolist() == [deadline] * NC
        # B sends 500 bytes of its own on connection 0: the frame carries the ACK
        now += 1_000_000
        push_b = PushList.from_numpy([0], [2000], [500])
        res_b = TcpTxResults(cap, 1)
        batch_b = snd_b.segment_batch(d_src, push_b, d_tx_b, d_links, d_out_b, res_b, slot_stride=stride, rx_conns=d_rx_b)
        cout_b = CommitOut(NC)
        tx_commit(snd_b, push_b, res_b, d_ak_b, queue_b, now, cout_b, dack=d_dack if piggyback else None)
        dk = dack_to_host(d_dack)
        assert batch_b.n == 1 and cout_b.to_numpy()["appended"].tolist() == [1, 0]
        assert dk["armed"].tolist() == ([0, 1] if piggyback else [1, 1]) and dk["deadline_ns"].tolist() == [deadline] * NC
        # B's timer wheel at the deadline
        tout = TimersOut(NC)
        timers(snd_b, d_tx_b, d_ak_b, d_cc_b, deadline, tout, dack=d_dack)
        t = tout.to_numpy()
        assert t["n_ack"] == (1 if piggyback else 2) and t["ack_fire"].tolist() == ([0, 1] if piggyback else [1, 1])
        assert t["n_timeout"] == 0 and t["n_fast"] == 0
        # and A: B's data frame acknowledges connection 0's segment
        sync_send_next(d_rx_a, d_tx_a)
        ra = eng_a.results(1, tcp_fields=True)
        eng_a.receive_batch(batch_b, ra)
        out_a, aout = TcpOut(1, NC), TcpAckOut(1, NC)
        tcp_a.process(ra, d_rx_a, out_a)
        acker.process(tcp_a, ra, out_a, d_rx_a, d_tx_a, d_ak_a, queue_a, now + 500_000, aout)
        torch.cuda.synchronize()
        assert out_a.to_numpy()["action"].tolist() == [N.A["DELIVERED"]] and not aout.to_numpy()["status"].any()
        tx_a, ak_a = snd_a.conns_to_host(d_tx_a), TcpAcker.conns_to_host(d_ak_a)
        assert tx_a["snd_una"].tolist() == [(int(isn[0]) + 1000) & 0xFFFFFFFF, int(isn[1])]
        assert ak_a["q_count"].tolist() == [0, 1] and ak_a["rtx_armed"].tolist() == [0, 1]
    finally:
        for o in (snd_a, eng_a, tcp_a, snd_b, eng_b, tcp_b):
            o.close()
