"""The loop closed on the MI355X: the replay of tests/test_gpu_ack_net.py with the host's retransmissions done by
dk_tcp_retransmit. Where that replay pokes the retransmitted fronts' tx_time, the timer's rto and rtx_base_ns into the
device tables by hand, this one makes one retransmit call per round that has retransmissions, fire = TIMEOUT for the
connections whose timer the recording fired and FAST for the rest. After the call the ACK table and the pool must be
what those pokes would have left, bit for bit, and the frames must be the restatement's (tests/tcp_rtx_reference.py)
byte for byte; the TX table is untouched. Everything else is that replay: dk_tcp_tx_segment's frames against the
recording, UnackedQueue.append_frames, the recorded ACK batch through dk_rx_process, dk_tcp_rx_process and
dk_tcp_ack_process under the engine's own rule, every comparison with the recorded call, and AckChecker T1-T6 through
to finish. No payload byte of the transfer is on the host side of the calls."""
import numpy as np
import pytest

import ack_net as AN
import tcp_rtx_reference as X
from demikernel_amd import Config, FrameBatch, RxEngine, synth
from demikernel_amd import _native as N
from demikernel_amd.tcp import TcpOut, TcpReceiver
from demikernel_amd.tcp_ack import TcpAcker, TcpAckOut, UnackedQueue, sync_send_next
from demikernel_amd.tcp_rtx import RtxResults, fire_to_device, retransmit_batch
from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults
from test_gpu_ack_net import rule_form
from test_gpu_tcp import assert_same
from test_gpu_tcp_ack import CANARY, compare

pytestmark = pytest.mark.gpu


def replay(name: str) -> dict:
    import torch

    tr = AN.trace(name)
    rows, dev = len(tr.tx0), torch.device("cuda", 0)
    sender, tcp, acker = TcpSender(0), TcpReceiver(0), TcpAcker(None)
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    try:
        eng.set_sockets(tr.flows)
        d_tx, d_ak = sender.conns_to_device(tr.tx0), TcpAcker.conns_to_device(tr.ak0)
        queue = UnackedQueue(rows, tr.cap)
        d_src = torch.from_numpy(tr.src).to(dev)
        d_links = torch.from_numpy(tr.links.view(np.uint8).copy()).to(dev)
        d_out = torch.zeros(tr.max_frames * tr.stride, dtype=torch.uint8, device=dev)
        d_rtx = torch.zeros(rows * tr.stride, dtype=torch.uint8, device=dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        tx32 = d_tx.view(torch.int32).view(rows, N.TX_CONN_DTYPE.itemsize // 4)
        rx = tr.rx0.copy()
        chk = AN.AckChecker(tr)
        forms, k = [], 0
        seen = dict(calls=0, timer=0, fast=0, fin=0)
        for rnd, r in enumerate(tr.rounds):
            ctx = f"{name} round {rnd}"
            tx32[:, N.TX_CONN_DTYPE.fields["mss"][1] // 4] = up(r.mss.astype(np.uint32).view(np.int32))
            if len(r.rtx):
                # the tables the call starts from, and what the host's hand-written pokes would make of them
                tx0, ak0, pool0 = sender.conns_to_host(d_tx), TcpAcker.conns_to_host(d_ak), queue.to_numpy()
                want_ak, want_tt = ak0.copy(), pool0["tx_time"].copy()
                want_tt[ak0["q_first"][r.rtx]] = AN.NONE
                want_ak["rto"][r.rto_set[0]] = r.rto_set[1]
                want_ak["rtx_base_ns"][r.base_set[0]] = r.base_set[1]
                fire = np.zeros(rows, np.uint8)
                fire[r.rtx] = X.FIRE_FAST
                fire[r.rto_set[0]] = X.FIRE_TIMEOUT
                d_rtx.fill_(CANARY & 0xFF)
                res = RtxResults(rows, rows)
                batch = retransmit_batch(sender, d_src, fire_to_device(fire), d_tx, d_ak, queue, r.t_send, d_links,
                                         d_rtx, res, slot_stride=tr.stride)
                exp = X.retransmit(tr.src, fire, tx0, ak0, pool0, r.t_send, tr.links,
                                   np.full(rows * tr.stride, CANARY & 0xFF, np.uint8), slot_stride=tr.stride,
                                   max_frames=rows)
                h = res.to_numpy()
                assert batch.n == h["n_frames"] == len(r.rtx) == exp["n_frames"], f"{ctx}: {batch.n} frames"
                for f in ("status", "frame", "off_out", "len_out", "frame_conn"):
                    assert np.array_equal(h[f], exp[f]), f"{ctx}: dk_tcp_retransmit's {f}"
                assert np.array_equal(h["frame_conn"], np.sort(r.rtx)), ctx
                assert np.array_equal(d_rtx.cpu().numpy(), exp["out"]), f"{ctx}: the frames are not the restatement's"
                got_ak, got_pool = TcpAcker.conns_to_host(d_ak), queue.to_numpy()
                assert got_ak.tobytes() == want_ak.tobytes() == exp["ack_conns"].tobytes(), f"{ctx}: the ACK table"
                assert np.array_equal(got_pool["tx_time"], want_tt), f"{ctx}: tx_time"
                assert all(np.array_equal(got_pool[f], pool0[f]) for f in ("off", "len")), f"{ctx}: off / len"
                assert sender.conns_to_host(d_tx).tobytes() == tx0.tobytes(), f"{ctx}: the TX table was written"
                seen["calls"] += 1
                seen["timer"] += len(r.rto_set[0])
                seen["fast"] += len(r.rtx) - len(r.rto_set[0])
                seen["fin"] += int((h["len_out"] == 54).sum())
            if r.push is not None:
                push = PushList.from_numpy(*r.push)
                res = TcpTxResults(tr.max_frames, push.n)
                batch = sender.segment_batch(d_src, push, d_tx, d_links, d_out, res, slot_stride=tr.stride)
                h, e = res.to_numpy(), r.seg
                assert batch.n == h["frames_written"] == len(e["off_out"]), f"{ctx}: {batch.n} frames"
                for f in ("off_out", "len_out", "frame_buf", "first_frame", "sent", "status"):
                    assert np.array_equal(h[f], e[f]), f"{ctx}: dk_tcp_tx_segment's {f}"
                ln = e["len_out"].astype(np.int64)  # the frames' own bytes: the rest of a slot is not the call's
                at_b = np.repeat(e["off_out"].astype(np.int64) - np.cumsum(ln) + ln, ln) + np.arange(ln.sum())
                bad = np.nonzero(d_out[:batch.n * tr.stride].cpu().numpy()[at_b] != e["out"][at_b])[0]
                assert not len(bad), f"{ctx}: frame {at_b[bad[0]] // tr.stride} is not the recorded one"
                assert sender.conns_to_host(d_tx).tobytes() == e["tx_conns"].tobytes(), f"{ctx}: the TX table"
                queue.append_frames(d_ak, res, push, r.t_send, batch.n)
            chk.host(r)
            a = r.ack
            if a is None:
                continue
            n = len(a.off)
            d_rx = tcp.conns_to_device(rx)
            sync_send_next(d_rx, d_tx)
            res_rx = eng.results(n, tcp_fields=True)
            eng.receive_batch(FrameBatch.from_numpy(a.blob, a.off, a.lens, device=0), res_rx)
            out, aout = TcpOut(n, rows), TcpAckOut(n, rows, fill=CANARY)
            tcp.process(res_rx, d_rx, out)
            acker.process(tcp, res_rx, out, d_rx, d_tx, d_ak, queue, a.now, aout)
            torch.cuda.synchronize()
            forms.append(TcpAcker.last_form(tcp))
            ctx = f"{name} call {k} (round {rnd}, {n} frames, {forms[-1]} form)"
            got_rx, got_out = tcp.conns_to_host(d_rx), out.to_numpy()
            assert_same(got_rx, got_out, a.rx_after, a.rx_out, ctx)
            got = aout.to_numpy()
            got.update(tx_conns=sender.conns_to_host(d_tx), ack_conns=TcpAcker.conns_to_host(d_ak),
                       pool=queue.to_numpy())
            compare(got, a.exp, ctx)
            chk.feed(a, got_out["action"], got, got["tx_conns"], got["ack_conns"], got["pool"])
            AN.carry_refs(got_rx, a.base)
            rx = got_rx
            k += 1
        chk.finish(got["tx_conns"], got["ack_conns"], tr.peer_got, tr.peer_fin)
        assert forms == [rule_form(len(r.ack.off), rows) for r in tr.calls]
        return seen
    finally:
        for o in (sender, tcp, eng):
            o.close()


@pytest.mark.parametrize("name", list(AN.CASES))
def test_lossy_transfer_with_device_retransmissions(name):
    tr = AN.trace(name)
    seen = replay(name)
    print(name, seen)
    assert (seen["timer"], seen["fast"], seen["fin"]) == (tr.stats["timer_rtx"], tr.stats["fast_rtx"],
                                                          tr.stats["fin_rtx"])
    assert seen["calls"] == sum(1 for r in tr.rounds if len(r.rtx))
