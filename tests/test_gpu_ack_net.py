"""The sender's side of a transfer across calls on the MI355X (tests/ack_net.py): every case's recording replayed on
one TcpSender / TcpReceiver / UnackedQueue whose tables stay on the device for the whole case. Each round the recorded
host actions (the MSS column, the retransmitted fronts' tx_time := NONE, the timer's back-off and restart) are applied
to the device tables; dk_tcp_tx_segment cuts the recorded push list, and its frames must be the recorded ones byte for
byte; UnackedQueue.append_frames queues them; the recorded ACK batch goes through dk_rx_process, dk_tcp_rx_process
and dk_tcp_ack_process. After every call all outputs, both tables as bytes and the whole pool are compared with the
recorded call (so a divergence is reported at the first call that shows it), then AckChecker (no reference inside)
is fed what the device returned. Every case runs in the three forced forms and once under the engine's own rule."""
import numpy as np
import pytest

import ack_net as AN
from demikernel_amd import Config, FrameBatch, RxEngine, synth
from demikernel_amd import _native as N
from demikernel_amd.tcp import TcpOut, TcpReceiver
from demikernel_amd.tcp_ack import TcpAcker, TcpAckOut, UnackedQueue, sync_send_next
from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults
from test_gpu_tcp import assert_same
from test_gpu_tcp_ack import CANARY, FORMS, compare

pytestmark = pytest.mark.gpu


def rule_form(n: int, rows: int) -> str:
    """dk_tcp_ack_process's own choice (tcp_ack_kernels.hip)."""
    return "chip" if n >= 1024 * rows and rows <= 256 else "wave" if n >= 8 * rows else "lane"


def replay(name: str, form, radix: bool = False):
    """The case's recording on the device; returns the form and the sort of every ACK call."""
    import torch

    tr = AN.trace(name)
    rows, dev = len(tr.tx0), torch.device("cuda", 0)
    sender, tcp, acker = TcpSender(0), TcpReceiver(0, radix_sort=radix), TcpAcker(form)
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    try:
        eng.set_sockets(tr.flows)
        d_tx, d_ak = sender.conns_to_device(tr.tx0), TcpAcker.conns_to_device(tr.ak0)
        queue = UnackedQueue(rows, tr.cap)
        d_src = torch.from_numpy(tr.src).to(dev)
        d_links = torch.from_numpy(tr.links.view(np.uint8).copy()).to(dev)
        d_out = torch.zeros(tr.max_frames * tr.stride, dtype=torch.uint8, device=dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        tx32 = d_tx.view(torch.int32).view(rows, N.TX_CONN_DTYPE.itemsize // 4)
        ak32 = d_ak.view(torch.int32).view(rows, N.ACK_CONN_DTYPE.itemsize // 4)
        ak64 = d_ak.view(torch.int64).view(rows, N.ACK_CONN_DTYPE.itemsize // 8)
        akf = d_ak.view(torch.float64).view(rows, N.ACK_CONN_DTYPE.itemsize // 8)
        at = lambda dt, k, w: dt.fields[k][1] // w  # noqa: E731
        rx = tr.rx0.copy()
        chk = AN.AckChecker(tr)
        forms, sorts, k = [], [], 0
        for rnd, r in enumerate(tr.rounds):
            ctx = f"{name} round {rnd}"
            # what the host does between two calls
            tx32[:, at(N.TX_CONN_DTYPE, "mss", 4)] = up(r.mss.astype(np.uint32).view(np.int32))
            if len(r.rtx):
                front = ak32[up(r.rtx), at(N.ACK_CONN_DTYPE, "q_first", 4)].long()
                queue.tx_time[front] = -1  # DK_TCP_TX_TIME_NONE
            if len(r.rto_set[0]):
                akf[up(r.rto_set[0]), at(N.ACK_CONN_DTYPE, "rto", 8)] = up(r.rto_set[1])
                ak64[up(r.base_set[0]), at(N.ACK_CONN_DTYPE, "rtx_base_ns", 8)] = r.base_set[1]
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
            sorts.append(tcp.last_sort)
            ctx = f"{name} call {k} (round {rnd}, {n} frames, {forms[-1]} form, {sorts[-1]} sort)"
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
        return forms, sorts
    finally:
        for o in (sender, tcp, eng):
            o.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(AN.CASES))
def test_transfer_forced_form(name, form):
    forms, sorts = replay(name, form)
    assert set(forms) == {form}, set(forms)


@pytest.mark.parametrize("name", list(AN.CASES))
def test_transfer_engine_rule(name):
    """No form forced: the rule changes form with the batch's shape mid-case, on one context whose chip-form scratch
    grows with the largest batch so far."""
    tr = AN.trace(name)
    rows = len(tr.tx0)
    forms, sorts = replay(name, None)
    print(name, "forms by rule:", forms)
    assert forms == [rule_form(len(r.ack.off), rows) for r in tr.calls]
    assert set(sorts) == {"counting" if rows <= 255 else "radix"}
    want = {"one_long": "chip", "few": "wave", "many": "lane"}.get(name)
    assert want is None or want in forms, (want, forms)


def test_wide_300_radix_sort_forced():
    forms, sorts = replay("wide_300", None, radix=True)
    assert set(sorts) == {"radix"}
