"""dk_tcp_ack_process on the MI355X against tests/tcp_ack_reference.py, bit for bit on every output and every piece
of state (the tables compared as bytes, so srtt / rttvar / rto as their 64 bits). The frames of tests/tcp_ack_cases.py
go through dk_rx_process and dk_tcp_rx_process first, so the actions are the engine's own; the reference then gets the
device's per-frame results. Every case runs in all three forms (dk_diag_tcp_ack_set_form); cases whose outcome depends on
the arrival order also run under both sorts of dk_tcp_rx_process. Outputs start canary-filled: everything the contract
says is written must be."""
import functools

import numpy as np
import pytest

import tcp_ack_cases as C
import tcp_ack_reference as R
from ctl_calls import delayed, stream_pair
from demikernel_amd import Config, FrameBatch, RxEngine, synth
from demikernel_amd import _native as N
from demikernel_amd.rx import Fail
from demikernel_amd.tcp import TcpOut, TcpReceiver
from demikernel_amd.tcp_ack import TcpAcker, TcpAckOut, UnackedQueue

pytestmark = pytest.mark.gpu
CANARY = 0x5A5A5A5A
FORMS = ["lane", "wave", "chip"]
OUT_KEYS = ("acked", "status", "new_acks", "dup_acks", "bytes_acked", "samples")


class Device:
    """One case on the device up to and including dk_tcp_rx_process; ack() runs the ACK pass and reads everything."""

    def __init__(self, case: dict, radix: bool = False):
        import torch

        self.case, self.n, self.nrows = case, case["n"], case["nconns"]
        self.tcp = TcpReceiver(0, radix_sort=radix)
        self.eng = RxEngine(Config(synth.BOB_IPV4), device=0)
        self.eng.set_sockets(case["flows"])
        self.r = self.eng.results(self.n, tcp_fields=True)
        self.d_rx = self.tcp.conns_to_device(case["rx"])
        self.d_tx = torch.from_numpy(case["tx"].view(np.uint8).copy()).cuda()
        self.d_ak = TcpAcker.conns_to_device(case["ak"])
        self.q = UnackedQueue.from_numpy(case["pool"]["off"], case["pool"]["len"], case["pool"]["tx_time"])
        self.out = TcpOut(self.n, self.nrows)
        self.aout = TcpAckOut(self.n, self.nrows, fill=CANARY)

    def receive(self):
        if self.n:
            c = self.case
            self.eng.receive_batch(FrameBatch.from_numpy(c["blob"], c["off"], c["lens"], device=0), self.r)
        self.tcp.process(self.r, self.d_rx, self.out)

    def ack(self, form, **kw):
        TcpAcker(form).process(self.tcp, self.r, self.out, self.d_rx, self.d_tx, self.d_ak, self.q, self.case["now"],
                               self.aout, **kw)

    def read(self) -> dict:
        import torch

        torch.cuda.synchronize()
        got = self.aout.to_numpy()
        got.update(tx_conns=self.d_tx.cpu().numpy().view(N.TX_CONN_DTYPE).copy(),
                   ack_conns=TcpAcker.conns_to_host(self.d_ak), pool=self.q.to_numpy(),
                   rx_conns=self.tcp.conns_to_host(self.d_rx))
        return got

    def close(self):
        self.tcp.close()
        self.eng.close()


def compare(got: dict, exp: dict, ctx: str):
    for k in OUT_KEYS:
        if not np.array_equal(got[k], exp[k]):
            bad = np.nonzero(got[k] != exp[k])[0][:8]
            raise AssertionError(f"{ctx}: {k} differs at {bad}: got {got[k][bad]} expected {exp[k][bad]}")
    for k in ("tx_conns", "ack_conns"):
        g, e = got[k].view(np.uint8).reshape(len(got[k]), -1), exp[k].view(np.uint8).reshape(len(exp[k]), -1)
        bad = np.nonzero((g != e).any(1))[0][:4]
        assert not len(bad), f"{ctx}: {k} differs at rows {bad}: got {got[k][bad]} expected {exp[k][bad]}"
    for k, v in exp["pool"].items():
        bad = np.nonzero(got["pool"][k] != v)[0][:8]
        assert not len(bad), f"{ctx}: pool {k} differs at {bad}: got {got['pool'][k][bad]} expected {v[bad]}"


def run(case: dict, form, radix: bool = False, expect_form=None) -> dict:
    """The whole chain on the device, compared with the reference; returns the reference's result and the actions."""
    d = Device(case, radix)
    try:
        d.receive()
        import torch

        torch.cuda.synchronize()
        rx_before = d.tcp.conns_to_host(d.d_rx)
        h, act = d.r.to_numpy(), d.out.to_numpy()["action"]
        d.ack(form)
        got = d.read()
        ran = TcpAcker.last_form(d.tcp)
        sort = d.tcp.last_sort
    finally:
        d.close()
    exp = R.ack_process(h["flow_id"], act, h["tcp_seq"], h["tcp_ack"], h["tcp_win"], rx_before, case["tx"], case["ak"],
                        case["pool"], case["now"])
    ctx = f"{ran} form, {sort} sort"
    compare(got, exp, ctx)
    assert np.array_equal(got["rx_conns"].view(np.uint8), rx_before.view(np.uint8)), f"{ctx}: the RX table was written"
    assert ran == (expect_form or form), (ran, form)
    if case["n"] and case["nconns"]:
        assert sort == ("radix" if radix or case["nconns"] > 255 else "counting")
    exp["action"] = act
    return exp


def hist(exp) -> dict:
    return {N.TCP_ACTIONS[a]: int(k) for a, k in enumerate(np.bincount(exp["action"], minlength=13)) if k}


@functools.lru_cache(maxsize=None)
def case_one(m: int):
    k = (0, 1, 63, 64, 65, 129, 4097).index(m)
    return C.build([C.Script(m=m, stream=C.ACK_STREAMS[k % 3], qn=C.QUEUE_COUNTS[k % 6] if m < 4097 else 200,
                             marker=k % 2 == 0, mixed=True)], seed=20 + k, udp_every=7)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 129, 4097])
def test_one_connection(m, form):
    exp = run(case_one(m), form)
    if m >= 63:
        assert exp["new_acks"][0] > 0 and exp["samples"][0] > 0, hist(exp)
    assert exp["status"][0] == R.OK and exp["status"][1] == R.E_STATE  # the listener's row


@functools.lru_cache(maxsize=None)
def case_three(k: int):
    ms = [(0, 1, 63), (64, 65, 129), (4097, 0, 64)][k]
    return C.build([C.Script(m=m, stream=C.ACK_STREAMS[(k + j) % 5], qn=C.QUEUE_COUNTS[(2 * k + j) % 6],
                             marker=j == 1, close=("", "fin", "rst")[(j + k) % 3], end=("whole", "inside", "boundary")[j])
                    for j, m in enumerate(ms)], seed=40 + k)


@pytest.mark.parametrize("radix", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [0, 1, 2])
def test_three_connections(k, form, radix):
    exp = run(case_three(k), form, radix)
    assert list(exp["status"][:3]) == [R.OK] * 3


@functools.lru_cache(maxsize=None)
def case_wide():
    return C.build(C.shapes(300), seed=7)


@pytest.mark.parametrize("form", FORMS)
def test_300_connections(form):
    """Above the counting pass's 255 rows: the radix order. Every segment count and queue size, every ACK stream, a
    FIN or an RST mid-stream on two connections in seven, connections without a segment, one with 4,097."""
    exp = run(case_wide(), form)
    h = hist(exp)
    assert {"DELIVERED", "STORED", "NO_DATA", "FIN", "DUPLICATE", "OUT_OF_WINDOW", "RST", "NO_ACK", "ACK_UNSENT",
            "UNPROCESSED", "SKIP"} <= set(h), h
    assert (exp["status"][:300] == R.OK).all() and exp["dup_acks"].sum() > 0 and exp["samples"].sum() > 0
    old = exp["acked"][(exp["acked"] >= 1 << 31)]
    assert len(old) > 0  # old ACKs


@functools.lru_cache(maxsize=None)
def case_streams(stream: str):
    return C.build([C.Script(m=m, stream=stream, qn=qn, mixed=mixed, end=end)
                    for m, qn, mixed, end in ((129, 65, True, "whole"), (65, 64, False, "inside"),
                                              (64, 200, True, "boundary"), (8, 1, False, "whole"))],
                   seed=60 + C.ACK_STREAMS.index(stream))


@pytest.mark.parametrize("radix", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("stream", C.ACK_STREAMS)
def test_ack_streams(stream, form, radix):
    exp = run(case_streams(stream), form, radix)
    if stream == "all_una":
        assert exp["new_acks"][:4].sum() == 0 and exp["dup_acks"][:4].sum() > 0 and exp["bytes_acked"].sum() == 0
    if stream == "all_nxt":
        assert (exp["new_acks"][:4] == 1).all() and (exp["ack_conns"]["q_count"][:4] == 0).all()
        assert (exp["ack_conns"]["rtx_armed"][:4] == 0).all()
    if stream == "rising_dups":
        assert exp["dup_acks"].sum() > 0 and (exp["acked"] >= 1 << 31).any()


@functools.lru_cache(maxsize=None)
def case_wrap():
    top = 1 << 32
    return C.build([C.Script(m=129, una=top - 1000, qn=65), C.Script(m=65, una=top - 1, qn=64, marker=True),
                    C.Script(m=129, rn=top - 100, qn=63, stream="reordered"),
                    C.Script(m=64, rn=top - 3, una=top - 700, qn=20, wl1_off=-2, wl2_off=0, mixed=False)], seed=77)


@pytest.mark.parametrize("form", FORMS)
def test_wrapping(form):
    exp = run(case_wrap(), form)
    tx0 = case_wrap()["tx"]
    assert (exp["tx_conns"]["snd_una"][:2] < tx0["snd_una"][:2]).all()  # SND.UNA went through zero
    assert exp["ack_conns"]["wl1"][2] < case_wrap()["ak"]["wl1"][2]  # and wl1


@functools.lru_cache(maxsize=None)
def case_queues():
    s = []
    for qn in C.QUEUE_COUNTS:
        for end in ("whole", "boundary", "inside"):
            s.append(C.Script(m=65 if qn % 2 else 12, qn=qn, end=end, marker=end == "whole" and qn in (0, 64, 200),
                              mixed=False))
    return C.build(s, seed=88)


@pytest.mark.parametrize("form", FORMS)
def test_queues(form):
    exp = run(case_queues(), form)
    assert (exp["status"][:18] == R.OK).all()
    armed = exp["ack_conns"]["rtx_armed"][:18]
    assert armed.any() and not armed.all()
    assert (exp["pool"]["tx_time"] != case_queues()["pool"]["tx_time"]).any()  # an entry was trimmed


@functools.lru_cache(maxsize=None)
def case_extremes(now: int):
    return C.extremes(now)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("now", C.EXTREME_NOWS)
def test_rtt_and_rto_extremes(now, form):
    """RTT samples from 0 to 2^64 - 2 ns at a clock of 2^64 - 2 (and at 2^63, where transmit times above the clock
    exist), RTO states on both clamps, carried and backed off by the host, srtt subnormal: tcp_ack_cases.extremes.
    tests/test_tcp_ack_model.py shows that a sample cut to 32 bits or taken as an int64 gives another srtt here."""
    case = case_extremes(now)
    exp = run(case, form)
    C.check_extremes(case, exp)


@functools.lru_cache(maxsize=None)
def case_fallbacks():
    """Connections the wave form hands to its one lane: segments 2^30 behind wl1 or 3 * 2^29 ahead of it, wl2 2^31 behind
    SND.NXT, a marker in the middle of the queue swallowing a remainder, bytes acknowledged behind the marker."""
    return C.build([C.Script(m=65, wl1_off=(1 << 30) + 5, qn=20), C.Script(m=65, wl1_off=-(3 << 29) - 5, qn=20),
                    C.Script(m=65, wl2_off=-0x7FFFFFF0, qn=20), C.Script(m=129, qn=70),
                    C.Script(m=20, qn=5, marker=True, extra_flight=3, stream="all_nxt", mixed=False),
                    C.Script(m=70, qn=66, marker=True, extra_flight=40, mixed=False)], seed=99)


@pytest.mark.parametrize("form", FORMS)
def test_wave_form_fallbacks(form):
    exp = run(case_fallbacks(), form)
    assert list(exp["status"][:5]) == [R.OK] * 5 and exp["status"][5] in (R.OK, R.E_DRY)


def failure_scripts():
    f = {R.E_STATE: dict(tx__state=N.DK_TCP_CLOSED), R.E_SND_NXT: dict(rx__send_next=12345),
         R.E_WSCALE: dict(ak__snd_wscale=15), R.E_QUEUE: dict(ak__q_count=1 << 20)}
    s = [C.Script(m=40, qn=30)]
    for st in (R.E_STATE, R.E_SND_NXT, R.E_WSCALE, R.E_QUEUE):
        s += [C.Script(m=70, qn=30, bad=f[st]), C.Script(m=9, qn=30, mixed=False)]
    s += [C.Script(m=70, qn=30, wl2_off=5), C.Script(m=70, qn=30, extra_flight=900, end="whole", mixed=False),
          C.Script(m=66, qn=3)]
    return s


@functools.lru_cache(maxsize=None)
def case_failures():
    case = C.build(failure_scripts(), seed=111)
    # E_FLIGHT: SND.NXT 2^31 ahead of SND.UNA (both tables agree on SND.NXT; every ack of the batch is then ACK_UNSENT
    # or old against it, the status comes first)
    c = 11
    case["tx"]["snd_nxt"][c] = case["rx"]["send_next"][c] = (int(case["tx"]["snd_una"][c]) + (1 << 31)) & R.M32
    return case


@pytest.mark.parametrize("form", FORMS)
def test_failure_statuses(form):
    exp = run(case_failures(), form)
    want = [R.OK, R.E_STATE, R.OK, R.E_SND_NXT, R.OK, R.E_WSCALE, R.OK, R.E_QUEUE, R.OK, R.E_WL2, R.E_DRY, R.E_FLIGHT]
    assert list(exp["status"][:12]) == want, exp["status"]
    ok = np.array(want) == R.OK
    assert (exp["new_acks"][:12][ok] > 0).all() and (exp["new_acks"][:12][~ok] == 0).all()


def test_engine_rule_picks_the_form():
    """No form forced: one lane per connection below 8 segments per table row, one wave from there, the chip form from
    1,024 (the 4,097-segment connection and the listener's row: 4,682 frames over 2 rows)."""
    assert case_one(4097)["n"] >= 1024 * case_one(4097)["nconns"]
    run(case_one(4097), None, expect_form="chip")
    few = C.build([C.Script(m=7, qn=4), C.Script(m=3, qn=4)], seed=5, udp_every=0)  # 10 frames, 3 rows
    many = C.build([C.Script(m=20, qn=4), C.Script(m=4, qn=4)], seed=6, udp_every=0)  # 24 frames, 3 rows
    assert few["n"] < 8 * few["nconns"] and many["n"] >= 8 * many["nconns"]
    run(few, None, expect_form="lane")
    run(many, None, expect_form="wave")


def test_call_order():
    """Out of turn (before any dk_tcp_rx_process, twice after one, with another n or nconns) the call is EINVAL and
    writes nothing; in turn it then still works."""
    case = case_streams("rising")
    d = Device(case)
    try:
        before = d.read()

        full = (d.d_ak, d.d_tx, d.d_rx, d.aout.nconns)

        def refused(**kw):
            with pytest.raises(Fail) as e:
                d.ack("wave", **kw)
            assert e.value.errno == 22
            d.d_ak, d.d_tx, d.d_rx, d.aout.nconns = full
            now = d.read()
            for k in OUT_KEYS:
                assert (now[k] == CANARY).all(), k
            for k in ("tx_conns", "ack_conns"):
                assert now[k].tobytes() == before[k].tobytes(), k
            assert all(np.array_equal(now["pool"][k], before["pool"][k]) for k in before["pool"])

        refused()  # no dk_tcp_rx_process yet
        d.receive()
        refused(n=case["n"] - 1)  # another n
        d.d_ak, d.d_tx, d.d_rx, d.aout.nconns = d.d_ak[:-64], d.d_tx[:-64], d.d_rx[:-288], d.aout.nconns - 1
        refused()  # another nconns
        d.d_ak = d.d_ak.new_zeros(d.d_ak.numel() + 8)[8:]
        refused()  # a misaligned table
        h, act = d.r.to_numpy(), d.out.to_numpy()["action"]
        rx_t = d.tcp.conns_to_host(d.d_rx)
        d.ack("wave")  # in turn
        got = d.read()
        exp = R.ack_process(h["flow_id"], act, h["tcp_seq"], h["tcp_ack"], h["tcp_win"], rx_t, case["tx"], case["ak"],
                            case["pool"], case["now"])
        compare(got, exp, "in turn")
        with pytest.raises(Fail):
            d.ack("wave")  # a second time on the same dk_tcp_rx_process call
        compare(d.read(), exp, "after the refused second call")
    finally:
        d.close()


def test_other_stream_is_serialised():
    """dk_tcp_ack_process on another stream than its dk_tcp_rx_process waits for it on the device: the receive call
    sits behind 100 ms of sleep on its stream and is still pending when the ACK pass has been queued on the other
    (tests/test_gpu_tcp_ctx_streams.py has the other chains of the context)."""
    import torch

    case = case_three(1)
    d = Device(case)
    try:
        c = d.case
        d.eng.receive_batch(FrameBatch.from_numpy(c["blob"], c["off"], c["lens"], device=0), d.r)
        A, B, _ = stream_pair()
        for s in (A, B):
            s.wait_stream(torch.cuda.current_stream())  # the uploads and dk_rx_process; the context's event orders the rest
        ev = delayed(A)
        d.tcp.process(d.r, d.d_rx, d.out, stream=A)
        d.ack("wave", stream=B)
        assert not ev.query(), "the delay ended while the calls were being issued: a call waited on the host"
        B.synchronize()
        h, act = d.r.to_numpy(), d.out.to_numpy()["action"]
        got = d.read()
        exp = R.ack_process(h["flow_id"], act, h["tcp_seq"], h["tcp_ack"], h["tcp_win"], got["rx_conns"], case["tx"],
                            case["ak"], case["pool"], case["now"])
        compare(got, exp, "second stream")
    finally:
        d.close()
