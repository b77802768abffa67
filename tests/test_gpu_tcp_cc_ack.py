"""dk_tcp_cc_ack on the MI355X against tests/tcp_cc_reference.py (pinned on the CPU by tests/test_tcp_cc_model.py). The
batch of tests/tcp_cc_cases.py goes through dk_tcp_rx_process first, so the actions and the order by connection are the
engine's own. Every table, output and untouched byte is compared whole: status, new_acks, dup_acks and the per-segment
cwnd_after over a canary fill, the congestion-control table and the TX table as bytes, the receive and ACK tables
unchanged."""
import errno
import functools

import numpy as np
import pytest

import tcp_cc_cases as C
import tcp_cc_reference as R
import tx_segment_reference as M
from demikernel_amd import _native as N
from demikernel_amd.rx import Fail
from demikernel_amd.tcp import TcpOut, TcpReceiver
from demikernel_amd.tcp_ack import TcpAcker, TcpAckOut, UnackedQueue
from demikernel_amd.tcp_ackemit import AckEmitResults, ack_emit, dack_to_device, dack_to_host
from demikernel_amd.tcp_cc import CcAckOut, cc_ack, cc_to_device, cc_to_host
from test_gpu_tcp import rx_device

pytestmark = pytest.mark.gpu
CANARY = 0x5A5A5A5A
LINKS = M.links_table()


class Device:
    """One case on the device up to and including dk_tcp_rx_process."""

    def __init__(self, case: dict):
        import torch

        self.case, self.n, self.nrows = case, case["n"], case["nconns"]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()  # noqa: E731
        self.tcp = TcpReceiver(0)
        self.r = rx_device(case["rx"])
        self.d_rx = self.tcp.conns_to_device(case["table"])
        self.d_tx, self.d_ak, self.d_cc = up(case["tx"]), up(case["ak"]), cc_to_device(case["cc"])
        self.d_dack, self.d_links = dack_to_device(case["dack"]), up(LINKS)
        self.q = UnackedQueue.from_numpy(case["pool"]["off"], case["pool"]["len"], case["pool"]["tx_time"])
        self.out = TcpOut(self.n, self.nrows)
        self.res = CcAckOut(self.n, self.nrows, fill=CANARY)
        self.aout = TcpAckOut(self.n, self.nrows)
        self.eres = AckEmitResults(self.n, self.nrows, self.n)
        self.d_frames = torch.zeros(max(self.n, 1) * 64, dtype=torch.uint8, device=self.d_rx.device)

    def receive(self):
        self.tcp.process(self.r, self.d_rx, self.out)

    def cc(self, **kw):
        cc_ack(self.tcp, self.r, self.out, self.d_rx, self.d_tx, self.d_ak, self.d_cc, self.case["now"], self.res, **kw)

    def ack(self):
        TcpAcker("lane").process(self.tcp, self.r, self.out, self.d_rx, self.d_tx, self.d_ak, self.q, self.case["now"],
                                 self.aout)

    def emit(self):
        ack_emit(self.tcp, self.r, self.out, self.d_rx, self.d_tx, self.d_dack, self.d_links, self.case["now"],
                 self.d_frames, self.eres, slot_stride=64)

    def read(self) -> dict:
        import torch

        torch.cuda.synchronize()
        got = self.res.to_numpy()
        got.update(cc=cc_to_host(self.d_cc), tx=self.d_tx.cpu().numpy().view(N.TX_CONN_DTYPE).copy(),
                   ak=self.d_ak.cpu().numpy().tobytes(), table=self.tcp.conns_to_host(self.d_rx),
                   action=self.out.to_numpy()["action"])
        return got

    def close(self):
        self.tcp.close()


def reference(case: dict, action) -> dict:
    segs = C.segs_by_conn(case["rx"]["flow_id"], action, case["rx"]["tcp_ack"], case["nconns"])
    tx, cc = case["tx"].copy(), case["cc"].copy()
    exp = R.cc_ack(segs, case["table"], tx, case["ak"], cc, case["now"], case["n"])
    exp.update(tx=tx, cc=cc, segs=segs)
    return exp


def compare(got: dict, exp: dict, ctx: str = ""):
    for k in ("status", "new_acks", "dup_acks", "cwnd_after"):
        if not np.array_equal(got[k], exp[k]):
            bad = np.nonzero(got[k] != exp[k])[0][:8]
            raise AssertionError(f"{ctx}: {k} differs at {bad}: got {got[k][bad]} expected {exp[k][bad]}")
    for k in ("cc", "tx"):
        rows = [c for c in range(len(exp[k])) if got[k][c].tobytes() != exp[k][c].tobytes()]
        assert not rows, f"{ctx}: {k} differs at rows {rows[:4]}: got {got[k][rows[:4]]} expected {exp[k][rows[:4]]}"


@functools.lru_cache(maxsize=None)
def walked():
    """The walk case on the device and its restatement, computed once for the tests below."""
    case = C.walk_case()
    d = Device(case)
    try:
        d.receive()
        before = d.tcp.conns_to_host(d.d_rx)  # dk_tcp_rx_process moved RCV.NXT; nothing after it may
        d.cc()
        got = d.read()
    finally:
        d.close()
    assert np.array_equal(got["action"], C.host_actions(case)), "the engine's actions are not the restatement's"
    return case, got, reference(case, got["action"]), before


def test_walk_case_whole():
    case, got, exp, before = walked()
    assert case["n"] <= 4096
    compare(got, exp)
    assert got["ak"] == case["ak"].tobytes() and got["table"].tobytes() == before.tobytes()
    # per-segment: every visited frame carries the window as it stood behind it, every other frame 0
    visited = np.isin(got["action"], R.VISITED)
    ok = np.isin(case["rx"]["flow_id"], np.nonzero((exp["status"] == R.OK) & (case["cc"]["flags"] & R.CUBIC != 0))[0])
    assert (got["cwnd_after"][~(visited & ok)] == 0).all() and (visited & ok).sum() == 5 * 208 + 2 * 200 + 110
    visits = [sum(a in R.VISITED for _, a, _ in s) for s in exp["segs"]]
    assert set(C.VISITS) <= set(visits)


def test_failing_and_none_rows_stay_byte_for_byte():
    case, got, exp, _ = walked()
    seen = set()
    for c in range(case["nconns"]):
        none = not case["cc"]["flags"][c] & R.CUBIC
        if got["status"][c] != R.OK or none:
            seen.add("NONE" if got["status"][c] == R.OK else R.OK + int(got["status"][c]))
            assert got["cc"][c].tobytes() == case["cc"][c].tobytes(), c
            assert got["tx"][c].tobytes() == case["tx"][c].tobytes(), c
            assert got["new_acks"][c] == got["dup_acks"][c] == 0
    assert seen == {"NONE", R.E_STATE, R.E_SND_NXT, R.E_MSS, R.E_RTO}


def small_case():
    return C.build([C.Script(m=m, phase=p) for m, p in ((9, "fresh"), (70, "avoidance"), (33, "recovery"))], seed=21)


def test_turn_rules():
    case = small_case()
    d = Device(case)
    try:
        # not before any dk_tcp_rx_process call
        with pytest.raises(Fail) as e:
            d.cc()
        assert e.value.errno == errno.EINVAL
        d.receive()
        for kw in (dict(n=case["n"] - 1),):  # another n than the call it follows
            with pytest.raises(Fail) as e:
                d.cc(**kw)
            assert e.value.errno == errno.EINVAL
        d.cc()
        first = d.read()
        with pytest.raises(Fail) as e:  # twice
            d.cc()
        assert e.value.errno == errno.EINVAL
        again = d.read()
        assert again["cc"].tobytes() == first["cc"].tobytes() and again["tx"].tobytes() == first["tx"].tobytes()
        d.ack()  # dk_tcp_ack_process after it is in turn
        import torch

        torch.cuda.synchronize()
        assert (d.aout.to_numpy()["status"][:-1] == 0).all()
        compare(first, reference(case, first["action"]), "before dk_tcp_ack_process")
        # the next batch: dk_tcp_ack_process first, then dk_tcp_cc_ack is too late and writes nothing
        d.receive()
        d.ack()
        d.res = CcAckOut(d.n, d.nrows, fill=CANARY)
        before = d.read()
        with pytest.raises(Fail) as e:
            d.cc()
        assert e.value.errno == errno.EINVAL
        after = d.read()
        assert after["cc"].tobytes() == before["cc"].tobytes() and after["tx"].tobytes() == before["tx"].tobytes()
        assert all((after[k] == CANARY).all() for k in ("status", "new_acks", "dup_acks", "cwnd_after"))
    finally:
        d.close()


def test_either_order_with_ack_emit():
    case = small_case()
    results = []
    for first in ("cc", "emit"):
        d = Device(case)
        try:
            d.receive()
            for step in (("cc", "emit") if first == "cc" else ("emit", "cc")):
                getattr(d, step)()
            got = d.read()
            got["emit"] = d.eres.to_numpy()
            got["dack"] = dack_to_host(d.d_dack).tobytes()
            got["frames"] = d.d_frames.cpu().numpy()
        finally:
            d.close()
        results.append(got)
    a, b = results
    compare(a, reference(case, a["action"]), "cc first")
    compare(b, reference(case, b["action"]), "emit first")
    assert a["dack"] == b["dack"] and np.array_equal(a["frames"], b["frames"]) and a["emit"]["n_frames"] > 0
    for k in ("status", "n_acks", "ack_frame", "off_out", "len_out"):
        assert np.array_equal(a["emit"][k], b["emit"][k]), k


def test_without_cwnd_after():
    import torch

    case = C.build([C.Script(m=12, phase="avoidance")], seed=4)
    d = Device(case)
    try:
        d.receive()
        d.res = CcAckOut(d.n, d.nrows, cwnd_after=False, fill=CANARY)
        d.cc()
        torch.cuda.synchronize()
        got = d.res.to_numpy()
        got.update(cc=cc_to_host(d.d_cc), tx=d.d_tx.cpu().numpy().view(N.TX_CONN_DTYPE).copy())
        exp = reference(case, d.out.to_numpy()["action"])
        got["cwnd_after"] = exp["cwnd_after"]  # not asked for
        compare(got, exp)
    finally:
        d.close()
