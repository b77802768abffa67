"""dk_tcp_tx_commit and dk_tcp_rtx_piggyback on the MI355X against tests/tcp_commit_reference.py, over real
dk_tcp_tx_segment outputs. Every case runs in both forced forms and under the engine's rule, each on fresh tables after
a segmentation call of its own; after each the outputs, the ACK table and the delayed-ACK table as bytes, every pool
entry the contract fixes (tcp_commit_reference.live_mask: all of the untouched regions and of the guard entries behind
the last region, the live range of the committed ones) are compared with the model, the TX table, the push list and
the segmentation results must be what they were, and the forms must agree byte for byte, the whole pool included.
A push.off near 2^32 is not covered: a buffer's range must lie inside src_bytes <= DK_RX_MAX_BLOB = 0xFFFFFF00, so a
wrapping offset cannot come out of a dk_tcp_tx_segment call that sent anything."""
import errno

import numpy as np
import pytest

import tcp_commit_reference as C
import tx_segment_reference as M
from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd import tcp_rtx as X
from demikernel_amd.rx import Fail
from demikernel_amd.tcp_ack import ack_conn_table, UnackedQueue
from demikernel_amd.tcp_ackemit import dack_conn_table
from demikernel_amd.tcp_cc import AFTER_SEND, cc_conn_table, cc_send, cc_to_device, cc_to_host
from demikernel_amd.tcp_commit import CommitOut, last_form, rtx_piggyback, tx_commit
from demikernel_amd.tcp_rtx import RtxResults, fire_to_device, retransmit
from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults

pytestmark = pytest.mark.gpu
NOW = 91 * 10**9 + 7
CANARY = 0x5A5A5A5A
GUARD = 5
FORMS = ("conn", "chip", None)


@pytest.fixture(scope="module")
def sender():
    s = TcpSender(0)
    yield s
    s.close()


def up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def random_pool(nq: int, seed: int = 3) -> dict:
    rng = np.random.default_rng(seed)
    return {"off": rng.integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32),
            "len": rng.integers(0, 1 << 32, nq, dtype=np.uint64).astype(np.uint32),
            "tx_time": rng.integers(0, 1 << 63, nq, dtype=np.uint64)}


def device_queue(pool: dict, nconns: int, q_cap: int) -> UnackedQueue:
    """The pool as given (its regions and the guard entries behind them) as a queue of nconns regions of q_cap."""
    q = UnackedQueue.from_numpy(pool["off"], pool["len"], pool["tx_time"])
    q.nconns, q.capacity, q.nq = nconns, q_cap, len(pool["off"])
    return q


def mss_table(nconns: int, mss=8, **kw):
    flows = synth.make_flows(nconns, passive=False)
    args = dict(snd_wnd=1 << 24, mss=mss, link=0, snd_nxt=np.arange(nconns, dtype=np.int64) * 77_003 + 0xFFFFFF00)
    args.update(kw)
    return M.conns_toward(flows, **args)


class Commit:
    """One segmentation call and its commit on fresh device tables."""

    def __init__(self, sender, tx, conn, lens, ak, pool, q_cap, dack=None, max_frames=None, seg_frames=None, stride=64):
        import torch

        self.sender, self.q_cap, self.nconns = sender, q_cap, len(ak)
        self.ak, self.pool, self.dack = ak, pool, dack
        src, self.pc, self.po, self.pl = M.pack_push(conn, lens)
        self.push = PushList.from_numpy(self.pc, self.po, self.pl)
        self.max_frames = max_frames if max_frames is not None else max(int(np.sum(np.maximum(1, -(-self.pl.astype(np.int64) // 8)))), 1)
        self.res = TcpTxResults(self.max_frames, len(self.pc))
        self.d_tx, self.d_ak = up(tx), up(ak)
        self.d_dack = None if dack is None else up(dack)
        self.queue = device_queue(pool, self.nconns, q_cap)
        self.d_src = torch.from_numpy(src).cuda()
        self.d_links = up(M.links_table())
        self.d_out = torch.zeros(self.max_frames * stride, dtype=torch.uint8, device="cuda")
        self.stride = stride
        self.seg_frames = seg_frames
        self.out = CommitOut(self.nconns, fill=CANARY)

    def segment(self):
        import torch

        self.sender.segment(self.d_src, self.push, self.d_tx, self.d_links, self.d_out, self.res,
                            slot_stride=self.stride, max_frames=self.seg_frames)
        torch.cuda.synchronize()
        self.h = self.res.to_numpy()
        self.tx_after = self.d_tx.cpu().numpy().copy()
        return self.h

    def commit(self, form, now=NOW, **kw):
        tx_commit(self.sender, self.push, self.res, self.d_ak, self.queue, now, self.out, dack=self.d_dack, form=form,
                  max_frames=self.seg_frames, **kw)
        return self.read()

    def read(self) -> dict:
        import torch

        torch.cuda.synchronize()
        got = self.out.to_numpy()
        got.update(ack_conns=self.d_ak.cpu().numpy().view(N.ACK_CONN_DTYPE).copy(), pool=self.queue.to_numpy(),
                   dack=None if self.d_dack is None else self.d_dack.cpu().numpy().view(N.DACK_CONN_DTYPE).copy())
        return got

    def check_inputs_untouched(self, ctx):
        h2 = self.res.to_numpy()
        assert all(np.array_equal(h2[k], self.h[k]) for k in self.h if k not in ("n_frames", "frames_written")), ctx
        assert h2["n_frames"] == self.h["n_frames"] and np.array_equal(self.d_tx.cpu().numpy(), self.tx_after), ctx
        for a, b in ((self.push.conn, self.pc), (self.push.off, self.po), (self.push.len, self.pl)):
            assert np.array_equal(a.cpu().numpy().view(np.uint32), b), ctx


def same(got: dict, exp: dict, q_cap: int, ctx: str):
    for k in ("status", "appended"):
        assert np.array_equal(got[k], exp[k]), f"{ctx}: {k} {got[k]} expected {exp[k]}"
    g, e = got["ack_conns"], exp["ack_conns"]
    rows = [c for c in range(len(g)) if g[c].tobytes() != e[c].tobytes()]
    assert not rows, f"{ctx}: ACK rows {rows}: got {g[rows]} expected {e[rows]}"
    mask = C.live_mask(exp, q_cap, len(got["pool"]["off"]))
    for k, v in exp["pool"].items():
        bad = np.nonzero((got["pool"][k] != v) & mask)[0][:8]
        assert not len(bad), f"{ctx}: pool {k} differs at {bad}: got {got['pool'][k][bad]} expected {v[bad]}"
    if exp["dack"] is not None:
        assert got["dack"].tobytes() == exp["dack"].tobytes(), f"{ctx}: dack {got['dack']} expected {exp['dack']}"


def run(sender, tx, conn, lens, ak, pool, q_cap, dack=None, forms=FORMS, want_rule=None, **kw) -> dict:
    """The case in every form; returns the model's result and the segmentation results."""
    first = None
    for form in forms:
        cm = Commit(sender, tx, conn, lens, ak, pool, q_cap, dack=dack, **kw)
        h = cm.segment()
        got = cm.commit(form)
        ran = last_form(sender)
        assert ran == (form or want_rule or ran), (form, ran)
        exp = C.tx_commit(cm.pc, cm.po, h, ak, pool, q_cap, NOW, dack=dack)
        ctx = f"{form or 'rule'} form ({ran})"
        same(got, exp, q_cap, ctx)
        cm.check_inputs_untouched(ctx)
        if first is None:
            first = got
        else:
            assert got["ack_conns"].tobytes() == first["ack_conns"].tobytes(), ctx
            assert all(np.array_equal(got["pool"][k], first["pool"][k]) for k in got["pool"]), ctx
    exp["h"] = h
    return exp


# ---------------------------------------------------------------------------------------------------------------------
# placement
# ---------------------------------------------------------------------------------------------------------------------
Q = 200
#          q_first - region start, q_count, frames pushed (8 bytes each)
EDGES = [(140, 50, 10),            # 0  ends exactly at the region's end: in place
         (140, 50, 11),            # 1  one more frame: the live entries move
         (4_000_000_000, 0, 3),    # 2  an empty queue whose q_first points anywhere
         (3, 130, 68),             # 3  130 entries move by 3: longer than two chunks, the shift inside a chunk
         (64, 130, 7),             # 4  the shift exactly a chunk
         (65, 130, 6),             # 5  and one more
         (10, 190, 10),            # 6  q_count + k == q_cap
         (5, 190, 11),             # 7  q_cap + 1: E_FULL
         (0, 1, 1),                # 8  its neighbour commits
         (0, 201, 1),              # 9  E_QUEUE: more than the region holds
         (-1, 3, 1),               # 10 E_QUEUE: starts before the region
         (199, 2, 1),              # 11 E_QUEUE: ends behind it
         (7, 20, 5)]               # 12 in place, in the middle


def test_placement_edges(sender):
    nc = len(EDGES)
    r0 = np.arange(nc, dtype=np.int64) * Q
    qf = np.array([e[0] if e[0] > Q * nc else r0[c] + e[0] for c, e in enumerate(EDGES)])
    ak = ack_conn_table(nc, q_first=qf, q_count=[e[1] for e in EDGES])
    ak["rtx_base_ns"] = 5
    pool = random_pool(nc * Q + GUARD)
    exp = run(sender, mss_table(nc), list(range(nc)), [8 * e[2] for e in EDGES], ak, pool, Q)
    assert exp["k"].tolist() == [e[2] for e in EDGES]
    want = [0] * nc
    want[7], want[9], want[10], want[11] = C.E_FULL, C.E_QUEUE, C.E_QUEUE, C.E_QUEUE
    assert exp["status"].tolist() == want
    e = exp["ack_conns"]
    assert (e["q_first"] - r0).tolist()[:9] == [140, 0, 0, 0, 0, 0, 0, 5, 0] and e["q_first"][12] == r0[12] + 7
    assert e["q_count"].tolist()[:9] == [60, 61, 3, 198, 137, 136, 200, 190, 2]
    assert e[[7, 9, 10, 11]].tobytes() == ak[[7, 9, 10, 11]].tobytes()
    for c in (3, 4, 5):  # the moved entries are the old live ones, in order
        a, b = int(qf[c]), int(r0[c])
        assert all(np.array_equal(exp["pool"][k][b:b + 130], pool[k][a:a + 130]) for k in pool)


# ---------------------------------------------------------------------------------------------------------------------
# which frames
# ---------------------------------------------------------------------------------------------------------------------
def which_frames_case():
    nc, q = 10, 24
    tx = mss_table(nc)
    tx["snd_wnd"][1] = 27          # 8 + 8 + 8 + 3, then the window is closed
    tx["fin_sent"][4] = 1
    tx["state"][5] = N.DK_TCP_CLOSED
    pushes = {0: [20, 13, 5], 1: [40, 10, 0], 2: [10, 0, 5], 3: [0], 4: [5], 5: [5, 6], 7: [9], 9: [30], nc: [4]}
    conn = [c for c, ls in pushes.items() for _ in ls]
    lens = [ln for ls in pushes.values() for ln in ls]
    ak = ack_conn_table(nc, q_first=np.arange(nc) * q + 2, q_count=3)
    for c in (6, 8):               # no buffer at all: their rows are garbage and stay so
        ak["q_first"][c], ak["q_count"][c], ak["rtx_armed"][c] = 0xFFFFFFF0, 0xFFFF0000, 9
    ak["q_count"][4] = 4_000_000   # sends nothing either
    return nc, q, tx, conn, lens, ak


def test_which_frames(sender):
    nc, q, tx, conn, lens, ak = which_frames_case()
    pool = random_pool(nc * q + GUARD, seed=4)
    dack = dack_conn_table(nc, delay_ns=40_000_000)
    dack["armed"], dack["deadline_ns"] = [1, 1, 0, 1, 1, 1, 1, 3, 1, 1], np.arange(nc) + NOW
    exp = run(sender, tx, conn, lens, ak, pool, q, dack=dack)
    h = exp["h"]
    S = M
    assert h["status"].tolist() == [S.SENT] * 3 + [S.PARTIAL, S.UNSENT, S.UNSENT] + [S.SENT, S.SENT, S.CLOSED] + \
        [S.SENT, S.CLOSED, S.E_CONN, S.E_CONN, S.SENT, S.SENT, S.E_CONN]
    assert exp["k"].tolist() == [3 + 2 + 1, 4, 2 + 1, 1, 0, 0, 0, 2, 0, 4] and not exp["status"].any()
    p, e = exp["pool"], exp["ack_conns"]
    at = lambda c: slice(int(e["q_first"][c]) + 3, int(e["q_first"][c]) + int(e["q_count"][c]))  # noqa: E731
    o = [int(v) for v in np.cumsum([0] + lens[:-1])]  # pack_push packs back to back
    assert p["off"][at(0)].tolist() == [o[0], o[0] + 8, o[0] + 16, o[1], o[1] + 8, o[2]]  # within restarts per buffer
    assert p["len"][at(0)].tolist() == [8, 8, 4, 8, 5, 5]
    assert p["len"][at(1)].tolist() == [8, 8, 8, 3] and p["off"][at(1)].tolist() == [o[3] + 8 * j for j in range(4)]
    assert p["len"][at(2)].tolist() == [8, 2, 0] and p["len"][at(3)].tolist() == [0]  # the FIN is the marker
    assert p["off"][at(2)][2] == o[7] and p["off"][at(3)][0] == o[9]
    assert e[[4, 5, 6, 8]].tobytes() == ak[[4, 5, 6, 8]].tobytes()
    assert exp["dack"]["armed"].tolist() == [0, 0, 0, 0, 1, 1, 1, 0, 1, 0]
    assert np.array_equal(exp["dack"]["deadline_ns"], dack["deadline_ns"])
    for k in pool:  # the guard entries, and the regions of the connections that sent nothing
        assert np.array_equal(p[k][nc * q:], pool[k][nc * q:])
        for c in (4, 5, 6, 8):
            assert np.array_equal(p[k][c * q:(c + 1) * q], pool[k][c * q:(c + 1) * q])


def test_dack_is_optional_and_cleared_on_e_full(sender):
    nc, q = 4, 6
    ak = ack_conn_table(nc, q_first=np.arange(nc) * q, q_count=[0, 5, 0, 0])
    dack = dack_conn_table(nc, delay_ns=1)
    dack["armed"], dack["deadline_ns"], dack["reserved1"] = [1, 1, 1, 1], 99, 0x1234
    pool = random_pool(nc * q)
    exp = run(sender, mss_table(nc), [1, 3], [16, 8], ak, pool, q, dack=dack)
    assert exp["status"].tolist() == [0, C.E_FULL, 0, 0] and exp["dack"]["armed"].tolist() == [1, 0, 1, 0]
    assert exp["dack"][[0, 2]].tobytes() == dack[[0, 2]].tobytes()
    run(sender, mss_table(nc), [1, 3], [16, 8], ak, pool, q, dack=None)


def test_timer(sender):
    nc, q = 4, 8
    ak = ack_conn_table(nc, q_first=np.arange(nc) * q)
    ak["rtx_armed"], ak["rtx_base_ns"] = [0, 1, 7, 0], [11, 12, 13, 14]
    exp = run(sender, mss_table(nc), [0, 1, 2], [8, 8, 8], ak, random_pool(nc * q), q)
    e = exp["ack_conns"]
    assert e["rtx_armed"].tolist() == [1, 1, 7, 0] and e["rtx_base_ns"].tolist() == [NOW, 12, 13, 14]


# ---------------------------------------------------------------------------------------------------------------------
# the turn
# ---------------------------------------------------------------------------------------------------------------------
def einval(fn):
    with pytest.raises(Fail) as e:
        fn()
    assert e.value.errno == errno.EINVAL


def test_turn():
    nc, q = 3, 8
    ak = ack_conn_table(nc, q_first=np.arange(nc) * q)
    pool = random_pool(nc * q)
    s = TcpSender(0)  # a context that has not segmented yet
    try:
        cm = Commit(s, mss_table(nc), [0, 2], [20, 8], ak, pool, q)
        before = cm.read()
        einval(lambda: cm.commit("conn"))  # no segmentation call before it
        cm.segment()
        einval(lambda: cm.commit("conn", nbufs=1))  # another nbufs
        einval(lambda: cm.commit("conn", now=N.DK_TCP_TX_TIME_NONE))
        after = cm.read()
        assert after["ack_conns"].tobytes() == before["ack_conns"].tobytes() == ak.tobytes()
        assert all(np.array_equal(after["pool"][k], pool[k]) for k in pool)
        assert (after["status"] == CANARY).all() and (after["appended"] == CANARY).all()
        got = cm.commit(None)
        exp = C.tx_commit(cm.pc, cm.po, cm.h, ak, pool, q, NOW)
        same(got, exp, q, "the commit in turn")
        einval(lambda: cm.commit("conn"))  # twice
        einval(lambda: cm.commit("chip"))
        again = cm.read()
        assert again["ack_conns"].tobytes() == got["ack_conns"].tobytes()
        assert all(np.array_equal(again["pool"][k], got["pool"][k]) for k in pool)
        cm.segment()  # the next call (the windows are wide open: the same frames again) has a turn of its own
        got2 = cm.commit("chip")
        same(got2, C.tx_commit(cm.pc, cm.po, cm.h, got["ack_conns"], got["pool"], q, NOW), q, "the second turn")
    finally:
        s.close()


def test_commit_after_no_room_changes_nothing(sender):
    nc, q = 3, 8
    ak = ack_conn_table(nc, q_first=[3, 77, 5], q_count=[1, 0, 9])
    pool = random_pool(nc * q)
    dack = dack_conn_table(nc, delay_ns=1)
    dack["armed"] = 1
    for form in FORMS:
        cm = Commit(sender, mss_table(nc), [0, 1, 2], [20, 8, 30], ak, pool, q, dack=dack, max_frames=16, seg_frames=4)
        h = cm.segment()
        assert h["frames_written"] == 0 and h["n_frames"] == 8 and (h["status"] == N.DK_TCP_TX_NO_ROOM).all()
        got = cm.commit(form)
        assert not got["status"].any() and not got["appended"].any()
        assert got["ack_conns"].tobytes() == ak.tobytes() and got["dack"].tobytes() == dack.tobytes()
        assert all(np.array_equal(got["pool"][k], pool[k]) for k in pool)


def test_order_with_cc_send_is_free(sender):
    import torch

    nc, q = 5, 16
    tx = mss_table(nc, cwnd=6000)
    ak = ack_conn_table(nc, q_first=np.arange(nc) * q + 1, q_count=2)
    ak["rto"] = 0.25
    cc = cc_conn_table(nc, mss=8, now_ns=NOW - 10**8)
    cc["ltci"] = 16
    pool = random_pool(nc * q)
    seen = []
    for commit_first in (True, False):
        cm = Commit(sender, tx, [0, 1, 1, 3], [24, 8, 3, 0], ak, pool, q)
        d_cc = cc_to_device(cc)
        status = torch.zeros(nc, dtype=torch.int32, device="cuda")
        cm.segment()
        hook = lambda: cc_send(sender, AFTER_SEND, cm.d_tx, cm.d_ak, d_cc, NOW, status, push=cm.push, res=cm.res)  # noqa: E731
        if commit_first:
            got = cm.commit(None)
            hook()
        else:
            hook()
            got = cm.commit(None)
        torch.cuda.synchronize()
        same(got, C.tx_commit(cm.pc, cm.po, cm.h, ak, pool, q, NOW), q, f"commit first: {commit_first}")
        seen.append((got["ack_conns"].tobytes(), cm.d_tx.cpu().numpy().tobytes(), cc_to_host(d_cc).tobytes(),
                     status.cpu().numpy().tobytes(), [got["pool"][k].tobytes() for k in pool]))
    assert seen[0] == seen[1]
    assert cc_to_host(d_cc).tobytes() != cc.tobytes()  # the hook did run


# ---------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_one_connection_many_frames(sender):
    """3,000 frames behind a queue of 1,000 that has to move first: the chip form's ground (and the rule's choice)."""
    q = 4096
    ak = ack_conn_table(1, q_first=500, q_count=1000)
    ak["rtx_armed"], ak["rtx_base_ns"] = 1, 4
    exp = run(sender, mss_table(1), [0], [24_000], ak, random_pool(q + GUARD), q, want_rule="chip")
    assert exp["k"].tolist() == [3000] and exp["ack_conns"]["q_first"][0] == 0 and exp["ack_conns"]["q_count"][0] == 4000
    assert np.array_equal(exp["pool"]["off"][1000:4000], np.arange(3000, dtype=np.uint32) * 8)


def test_many_connections(sender):
    nc, q = 1024, 8
    rng = np.random.default_rng(8)
    frames = rng.integers(1, 4, nc)
    qc = rng.integers(0, 8, nc)
    ak = ack_conn_table(nc, q_first=np.arange(nc) * q + np.minimum(rng.integers(0, 3, nc), q - qc), q_count=qc)
    ak["rtx_armed"] = rng.integers(0, 2, nc)
    exp = run(sender, mss_table(nc), list(range(nc)), (frames * 8 - rng.integers(0, 8, nc)).tolist(), ak,
              random_pool(nc * q + GUARD, seed=9), q, want_rule="conn")
    assert np.array_equal(exp["k"], frames) and len(set(exp["status"].tolist())) == 2  # OK and E_FULL both occur
    assert (exp["status"] == C.E_FULL).sum() == (qc + frames > q).sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# dk_tcp_rtx_piggyback
# ---------------------------------------------------------------------------------------------------------------------
def test_rtx_piggyback(sender):
    import torch

    nc = 6
    tx = mss_table(nc, snd_una=np.arange(nc, dtype=np.int64) * 77_003 + 0xFFFFFF00 - 8)
    tx["state"][4] = N.DK_TCP_CLOSED
    ak = ack_conn_table(nc, q_first=np.arange(nc), q_count=[1, 0, 1, 1, 1, 1])
    ak["rtx_armed"] = 1
    pool = {"off": np.zeros(nc, np.uint32), "len": np.full(nc, 8, np.uint32), "tx_time": np.full(nc, 5, np.uint64)}
    fire = np.array([X.FIRE_TIMEOUT, X.FIRE_TIMEOUT, X.FIRE_NONE, X.FIRE_FAST, X.FIRE_FAST, 9], np.uint8)
    dack = dack_conn_table(nc, delay_ns=3)
    dack["armed"], dack["deadline_ns"] = [1, 1, 1, 2, 1, 1], 77
    d_dack, queue = up(dack), device_queue(pool, nc, 1)
    res = RtxResults(nc, nc)
    retransmit(sender, torch.zeros(64, dtype=torch.uint8, device="cuda"), fire_to_device(fire), up(tx), up(ak), queue,
               NOW, up(M.links_table()), torch.zeros(nc * 64, dtype=torch.uint8, device="cuda"), res, slot_stride=64)
    torch.cuda.synchronize()
    st = res.to_numpy()["status"]
    assert st.tolist() == [X.SENT, X.IDLE, X.NOT_FIRED, X.SENT, X.E_STATE, X.E_FIRE]
    for _ in range(2):  # idempotent
        rtx_piggyback(sender, res, d_dack)
        torch.cuda.synchronize()
        got = d_dack.cpu().numpy().view(N.DACK_CONN_DTYPE)
        assert got.tobytes() == C.rtx_piggyback(st, dack).tobytes() and got["armed"].tolist() == [0, 1, 1, 0, 1, 1]
    assert np.array_equal(res.to_numpy()["status"], st)
