"""The two data-plane contexts' promise "calls on one context are serialised; asynchronous on the caller's stream",
tested so that a missing order, or a scratch freed under a call in flight, shows.

Every chain runs on two streams A and B that really run side by side (ctl_calls.stream_pair) and puts about 100 ms of
sleep on A first (ctl_calls.delayed), so the first call is still pending when the second is queued on B: without the
context's own ordering B's call runs first. Uploads and result fills are done before, on the current stream, and both
streams wait for them. The calls are then issued with no host wait between them, and right after the test asserts that
the delay's event has not completed. Every call is then compared bit for bit with the Python models, in issue order,
and each chain checks on the CPU, with the models alone, that applying the second call before the first gives another
answer than the one asserted.

A context waits on the host for its last call before it frees a scratch buffer (ctl_common.h, Buf::grow). The chains
therefore run on a context that a call of the same shape has sized already, which also keeps them independent of
whether a first allocation waits, and the growth cases assert the pending delay just before the growing call, not
after it. There the first call's results must still be the model's: they are not if its scratch was freed under it."""
import numpy as np
import pytest

import tcp_ack_reference as AR
import tcp_ackemit_cases as AEC
import tcp_ackemit_reference as E
import tcp_cc_cases as CCC
import tcp_cc_reference as CR
import tcp_commit_reference as CMR
import tcp_rtx_reference as X
import test_gpu_tcp as GT
import test_gpu_tcp_ack_timer as GAT
import test_gpu_tcp_cc_send as GCS
import test_gpu_tcp_commit as GCM
import test_gpu_tcp_rtx as GRX
import test_gpu_tcp_timers as GTM
import tx_segment_reference as M
from ctl_calls import delayed, stream_pair
from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table
from demikernel_amd.tcp_ack import TcpAcker, TcpAckOut, UnackedQueue, ack_conn_table
from demikernel_amd.tcp_ackemit import AckEmitResults, ack_emit, ack_timer, dack_conn_table, dack_to_device, dack_to_host
from demikernel_amd.tcp_cc import AFTER_SEND, CcAckOut, TimersOut, cc_ack, cc_send, cc_to_device, cc_to_host, timers
from demikernel_amd.tcp_commit import CommitOut, rtx_piggyback, tx_commit
from demikernel_amd.tcp_rtx import RtxResults, fire_to_device, retransmit
from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults

pytestmark = pytest.mark.gpu

LINKS = M.links_table()
NOW = 91 * 10**9 + 7
MODES = ["in_flight", "one_stream"]


@pytest.fixture
def closing():
    made = []
    yield made.append
    for d in made:
        d.close()


@pytest.fixture
def pair():
    """(A, B): two streams that run side by side."""
    import torch

    a, b, which = stream_pair()
    print(f"\nstream pair {which} of 8 fresh streams")
    torch.cuda.synchronize()
    return a, b


def streams_for(mode, pair):
    """(the first call's stream, the later calls' stream, whether the first stream is delayed)."""
    a, b = pair
    return (a, b, True) if mode == "in_flight" else (a, a, False)


def ready(*streams):
    """The uploads and fills, queued on the current stream, come before whatever the streams run next."""
    import torch

    for s in streams:
        s.wait_stream(torch.cuda.current_stream())


def up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def same(got, exp, keys, ctx):
    for k in keys:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, (ctx, k, g.shape, e.shape)
        if g.tobytes() != e.tobytes():
            bad = np.nonzero(g.reshape(len(g), -1).view(np.uint8) != e.reshape(len(e), -1).view(np.uint8))[0][:8] if g.ndim else []
            raise AssertionError(f"{ctx}: {k} differs at {bad}: got {g[bad] if g.ndim else g} expected {e[bad] if e.ndim else e}")


def differ(a, b, keys) -> bool:
    return any(np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes() for k in keys)


# =====================================================================================================================
# The receive context: dk_tcp_rx_process, then dk_tcp_cc_ack, dk_tcp_ack_emit and dk_tcp_ack_process on its order
# =====================================================================================================================
class Batch:
    """One batch of tests/tcp_cc_cases.py or tests/tcp_ackemit_cases.py on the device, with every table and output the
    receive call and its three followers take. Tables a case does not bring are neutral ones."""

    def __init__(self, case: dict, tcp: TcpReceiver):
        import torch

        self.case, self.tcp, self.n, self.nrows = case, tcp, case["n"], case["nconns"]
        n, nrows = self.n, self.nrows
        self.now = case.get("now", NOW)
        self.ak = case["ak"] if "ak" in case else ack_conn_table(nrows, wl1=case["table"]["receive_next"], wl2=case["tx"]["snd_nxt"])
        self.pool = case.get("pool") or {"off": np.zeros(nrows, np.uint32), "len": np.zeros(nrows, np.uint32),
                                         "tx_time": np.full(nrows, N.DK_TCP_TX_TIME_NONE, np.uint64)}
        self.r = GT.rx_device(case["rx"])
        self.d_rx = tcp.conns_to_device(case["table"])
        self.d_tx, self.d_ak, self.d_links = up(case["tx"]), up(self.ak), up(LINKS)
        self.d_cc = cc_to_device(case["cc"]) if "cc" in case else None
        self.d_dack = dack_to_device(case["dack"])
        self.q = UnackedQueue.from_numpy(self.pool["off"], self.pool["len"], self.pool["tx_time"])
        self.out = TcpOut(n, nrows)
        self.cres, self.aout = CcAckOut(n, nrows, fill=0x5A5A5A5A), TcpAckOut(n, nrows, fill=0x5A5A5A5A)
        self.eres = AckEmitResults(n, nrows, n, fill=0x5A5A5A5A)
        self.d_frames = torch.full((max(n, 1) * 64,), 0xA5, dtype=torch.uint8, device="cuda")

    # the four calls, each the library call and nothing else
    def receive(self, s):
        self.tcp.process(self.r, self.d_rx, self.out, stream=s)

    def cc(self, s):
        cc_ack(self.tcp, self.r, self.out, self.d_rx, self.d_tx, self.d_ak, self.d_cc, self.now, self.cres, stream=s)

    def emit(self, s):
        ack_emit(self.tcp, self.r, self.out, self.d_rx, self.d_tx, self.d_dack, self.d_links, self.now, self.d_frames,
                 self.eres, slot_stride=64, stream=s)

    def ack(self, s, form="wave"):
        TcpAcker(form).process(self.tcp, self.r, self.out, self.d_rx, self.d_tx, self.d_ak, self.q, self.now, self.aout,
                               stream=s)

    def read(self) -> dict:
        import torch

        torch.cuda.synchronize()
        got = {"rx": self.out.to_numpy(), "table": self.tcp.conns_to_host(self.d_rx),
               "tx": self.d_tx.cpu().numpy().view(N.TX_CONN_DTYPE).copy(),
               "ak": self.d_ak.cpu().numpy().view(N.ACK_CONN_DTYPE).copy(), "pool": self.q.to_numpy(),
               "cres": self.cres.to_numpy(), "aout": self.aout.to_numpy(), "eres": self.eres.to_numpy(),
               "dack": dack_to_host(self.d_dack), "frames": self.d_frames.cpu().numpy()}
        if self.d_cc is not None:
            got["cc"] = cc_to_host(self.d_cc)
        return got


def batch_models(case: dict, followers=("cc", "emit", "ack"), ak=None, pool=None) -> dict:
    """The receive call and its followers in the order given, through the models: the oracle's restatement of
    dk_tcp_rx_process, tcp_cc_reference, tcp_ackemit_reference, tcp_ack_reference."""
    from oracle import oracle as O

    n, nrows, now = case["n"], case["nconns"], case.get("now", NOW)
    rxb = case["rx"]
    table = case["table"].copy()
    m = {"rx": O.tcp_process(table, rxb), "table": table}
    action = m["rx"]["action"]
    tx = case["tx"].copy()
    ak = (case["ak"] if "ak" in case else ak).copy()
    pool = case.get("pool") or pool
    for f in followers:
        if f == "cc":
            cc = case["cc"].copy()
            segs = CCC.segs_by_conn(rxb["flow_id"], action, rxb["tcp_ack"], nrows)
            m["cres"] = CR.cc_ack(segs, table, tx, ak, cc, now, n)  # tx and cc in place
            m["cc"] = cc
        elif f == "emit":
            m["emit"] = E.ack_emit(rxb, case["table"], tx, case["dack"], LINKS, now, np.full(max(n, 1) * 64, 0xA5, np.uint8),
                                   slot_stride=64, frame_lead=0, max_frames=n)
        else:
            a = AR.ack_process(rxb["flow_id"], action, rxb["tcp_seq"], rxb["tcp_ack"], np.zeros(n, np.uint32), table, tx, ak,
                               pool, now)
            m["aout"], tx, ak, pool = a, a["tx_conns"], a["ack_conns"], a["pool"]
    m.update(tx=tx, ak=ak, pool=pool)
    return m


CC_KEYS = ("status", "new_acks", "dup_acks", "cwnd_after")
ACK_KEYS = ("acked", "status", "new_acks", "dup_acks", "bytes_acked", "samples")
EMIT_KEYS = ("status", "n_acks", "ack_frame", "off_out", "len_out", "frame_conn", "frame_seg")


def check_batch(got: dict, m: dict, ctx: str, followers=("cc", "emit", "ack")):
    GT.assert_same(got["table"], got["rx"], m["table"], m["rx"], f"{ctx}: dk_tcp_rx_process")
    if "cc" in followers:
        same(got["cres"], m["cres"], CC_KEYS, f"{ctx}: dk_tcp_cc_ack")
        same(got, m, ("cc",), f"{ctx}: dk_tcp_cc_ack")
    if "emit" in followers:
        assert got["eres"]["n_frames"] == m["emit"]["n_frames"], (ctx, got["eres"]["n_frames"], m["emit"]["n_frames"])
        same(got["eres"], m["emit"], EMIT_KEYS, f"{ctx}: dk_tcp_ack_emit")
        same(got, m["emit"], ("dack",), f"{ctx}: dk_tcp_ack_emit")
        same({"out": got["frames"]}, m["emit"], ("out",), f"{ctx}: dk_tcp_ack_emit")
    if "ack" in followers:
        same(got["aout"], m["aout"], ACK_KEYS, f"{ctx}: dk_tcp_ack_process")
        same(got["pool"], m["pool"], ("off", "len", "tx_time"), f"{ctx}: dk_tcp_ack_process")
    same(got, m, ("tx", "ak"), f"{ctx}: the tables after the last call")


def chain_case() -> dict:
    return CCC.build([CCC.Script(m=m, phase=p) for m, p in ((9, "fresh"), (70, "avoidance"), (33, "recovery"),
                                                           (64, "after_rto"), (120, "above_w_max"))], seed=31)


def test_receive_then_its_three_followers(closing, pair):
    """dk_tcp_rx_process on A behind the delay, then dk_tcp_cc_ack, dk_tcp_ack_emit and dk_tcp_ack_process on B, all
    three against the one receive call. Before the receive call the action array holds SKIP for every frame, so a
    follower that ran first would visit no segment; and dk_tcp_ack_process before dk_tcp_cc_ack moves SND.UNA under it."""
    A, B = pair
    case = chain_case()
    assert case["n"] <= 4096 and case["nconns"] <= 64
    tcp = TcpReceiver(0)
    closing(tcp)
    warm, b = Batch(case, tcp), Batch(case, tcp)
    import torch

    s0 = torch.cuda.current_stream()
    for step in (warm.receive, warm.cc, warm.emit, warm.ack):  # sizes every scratch of the context
        step(s0)
    torch.cuda.synchronize()
    ready(A, B)
    ev = delayed(A)
    b.receive(A)
    b.cc(B)
    b.emit(B)
    b.ack(B)
    assert not ev.query(), "the delay on A ended while the calls were being issued: a call waited on the host"
    m = batch_models(case)
    check_batch(b.read(), m, "receive on A, followers on B")
    # the second call before the first, on the models alone
    assert N.A["SKIP"] == 0 and m["emit"]["n_frames"] > 0 and m["cres"]["new_acks"].sum() > 0 and m["aout"]["new_acks"].sum() > 0
    none = CCC.segs_by_conn(case["rx"]["flow_id"], np.zeros(case["n"], np.uint8), case["rx"]["tcp_ack"], case["nconns"])
    assert not any(none), "a follower ahead of the receive call sees only SKIP"
    cc_first = case["cc"].copy()
    early = CR.cc_ack(none, case["table"], case["tx"].copy(), case["ak"], cc_first, case["now"], case["n"])
    assert differ(early, m["cres"], CC_KEYS) and cc_first.tobytes() != m["cc"].tobytes()
    swapped = batch_models(case, followers=("ack", "cc"))  # what the header forbids: the ACK pass first
    assert differ(swapped["cres"], m["cres"], CC_KEYS) or swapped["cc"].tobytes() != m["cc"].tobytes()


# ---- growth with work in flight -------------------------------------------------------------------------------------
def small_batch():
    return AEC.uniform(2, 25, seed=3, total=64)


def large_batch():
    return AEC.uniform(40, 80, seed=4, total=4096)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["scan_walk", "radix_sort"])
def test_receive_scratch_growth(closing, pair, mode, path):
    """dk_tcp_rx_process at n = 64 on A, then at n = 4,096 and 41 rows on B: every buffer of the order grows, and the
    scan walk's per-window buffers (walk forced) or the radix sort's temporary storage (sort forced)."""
    import torch

    s0, s1, delay = streams_for(mode, pair)
    tcp = TcpReceiver(0, walk="scan") if path == "scan_walk" else TcpReceiver(0, radix_sort=True)
    closing(tcp)
    small, large = small_batch(), large_batch()
    assert small["n"] == 64 and large["n"] == 4096 and large["nconns"] <= 64
    a, b = Batch(small, tcp), Batch(large, tcp)
    ready(s0, s1)
    ev = delayed(s0) if delay else None
    a.receive(s0)
    assert ev is None or not ev.query(), "the delay on A ended before the growing call was made: lengthen it"
    b.receive(s1)
    torch.cuda.synchronize()
    if path == "scan_walk":
        assert tcp.last_walk == "scan"
    else:
        assert tcp.last_sort == "radix"
    check_batch(a.read(), batch_models(small, (), ak=a.ak), "the small call", ())
    check_batch(b.read(), batch_models(large, (), ak=b.ak), "the growing call", ())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("follower", ["ack_chip", "emit"])
def test_follower_scratch_growth(closing, pair, mode, follower):
    """dk_tcp_ack_process in its chip form, or dk_tcp_ack_emit, after a batch of 64 frames on A; then the batch of 4,096
    on B (the receive call grows nothing: a first call of that size came before) and its follower, which needs more of
    its own scratch while the small one may still be using it."""
    import torch

    s0, s1, delay = streams_for(mode, pair)
    tcp = TcpReceiver(0)
    closing(tcp)
    small, large = small_batch(), large_batch()
    sizing, a, b = Batch(large, tcp), Batch(small, tcp), Batch(large, tcp)
    cur = torch.cuda.current_stream()
    sizing.receive(cur)
    a.receive(cur)
    torch.cuda.synchronize()
    step = (lambda x, s: x.ack(s, "chip")) if follower == "ack_chip" else (lambda x, s: x.emit(s))
    ready(s0, s1)
    ev = delayed(s0) if delay else None
    step(a, s0)
    b.receive(s1)
    assert ev is None or not ev.query(), "the delay on A ended before the growing call was made: lengthen it"
    step(b, s1)
    torch.cuda.synchronize()
    f = ("ack",) if follower == "ack_chip" else ("emit",)
    if follower == "ack_chip":
        assert TcpAcker.last_form(tcp) == "chip"
    check_batch(a.read(), batch_models(small, f, ak=a.ak, pool=a.pool), "the small batch", f)
    check_batch(b.read(), batch_models(large, f, ak=b.ak, pool=b.pool), "the growing batch", f)


# =====================================================================================================================
# The sender context
# =====================================================================================================================
class Push:
    """A push list and a dk_tcp_tx_segment call's device arrays over a TX table."""

    def __init__(self, sender, tx, conn, lens, *, stride, max_frames, rx=None, out=None, seed=9):
        import torch

        self.sender, self.tx, self.stride, self.max_frames, self.rx = sender, tx, stride, max_frames, rx
        self.src, self.pc, self.po, self.pl = M.pack_push(conn, lens, seed=seed)
        self.push = PushList.from_numpy(self.pc, self.po, self.pl)
        self.res = TcpTxResults(max_frames, len(self.pc))
        self.d_src, self.d_tx, self.d_links = up(self.src), up(tx), up(LINKS)
        self.d_rx = None if rx is None else up(rx)
        self.size = max_frames * stride + 64
        self.d_out = torch.full((self.size,), 0xA5, dtype=torch.uint8, device="cuda") if out is None else out

    def segment(self, s, res=None):
        self.sender.segment(self.d_src, self.push, self.d_tx, self.d_links, self.d_out, res or self.res,
                            slot_stride=self.stride, rx_conns=self.d_rx, stream=s)

    def model(self, tx=None, out=None) -> dict:
        out = np.full(self.size, 0xA5, np.uint8) if out is None else out
        return M.segment(self.src, self.pc, self.po, self.pl, self.tx if tx is None else tx, LINKS, out,
                         slot_stride=self.stride, frame_lead=0, max_frames=self.max_frames, rx_conns=self.rx)

    def read(self, res=None) -> dict:
        got = (res or self.res).to_numpy()
        got.update(tx_conns=self.d_tx.cpu().numpy().view(N.TX_CONN_DTYPE).copy(), out=self.d_out.cpu().numpy())
        return got


SEG_KEYS = ("status", "sent", "first_frame", "frame_count", "off_out", "len_out", "frame_buf")


def check_segment(got, exp, ctx, tables=True):
    assert got["n_frames"] == exp["n_frames"], (ctx, got["n_frames"], exp["n_frames"])
    same(got, exp, SEG_KEYS + (("tx_conns", "out") if tables else ()), f"{ctx}: dk_tcp_tx_segment")


def sized(sender, *calls):
    """Calls of the chain's shapes on throwaway tables, so that the chain itself grows nothing."""
    import torch

    for c in calls:
        c(torch.cuda.current_stream())
    torch.cuda.synchronize()


def test_segment_then_segment(closing, pair):
    """Two dk_tcp_tx_segment calls of one push list: the second must see the first one's SND.NXT (connection 0's window
    is then full) and writes its frames over the first one's."""
    A, B = pair
    sender = TcpSender(0)
    closing(sender)
    tx = M.conns_toward(synth.make_flows(2, passive=False), mss=300, snd_wnd=[1000, 1 << 20])
    mk = lambda: Push(sender, tx, [0, 0, 1], [700, 700, 40], stride=384, max_frames=12)  # noqa: E731
    sized(sender, mk().segment)
    p = mk()
    r2 = TcpTxResults(12, 3)
    ready(A, B)
    ev = delayed(A)
    p.segment(A)
    p.segment(B, r2)
    assert not ev.query(), "the delay on A ended while the calls were being issued: a call waited on the host"
    import torch

    torch.cuda.synchronize()
    e1 = p.model()
    e2 = p.model(e1["tx_conns"], e1["out"])
    check_segment(p.read(), e1, "first", tables=False)
    check_segment(p.read(r2), e2, "second")
    assert list(e1["status"]) == [M.SENT, M.PARTIAL, M.SENT] and list(e2["status"]) == [M.UNSENT, M.UNSENT, M.SENT]
    assert differ(e1, e2, ("status", "sent"))  # the two result sets swapped are not the ones asserted


def commit_case(nc, frames_of, q=16, seed=8):
    rng = np.random.default_rng(seed)
    frames = np.array([frames_of(c) for c in range(nc)])
    ak = ack_conn_table(nc, q_first=np.arange(nc) * q + 1, q_count=rng.integers(0, 4, nc))
    ak["rtx_armed"] = rng.integers(0, 2, nc)
    dack = dack_conn_table(nc, armed=1, deadline_ns=77)
    return GCM.mss_table(nc), list(range(nc)), (frames * 8 - rng.integers(0, 8, nc)).tolist(), ak, GCM.random_pool(nc * q + GCM.GUARD, seed), q, dack


class Committed:
    """A push list cut by dk_tcp_tx_segment and committed by dk_tcp_tx_commit (8-byte segments in 64-byte slots)."""

    def __init__(self, sender, case, form=None):
        tx, conn, lens, self.ak, self.pool, self.q_cap, self.dack = case
        frames = int(np.sum(np.maximum(1, -(-np.asarray(lens) // 8))))
        self.p = Push(sender, tx, conn, lens, stride=64, max_frames=frames)
        self.sender, self.form, nc = sender, form, len(self.ak)
        self.d_ak, self.d_dack = up(self.ak), up(self.dack)
        self.queue = GCM.device_queue(self.pool, nc, self.q_cap)
        self.out = CommitOut(nc, fill=0x5A5A5A5A)

    def commit(self, s):
        tx_commit(self.sender, self.p.push, self.p.res, self.d_ak, self.queue, NOW, self.out, dack=self.d_dack,
                  form=self.form, stream=s)

    def check(self, ctx):
        import torch

        torch.cuda.synchronize()
        seg = self.p.model()
        check_segment(self.p.read(), seg, ctx)
        exp = CMR.tx_commit(self.p.pc, self.p.po, seg, self.ak, self.pool, self.q_cap, NOW, dack=self.dack)
        got = self.out.to_numpy()
        got.update(ack_conns=self.d_ak.cpu().numpy().view(N.ACK_CONN_DTYPE).copy(), pool=self.queue.to_numpy(),
                   dack=self.d_dack.cpu().numpy().view(N.DACK_CONN_DTYPE).copy())
        GCM.same(got, exp, self.q_cap, f"{ctx}: dk_tcp_tx_commit")
        return seg, exp


def test_segment_then_commit(closing, pair):
    """dk_tcp_tx_commit on B reads the results of the dk_tcp_tx_segment call pending on A. Ahead of it those hold no
    frame (zero-filled: frame_count 0), and nothing would be appended."""
    A, B = pair
    sender = TcpSender(0)
    closing(sender)
    case = commit_case(32, lambda c: 1 + c % 4)
    w = Committed(sender, case, "chip")
    sized(sender, w.p.segment, w.commit)
    c = Committed(sender, case, "chip")
    ready(A, B)
    ev = delayed(A)
    c.p.segment(A)
    c.commit(B)
    assert not ev.query(), "the delay on A ended while the calls were being issued: a call waited on the host"
    seg, exp = c.check("segment on A, commit on B")
    assert exp["appended"].sum() > 32
    blank = {k: np.zeros_like(v) for k, v in seg.items() if k in ("status", "first_frame", "frame_count")}
    blank["len_out"] = seg["len_out"]
    early = CMR.tx_commit(c.p.pc, c.p.po, blank, c.ak, c.pool, c.q_cap, NOW, dack=c.dack)
    assert early["appended"].sum() == 0 and differ(early, exp, ("appended", "ack_conns"))


def test_segment_then_timers(closing, pair):
    """dk_tcp_timers on B collapses the window (tx_conns.cwnd) of every connection whose timer fires; the
    dk_tcp_tx_segment call pending on A reads that window. Ahead of it, the timers leave it one segment's worth."""
    import torch

    A, B = pair
    sender = TcpSender(0)
    closing(sender)
    nc = 48
    tx, ak, cc, dack = GTM.tables(nc, seed=12)
    tx["snd_wnd"], tx["link"] = 1 << 24, 0
    mk = lambda: Push(sender, tx, list(range(nc)), (3 * tx["mss"] + 5).tolist(), stride=9216, max_frames=4 * nc)  # noqa: E731
    mk_t = lambda: (up(ak), cc_to_device(cc), dack_to_device(dack), TimersOut(nc, fill=0x5A5A5A5A))  # noqa: E731
    w, (w_ak, w_cc, w_dack, w_out) = mk(), mk_t()
    sized(sender, w.segment, lambda s: timers(sender, w.d_tx, w_ak, w_cc, GTM.NOW, w_out, dack=w_dack, stream=s))
    p, (d_ak, d_cc, d_dack, out) = mk(), mk_t()
    ready(A, B)
    ev = delayed(A)
    p.segment(A)
    timers(sender, p.d_tx, d_ak, d_cc, GTM.NOW, out, dack=d_dack, stream=B)
    assert not ev.query(), "the delay on A ended while the calls were being issued: a call waited on the host"
    torch.cuda.synchronize()
    seg = p.model()
    etx, ecc = seg["tx_conns"].copy(), cc.copy()
    exp = CR.timers(etx, ak, ecc, GTM.NOW, dack)
    got = p.read()
    check_segment(got, dict(seg, tx_conns=etx), "segment on A, timers on B")
    g = out.to_numpy()
    same(g, exp, ("status", "rtx_fire", "ack_fire"), "dk_tcp_timers")
    assert (g["n_fast"], g["n_timeout"], g["n_ack"]) == (exp["n_fast"], exp["n_timeout"], exp["n_ack"]) and exp["n_timeout"] > 0
    same({"cc": cc_to_host(d_cc)}, {"cc": ecc}, ("cc",), "dk_tcp_timers")
    rtx, rcc = tx.copy(), cc.copy()  # the timers first: the segmentation then sees the collapsed windows
    CR.timers(rtx, ak, rcc, GTM.NOW, dack)
    assert differ(p.model(rtx), seg, ("status", "sent"))


def test_segment_then_cc_send(closing, pair):
    """dk_tcp_cc_send (after the send) on B reads the results of the dk_tcp_tx_segment call pending on A, and SND.NXT as
    that call leaves it: per connection it spends the limited-transmit increase frame by frame. Ahead of that call the
    results hold no frame (zero-filled) and no row changes."""
    import torch

    A, B = pair
    sender = TcpSender(0)
    closing(sender)
    tx, ak, cc = GCS.tables()
    conn = [c for c, lens in GCS.PUSHES.items() for _ in lens]
    lens = [ln for lens_ in GCS.PUSHES.values() for ln in lens_]
    now = GCS.NOW + 5

    def world():
        p = Push(sender, tx, conn, lens, stride=1100, max_frames=32)
        return p, up(ak), cc_to_device(cc), torch.full((GCS.NC,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")

    def call(w, s):
        p, d_ak, d_cc, status = w
        cc_send(sender, AFTER_SEND, p.d_tx, d_ak, d_cc, now, status, push=p.push, res=p.res, stream=s)

    w = world()
    sized(sender, w[0].segment, lambda s: call(w, s))
    w = world()
    p, d_ak, d_cc, status = w
    ready(A, B)
    ev = delayed(A)
    p.segment(A)
    call(w, B)
    assert not ev.query(), "the delay on A ended while the calls were being issued: a call waited on the host"
    torch.cuda.synchronize()
    seg = p.model()
    frames = [[] for _ in range(GCS.NC)]
    for f in range(len(seg["len_out"])):
        b = int(seg["len_out"][f]) - 54
        frames[conn[int(seg["frame_buf"][f])]].append(b if b else 1)
    etx, ecc = seg["tx_conns"].copy(), cc.copy()
    est = CR.cc_send_after(etx, ak, ecc, now, frames)
    check_segment(p.read(), dict(seg, tx_conns=etx), "segment on A, cc_send on B")
    assert np.array_equal(status.cpu().numpy().view(np.uint32), est)
    same({"cc": cc_to_host(d_cc)}, {"cc": ecc}, ("cc",), "dk_tcp_cc_send")
    assert d_ak.cpu().numpy().tobytes() == ak.tobytes()
    assert [len(f) for f in frames] == [0, 1, 5, 2, 1, 1, 3, 0, 2, 1] and ecc.tobytes() != cc.tobytes()
    early = cc.copy()  # the hook first: no frame in the results yet
    CR.cc_send_after(tx.copy(), ak, early, now, [[] for _ in range(GCS.NC)])
    assert early.tobytes() == cc.tobytes() != ecc.tobytes()


def rtx_tables(n, seed):
    lens = [1460 if c % 32 == 31 else GRX.LENS[c % 6] for c in range(n)]
    return GRX.table(lens, seed=seed)


class Rtx:
    """A dk_tcp_retransmit call's device arrays (tests/test_gpu_tcp_rtx.py's tables)."""

    def __init__(self, sender, n, seed, out=None):
        import torch

        self.sender, self.n = sender, n
        _, self.src, self.tx, self.ak, self.pool = rtx_tables(n, seed)
        self.fire = GRX.mask("kinds", n)
        self.max_frames, self.size = n + 2, (n + 2) * 1536 + 64
        self.d_src, self.d_tx, self.d_ak, self.d_links = up(self.src), up(self.tx), up(self.ak), up(LINKS)
        self.d_fire = fire_to_device(self.fire)
        self.queue = UnackedQueue.from_numpy(self.pool["off"], self.pool["len"], self.pool["tx_time"])
        self.res = RtxResults(self.max_frames, n)
        self.d_out = torch.full((self.size,), 0xA5, dtype=torch.uint8, device="cuda") if out is None else out

    def retransmit(self, s):
        retransmit(self.sender, self.d_src, self.d_fire, self.d_tx, self.d_ak, self.queue, NOW, self.d_links, self.d_out,
                   self.res, slot_stride=1536, stream=s)

    def model(self, out=None, tx=None) -> dict:
        out = np.full(self.size, 0xA5, np.uint8) if out is None else out
        return X.retransmit(self.src, self.fire, self.tx if tx is None else tx, self.ak, self.pool, NOW, LINKS, out,
                            slot_stride=1536, frame_lead=0, max_frames=self.max_frames)

    def check(self, exp, ctx):
        got = self.res.to_numpy()
        assert got["n_frames"] == exp["n_frames"], (ctx, got["n_frames"], exp["n_frames"])
        same(got, exp, ("status", "frame", "off_out", "len_out", "frame_conn"), f"{ctx}: dk_tcp_retransmit")
        same({"ack_conns": self.d_ak.cpu().numpy().view(N.ACK_CONN_DTYPE), "out": self.d_out.cpu().numpy()}, exp,
             ("ack_conns", "out"), f"{ctx}: dk_tcp_retransmit")
        same(self.queue.to_numpy(), exp["pool"], ("off", "len", "tx_time"), f"{ctx}: dk_tcp_retransmit")


def test_segment_then_retransmit_then_piggyback(closing, pair):
    """dk_tcp_tx_segment on A and dk_tcp_retransmit on B write their frames into one output blob and work on one TX
    table: the retransmissions must land over the new frames. Then dk_tcp_retransmit on A and dk_tcp_rtx_piggyback on B,
    which reads the statuses of the call pending on A; ahead of it they hold no SENT."""
    import torch

    A, B = pair
    sender = TcpSender(0)
    closing(sender)
    n = 40

    def world():
        r = Rtx(sender, n, seed=21)
        tx = r.tx.copy()
        tx["snd_wnd"], tx["link"] = 1 << 24, 0
        r.tx = tx
        r.d_tx = up(tx)
        p = Push(sender, tx, list(range(n)), [1000] * n, stride=1536, max_frames=n + 2, out=r.d_out)
        p.d_tx = r.d_tx  # one table: the retransmissions read it, the segmentation moves SND.NXT
        dack = dack_conn_table(n, armed=1, deadline_ns=77)
        return r, p, dack, up(dack)

    r, p, dack, d_dack = world()
    sized(sender, p.segment, r.retransmit, lambda s: rtx_piggyback(sender, r.res, d_dack, stream=s))
    r, p, dack, d_dack = world()
    ready(A, B)
    ev = delayed(A)
    p.segment(A)
    r.retransmit(B)
    assert not ev.query(), "the delay on A ended while the calls were being issued: a call waited on the host"
    torch.cuda.synchronize()
    seg = p.model()
    exp = r.model(seg["out"], seg["tx_conns"])
    check_segment(p.read(), seg, "segment on A", tables=False)
    r.check(exp, "segment on A, retransmit on B")
    assert seg["n_frames"] == n and exp["n_frames"] == n
    other = p.model(out=r.model()["out"])["out"]  # the retransmissions first, the new frames over them
    assert not np.array_equal(other, exp["out"])
    # the second chain, on fresh tables
    r, p, dack, d_dack = world()
    r.res.status.fill_(0)
    ready(A, B)
    ev = delayed(A)
    r.retransmit(A)
    rtx_piggyback(sender, r.res, d_dack, stream=B)
    assert not ev.query(), "the delay on A ended while the calls were being issued: a call waited on the host"
    torch.cuda.synchronize()
    exp = r.model()
    r.check(exp, "retransmit on A")
    want = CMR.rtx_piggyback(exp["status"], dack)
    assert d_dack.cpu().numpy().tobytes() == want.tobytes(), "retransmit on A, piggyback on B"
    assert (exp["status"] == X.SENT).sum() == n
    assert CMR.rtx_piggyback(np.zeros(n, np.uint32), dack).tobytes() == dack.tobytes() != want.tobytes()


def test_segment_then_ack_timer(closing, pair):
    """dk_tcp_ack_timer on B checks each connection's SND.NXT against the receive table's send_next, which here holds
    what the dk_tcp_tx_segment call pending on A will leave: ahead of that call every connection is E_SND_NXT and no
    ACK is built. Its frames go into the same output blob, over that call's."""
    import torch

    A, B = pair
    sender = TcpSender(0)
    closing(sender)
    n = 48
    tx, rx, dack, _ = GAT.table(n, seed=5)
    tx["snd_wnd"], tx["link"], tx["mss"] = 1 << 24, 0, 8
    rx["send_next"] = tx["snd_nxt"] + np.uint32(8)
    fire = GAT.mask("all", n)

    def world():
        p = Push(sender, tx, list(range(n)), [8] * n, stride=64, max_frames=n + 2)
        return p, up(rx), dack_to_device(dack), AckEmitResults(n + 2, n, fill=0x5A5A5A5A), fire_to_device(fire)

    def call(w, s):
        p, d_rx, d_dack, res, d_fire = w
        ack_timer(sender, d_fire, p.d_tx, d_rx, d_dack, p.d_links, p.d_out, res, slot_stride=64, stream=s)

    w = world()
    sized(sender, w[0].segment, lambda s: call(w, s))
    w = world()
    p, d_rx, d_dack, res, _ = w
    ready(A, B)
    ev = delayed(A)
    p.segment(A)
    call(w, B)
    assert not ev.query(), "the delay on A ended while the calls were being issued: a call waited on the host"
    torch.cuda.synchronize()
    seg = p.model()
    exp = E.ack_timer(fire, seg["tx_conns"], rx, dack, LINKS, seg["out"], slot_stride=64, frame_lead=0, max_frames=n + 2)
    check_segment(p.read(), dict(seg, out=exp["out"]), "segment on A, ack_timer on B")
    got = res.to_numpy()
    assert got["n_frames"] == exp["n_frames"] > 0 and seg["n_frames"] == n
    same(got, exp, ("status", "n_acks", "ack_frame", "off_out", "len_out", "frame_conn"), "dk_tcp_ack_timer")
    assert dack_to_host(d_dack).tobytes() == exp["dack"].tobytes()
    early = E.ack_timer(fire, tx, rx, dack, LINKS, np.full(p.size, 0xA5, np.uint8), slot_stride=64, frame_lead=0,
                        max_frames=n + 2)
    assert early["n_frames"] == 0 and (early["status"] == E.E_SND_NXT).all()


# ---- growth with work in flight -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_segment_scratch_growth(closing, pair, mode):
    """dk_tcp_tx_segment of 3 buffers on 2 connections on A, then of 4,096 buffers on 64 connections on B."""
    import torch

    s0, s1, delay = streams_for(mode, pair)
    sender = TcpSender(0)
    closing(sender)
    rng = np.random.default_rng(17)
    a = Push(sender, M.conns_toward(synth.make_flows(2, passive=False), mss=300), [0, 0, 1], [700, 700, 40], stride=384,
             max_frames=12)
    conn = np.sort(rng.integers(0, 64, 4096))
    b = Push(sender, M.conns_toward(synth.make_flows(64, passive=False), mss=32), conn, rng.choice([1, 16, 31, 33], 4096),
             stride=96, max_frames=2 * 4096)
    ready(s0, s1)
    ev = delayed(s0) if delay else None
    a.segment(s0)
    assert ev is None or not ev.query(), "the delay on A ended before the growing call was made: lengthen it"
    b.segment(s1)
    torch.cuda.synchronize()
    check_segment(a.read(), a.model(), "the small call")
    check_segment(b.read(), b.model(), "the growing call")


@pytest.mark.parametrize("mode", MODES)
def test_retransmit_scratch_growth(closing, pair, mode):
    """dk_tcp_retransmit over 8 connections on A, then over 64 on B: the per-connection flags and records grow."""
    import torch

    s0, s1, delay = streams_for(mode, pair)
    sender = TcpSender(0)
    closing(sender)
    a, b = Rtx(sender, 8, seed=2), Rtx(sender, 64, seed=3)
    ready(s0, s1)
    ev = delayed(s0) if delay else None
    a.retransmit(s0)
    assert ev is None or not ev.query(), "the delay on A ended before the growing call was made: lengthen it"
    b.retransmit(s1)
    torch.cuda.synchronize()
    a.check(a.model(), "the small call")
    b.check(b.model(), "the growing call")


@pytest.mark.parametrize("mode", MODES)
def test_commit_scratch_growth(closing, pair, mode):
    """dk_tcp_tx_commit in its chip form over 4 connections on A; then dk_tcp_tx_segment over 64 on B (it grows
    nothing: a first call of that size came before) and its chip-form commit, whose per-connection bases grow."""
    import torch

    s0, s1, delay = streams_for(mode, pair)
    sender = TcpSender(0)
    closing(sender)
    small, large = commit_case(4, lambda c: 2 + c, seed=5), commit_case(64, lambda c: 1 + c % 5, seed=6)
    sizing, a, b = Committed(sender, large, "chip"), Committed(sender, small, "chip"), Committed(sender, large, "chip")
    cur = torch.cuda.current_stream()
    sizing.p.segment(cur)
    a.p.segment(cur)
    torch.cuda.synchronize()
    ready(s0, s1)
    ev = delayed(s0) if delay else None
    a.commit(s0)
    b.p.segment(s1)
    assert ev is None or not ev.query(), "the delay on A ended before the growing call was made: lengthen it"
    b.commit(s1)
    _, ea = a.check("the small call")
    _, eb = b.check("the growing call")
    assert ea["appended"].sum() > 0 and eb["appended"].sum() > 64
