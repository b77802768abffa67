"""dk_tcp_ack_emit on the MI355X against tests/tcp_ackemit_reference.py (pinned on the CPU by
tests/test_tcp_ackemit_model.py). The batches of tests/tcp_ackemit_cases.py go through dk_tcp_rx_process first, so the
actions, the views and the order by connection are the engine's own; the restatement runs its own process_packet loop
from the table as it was before. Every call is compared whole: the output blob over a canary fill (nothing outside the
frames is written), every result array over a canary fill (everything the contract says is written must be), the dack
table as bytes, and the receive table, the TX table and the batch unchanged. Every case runs in both forms
(dk_diag_tcp_ack_emit_set_form)."""
import errno
import functools

import numpy as np
import pytest

import tcp_ackemit_cases as C
import tcp_ackemit_reference as E
import tx_segment_reference as M
from ctl_calls import delayed, stream_pair
from demikernel_amd import _native as N
from demikernel_amd.rx import Fail
from demikernel_amd.tcp import TcpOut, TcpReceiver
from demikernel_amd.tcp_ack import TcpAcker, TcpAckOut, UnackedQueue, ack_conn_table
from demikernel_amd.tcp_ackemit import AckEmitResults, ack_emit, ack_emit_batch, dack_to_device, dack_to_host, last_form
from test_gpu_tcp import rx_device

pytestmark = pytest.mark.gpu

CANARY, FILL = 0xA5, 0x5A5A5A5A
FORMS = ["lane", "scan"]
LINKS = M.links_table()
NOW = 123456789012
RESULT_KEYS = ("status", "n_acks", "ack_frame", "off_out", "len_out", "frame_conn", "frame_seg")


class Device:
    """One case on the device up to and including dk_tcp_rx_process; emit() runs the ACK pass."""

    def __init__(self, case: dict, radix: bool = False, walk=None):
        import torch

        self.case, self.n, self.nrows = case, case["n"], case["nconns"]
        dev = torch.device("cuda", 0)
        self.up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
        self.tcp = TcpReceiver(0, radix_sort=radix, walk=walk)
        self.r = rx_device(case["rx"])
        self.d_rx = self.tcp.conns_to_device(case["table"])
        self.d_tx, self.d_dack, self.d_links = self.up(case["tx"]), dack_to_device(case["dack"]), self.up(LINKS)
        self.out = TcpOut(self.n, self.nrows)

    def receive(self):
        self.tcp.process(self.r, self.d_rx, self.out)

    def emit(self, form, *, slot_stride=64, frame_lead=0, max_frames=None, out_size=None, **kw):
        import torch

        max_frames = self.n if max_frames is None else max_frames
        out_size = max(max_frames, 1) * slot_stride + 64 if out_size is None else out_size
        self.d_out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=self.d_rx.device)
        self.res = AckEmitResults(max_frames, self.nrows, self.n, fill=FILL)
        ack_emit(self.tcp, self.r, self.out, self.d_rx, self.d_tx, self.d_dack, self.d_links, NOW, self.d_out, self.res,
                 slot_stride=slot_stride, frame_lead=frame_lead, max_frames=max_frames, form=form, **kw)

    def read(self) -> dict:
        import torch

        torch.cuda.synchronize()
        got = self.res.to_numpy()
        w = got["frames_written"]  # entries of the per-frame arrays past the frames written are untouched
        for k in ("off_out", "frame_conn", "frame_seg"):
            assert (getattr(self.res, k).cpu().numpy().view(np.uint32)[w:] == FILL).all(), k
        assert (self.res.len_out.cpu().numpy().view(np.uint16)[w:] == FILL & 0xFFFF).all()
        got.update(out=self.d_out.cpu().numpy(), dack=dack_to_host(self.d_dack),
                   rx_conns=self.tcp.conns_to_host(self.d_rx), tx=self.d_tx.cpu().numpy(),
                   action=self.out.to_numpy()["action"], view=self.out.to_numpy()["view"],
                   rx={k: self.r.t[k].cpu().numpy().view(np.uint32) for k in self.case["rx"]})
        return got

    def close(self):
        self.tcp.close()


def reference(case, *, slot_stride=64, frame_lead=0, max_frames=None, out_size=None, flags=0, out_bytes=None, **_):
    max_frames = case["n"] if max_frames is None else max_frames
    out_size = max(max_frames, 1) * slot_stride + 64 if out_size is None else out_size
    return E.ack_emit(case["rx"], case["table"], case["tx"], case["dack"], LINKS, NOW, np.full(out_size, CANARY, np.uint8),
                      slot_stride=slot_stride, frame_lead=frame_lead, max_frames=max_frames, flags=flags,
                      out_bytes=out_bytes)


def compare(got: dict, exp: dict, case: dict, ctx: str):
    assert np.array_equal(got["action"], exp["action"]), f"{ctx}: the engine's actions are not the restatement's"
    assert got["n_frames"] == exp["n_frames"], (ctx, got["n_frames"], exp["n_frames"])
    for k in RESULT_KEYS:
        g, e = got[k], exp[k]
        assert len(g) == len(e), (ctx, k, len(g), len(e))
        if not np.array_equal(g, e):
            bad = np.nonzero(g != e)[0][:8]
            raise AssertionError(f"{ctx}: {k} differs at {bad}: got {g[bad]} expected {e[bad]}")
    g, e = got["dack"], exp["dack"]
    assert g.tobytes() == e.tobytes(), (ctx, [(c, g[c], e[c]) for c in range(len(e)) if g[c].tobytes() != e[c].tobytes()][:4])
    if not np.array_equal(got["out"], exp["out"]):
        bad = np.nonzero(got["out"] != exp["out"])[0]
        raise AssertionError(f"{ctx}: {len(bad)} output bytes differ, first at {bad[:8]}: got {got['out'][bad[:8]]} "
                             f"expected {exp['out'][bad[:8]]}")
    assert got["rx_conns"].tobytes() == exp["rx_conns"].tobytes(), f"{ctx}: the receive table"
    assert got["tx"].tobytes() == np.ascontiguousarray(case["tx"]).tobytes(), f"{ctx}: the TX table was written"
    for k, v in case["rx"].items():
        assert np.array_equal(got["rx"][k], v), f"{ctx}: the batch's {k} was written"


def run(case: dict, form, radix=False, walk=None, expect_form=None, **kw) -> tuple:
    d = Device(case, radix, walk)
    try:
        d.receive()
        d.emit(form, **kw)
        got = d.read()
        ran, rxwalk, sort = last_form(d.tcp), d.tcp.last_walk, d.tcp.last_sort
    finally:
        d.close()
    exp = reference(case, **kw)
    compare(got, exp, case, f"{ran} form after the {rxwalk} walk, {sort} sort")
    if case["n"] and case["nconns"]:
        assert ran == (expect_form or form), (ran, form)
    return got, exp


def hist(exp) -> dict:
    return {N.TCP_ACTIONS[a]: int(k) for a, k in enumerate(np.bincount(exp["action"], minlength=13)) if k}


# ---------------------------------------------------------------------------------------------------------------------
# 1. connections x segments per connection: the receive walk's form changes at 8 and 1,024 segments per table row, the
#    sort at 255 rows, and whichever ran leaves the order behind; 257 rows are above the scan walk's 256
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = ([(1, m) for m in (1, 7, 8, 9, 64, 65, 1025)] +
          [(nc, m) for nc in (63, 64, 65, 257) for m in (1, 7, 8, 9, 64, 65)] +
          [(nc, 1025) for nc in (63, 64, 65, 257)])


@functools.lru_cache(maxsize=4)
def case_uniform(nc: int, m: int):
    # rows = nc + 1: a batch of m * (nc + 1) segments or more reaches the walk's next form
    return C.uniform(nc, m, skip_every=0 if m in (8, 1025) else 9, total=(nc + 1) * m if m in (8, 1025) else None)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nc,m", SHAPES)
def test_connections_and_segments(nc, m, form):
    got, exp = run(case_uniform(nc, m), form)
    assert (exp["status"][:nc] == E.OK).all() and exp["status"][nc] == E.E_STATE
    if m >= 64:
        assert exp["n_frames"] > 0


def test_every_action_in_one_batch():
    case = case_uniform(65, 65)
    _, exp = run(case, None, expect_form="scan")
    assert len(hist(exp)) == 13, hist(exp)
    # strays the key kernel classified early, between walked segments of their connection: their ACKs carry the
    # RCV.NXT of their arrival, not the table's
    act, f = exp["action"], case["rx"]["flow_id"]
    mid = [(i, c, a) for i, c, a, w in exp["desc"] if act[i] in (N.A["DUPLICATE"], N.A["OUT_OF_WINDOW"])
           and a != int(exp["rx_conns"]["receive_next"][c]) and a != int(case["table"]["receive_next"][c])]
    assert len(mid) > 50, len(mid)
    assert any(act[i] in (N.A["DUPLICATE"], N.A["OUT_OF_WINDOW"]) and (case["rx"]["meta"][i] >> 16) & 4
               and exp["ack_frame"][i] == E.NO_FRAME for i in range(case["n"]))
    assert (case["dack"]["armed"][:65] == 0).any() and (case["dack"]["armed"][:65] == 1).any()


def test_engine_rule_picks_the_form():
    run(case_uniform(63, 7), None, expect_form="lane")   # 441 segments and the frames between over 64 rows
    few = C.uniform(63, 7, skip_every=0)
    assert few["n"] < 8 * few["nconns"]
    run(few, None, expect_form="lane")
    many = case_uniform(63, 8)
    assert many["n"] == 8 * many["nconns"]
    run(many, None, expect_form="scan")


# ---------------------------------------------------------------------------------------------------------------------
# 2. batch sizes around the frame-numbering scan's tile of 1,024 items, under every receive walk
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def case_total(total: int):
    return C.build([C.Script(m=total // 5), C.Script(m=total // 4, close="fin"), C.Script(m=total // 3, mix=C.PLAIN),
                    C.Script(m=7)], seed=total, skip_every=11, total=total)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("total", [1024, 1025, 2049])
def test_batch_sizes(total, form):
    got, exp = run(case_total(total), form)
    assert exp["n_frames"] > 200


@pytest.mark.parametrize("walk", ["lane", "wave", "relay", "scan"])
def test_after_every_receive_walk(walk):
    for form in FORMS:
        run(case_total(2049), form, walk=walk)
    run(case_total(2049), "scan", walk=walk, radix=True)


# ---------------------------------------------------------------------------------------------------------------------
# 3. sequence space and windows
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_wrap():
    top = 1 << 32
    return C.build([C.Script(m=200, rn=top - 100), C.Script(m=70, rn=top - 1, mix=C.PLAIN, armed=1),
                    C.Script(m=70, rn=top - 8, close="fin"), C.Script(m=9, rn=0)], seed=31)


@pytest.mark.parametrize("form", FORMS)
def test_rcv_nxt_wraps_inside_the_batch(form):
    got, exp = run(case_wrap(), form)
    acks = np.array([a for i, c, a, w in exp["desc"] if c < 3], np.int64)
    assert (acks > 1 << 31).any() and (acks < 1 << 20).any()
    assert (exp["rx_conns"]["receive_next"][:3] < 1 << 20).all()


@functools.lru_cache(maxsize=None)
def case_windows():
    # 20,000 bytes of buffer filled by segments of up to 1,400 bytes: the window closes to 0 mid-batch and the ACKs
    # behind say so; the same at a scale of 14 with 2^29 bytes (never closed), and with unread bytes at the start
    return C.build([C.Script(m=80, mix=C.PLAIN, bufsz=20000, big=True, armed=1),
                    C.Script(m=80, mix=(0.6, 0.4) + (0.0,) * 10, bufsz=20000, big=True, unread=7000),
                    C.Script(m=80, mix=C.PLAIN, bufsz=1 << 29, wscale=14, big=True),
                    C.Script(m=80, bufsz=0xFFFF << 14, wscale=14, unread=1 << 20),
                    C.Script(m=80, bufsz=0xFFFF, wscale=0, unread=65000)], seed=41)


@pytest.mark.parametrize("form", FORMS)
def test_windows_and_scales(form):
    got, exp = run(case_windows(), form)
    tx = case_windows()["tx"]
    win = {c: [w >> int(tx["rcv_wscale"][c]) for i, cc, a, w in exp["desc"] if cc == c] for c in range(5)}
    assert win[0][0] > 15000 and win[0][-1] == 0 and 0 in win[1], (win[0], win[1])  # closes to 0 mid-batch
    assert max(win[2]) == ((1 << 29) >> 14) - 1 and min(win[2]) < max(win[2])  # the first bytes cost a whole unit
    assert all(w <= 0xFFFF for c in win for w in win[c]) and max(win[3]) > 0xFF00
    # the windows as the frames carry them
    a = got["off_out"].astype(np.int64)
    on_wire = got["out"][a + 48].astype(int) << 8 | got["out"][a + 49]
    assert np.array_equal(on_wire, [w >> int(tx["rcv_wscale"][c]) for i, c, a_, w in exp["desc"]])


# ---------------------------------------------------------------------------------------------------------------------
# 4. connection-level failures
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_failures():
    case = C.build([C.Script(m=40) for _ in range(12)], seed=51)
    tx, t = case["tx"], case["table"]
    tx["state"][1] = N.DK_TCP_CLOSED
    tx["snd_nxt"][3] += 1
    tx["link"][5] = len(LINKS)
    tx["rcv_wscale"][7] = 15
    t["buffer_size"][9] = 0x10000            # full open: 17 bits at scale 0
    tx["state"][10], tx["link"][10] = N.DK_TCP_NONE, 99  # E_STATE comes first
    tx["link"][11], tx["rcv_wscale"][11] = 2, 31          # E_LINK before E_WSCALE
    return case


@pytest.mark.parametrize("form", FORMS)
def test_connection_failures(form):
    case = case_failures()
    got, exp = run(case, form)
    want = [E.OK, E.E_STATE, E.OK, E.E_SND_NXT, E.OK, E.E_LINK, E.OK, E.E_WSCALE, E.OK, E.E_WINDOW, E.E_STATE, E.E_LINK,
            E.E_STATE]
    assert exp["status"].tolist() == want
    bad = np.array(want) != E.OK
    assert (exp["n_acks"][bad] == 0).all() and (exp["n_acks"][~bad] > 0).all()
    assert got["dack"][bad].tobytes() == case["dack"][bad].tobytes() and not np.isin(got["frame_conn"], np.nonzero(bad)[0]).any()
    # a slot that does not hold 54 bytes behind its lead fails every connection: nothing at all is written
    got, exp = run(case, form, slot_stride=60, frame_lead=7)
    assert (exp["status"][~bad] == E.E_SLOT).all() and exp["n_frames"] == 0 and (got["out"] == CANARY).all()
    assert got["dack"].tobytes() == case["dack"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 5. capacity, layout, offload
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_capacity_is_all_or_nothing(form):
    case = case_total(1025)
    need = reference(case)["n_frames"]
    ok, _ = run(case, form, max_frames=need, out_size=need * 64 + 64, out_bytes=need * 64)
    assert ok["frames_written"] == need
    for kw in (dict(max_frames=need - 1), dict(max_frames=0), dict(max_frames=need, out_bytes=need * 64 - 1)):
        got, exp = run(case, form, out_size=need * 64 + 64, **kw)
        assert got["n_frames"] == need and got["frames_written"] == 0 and (got["ack_frame"] == E.NO_FRAME).all()
        assert (got["out"] == CANARY).all() and got["dack"].tobytes() == case["dack"].tobytes()
        assert np.array_equal(got["status"] == E.NO_ROOM, ok["n_acks"] > 0) and np.array_equal(got["n_acks"], ok["n_acks"])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("stride,lead", [(54, 0), (55, 1), (61, 7), (77, 2), (131, 3), (64, 10)])
def test_unaligned_slots(stride, lead, form):
    run(case_total(1024), form, slot_stride=stride, frame_lead=lead)


@pytest.mark.parametrize("form", FORMS)
def test_checksum_offload(form):
    got, _ = run(case_total(1024), form, flags=N.DK_TX_OFFLOAD_TCP)
    a = got["off_out"].astype(np.int64)
    assert not got["out"][a + 50].any() and not got["out"][a + 51].any() and got["out"][a + 24].any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. empty calls, the turn rule, both orders with dk_tcp_ack_process
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_empty_batches(form):
    case = C.build([C.Script(m=0), C.Script(m=0)], seed=3, skip_every=0)
    assert case["n"] == 0
    got, exp = run(case, form)
    assert got["n_frames"] == 0 and got["status"].tolist() == [E.OK, E.OK, E.E_STATE] and (got["out"] == CANARY).all()
    none = C.build([C.Script(m=0)], seed=4, skip_every=0, total=70)  # frames, none of a connection
    got, exp = run(none, form)
    assert got["n_frames"] == 0 and (got["ack_frame"] == E.NO_FRAME).all()


def acker_tables(case):
    nrows = case["nconns"]
    ak = ack_conn_table(nrows, wl1=case["table"]["receive_next"], wl2=case["tx"]["snd_nxt"])
    return TcpAcker.conns_to_device(ak), UnackedQueue(nrows, 1), TcpAckOut(case["n"], nrows, fill=7)


@pytest.mark.parametrize("first", ["emit", "ack_process"])
def test_either_order_with_ack_process(first):
    """dk_tcp_ack_emit and dk_tcp_ack_process on one dk_tcp_rx_process call, in either order: the same ACK frames and
    the same dk_tcp_ack_out (SND.UNA = SND.NXT here: every ack is a duplicate or old, no queue is touched)."""
    case = case_total(2049)
    outs = {}
    for order in ("emit", "ack_process"):
        d = Device(case)
        try:
            d.receive()
            d_ak, q, aout = acker_tables(case)
            steps = [lambda: d.emit(None), lambda: TcpAcker().process(d.tcp, d.r, d.out, d.d_rx, d.d_tx, d_ak, q, NOW, aout)]
            for s in (steps if order == "emit" else steps[::-1]):
                s()
            got = d.read()
            outs[order] = (got, aout.to_numpy())
        finally:
            d.close()
    compare(outs[first][0], reference(case), case, f"{first} first")
    a, b = outs["emit"][1], outs["ack_process"][1]
    assert all(np.array_equal(a[k], b[k]) for k in a) and (a["status"][:4] == 0).all() and a["dup_acks"].sum() > 0


def test_call_order():
    """Out of turn (before any dk_tcp_rx_process, twice after one, with another n or nconns, a misaligned table) the
    call is EINVAL and writes nothing; in turn it then still works, and a second dk_tcp_ack_process is still refused."""
    case = case_total(1025)
    d = Device(case)
    try:
        full = (d.d_dack, d.d_tx, d.d_rx)

        def refused(dack=case["dack"], **kw):
            with pytest.raises(Fail) as e:
                d.emit("scan", **kw)
            assert e.value.errno == errno.EINVAL
            d.d_dack, d.d_tx, d.d_rx = full
            now = d.read()
            for k in ("status", "n_acks", "ack_frame"):
                assert (now[k] == FILL).all(), k
            assert now["n_frames"] == FILL and (now["out"] == CANARY).all()
            assert now["dack"].tobytes() == dack.tobytes()

        refused()  # no dk_tcp_rx_process yet
        d.receive()
        refused(n=case["n"] - 1)  # another n
        d.d_dack, d.d_tx, d.d_rx = d.d_dack[:-32], d.d_tx[:-64], d.d_rx[:-288]
        refused()  # another nconns
        d.d_dack = d.d_dack.new_zeros(d.d_dack.numel() + 8)[8:]
        refused()  # a misaligned table
        d.emit("scan")  # in turn
        exp = reference(case)
        compare(d.read(), exp, case, "in turn")
        out1, res1 = d.d_out, d.res
        refused(exp["dack"])  # a second time on the same dk_tcp_rx_process call: the rows stay as the first left them
        d.d_out, d.res = out1, res1
        compare(d.read(), exp, case, "after the refused second call")
        d_ak, q, aout = acker_tables(case)
        TcpAcker().process(d.tcp, d.r, d.out, d.d_rx, d.d_tx, d_ak, q, NOW, aout)  # its own turn is still there
        with pytest.raises(Fail):
            TcpAcker().process(d.tcp, d.r, d.out, d.d_rx, d.d_tx, d_ak, q, NOW, aout)
    finally:
        d.close()


def test_other_stream_and_batch_helper():
    """On another stream than its dk_tcp_rx_process the call waits for it on the device: the receive call sits behind
    100 ms of sleep on its stream and is still pending when the ACKs are queued on the other (ack_emit_batch then waits
    for its stream, so the pending delay is asserted just before it). ack_emit_batch hands the frames on as a
    FrameBatch."""
    import torch

    case = case_total(2049)
    d = Device(case)
    try:
        d.receive()
        # sizes the call's scratch, so that the call below has nothing to wait for on the host; unchecked. The receive
        # and the dack tables it moved are uploaded anew below; d_tx is relied on to be unchanged (the call only reads it)
        d.emit(None)
        torch.cuda.synchronize()
        d.d_rx, d.d_dack = d.tcp.conns_to_device(case["table"]), dack_to_device(case["dack"])
        d.d_out = torch.full((case["n"] * 64,), CANARY, dtype=torch.uint8, device=d.d_rx.device)
        d.res = AckEmitResults(case["n"], d.nrows, d.n, fill=FILL)
        A, s, _ = stream_pair()
        for x in (A, s):
            x.wait_stream(torch.cuda.current_stream())  # the uploads and the fills; the context's own event orders the rest
        ev = delayed(A)
        d.tcp.process(d.r, d.d_rx, d.out, stream=A)
        assert not ev.query(), "the delay ended before the ACKs were queued"
        batch = ack_emit_batch(d.tcp, d.r, d.out, d.d_rx, d.d_tx, d.d_dack, d.d_links, NOW, d.d_out, d.res,
                               slot_stride=64, stream=s)
        exp = reference(case, out_size=case["n"] * 64)
        compare(d.read(), exp, case, "second stream")
        assert batch.n == exp["n_frames"]
    finally:
        d.close()
