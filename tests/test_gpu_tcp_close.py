"""dk_tcp_close_start / _process / _timers on the MI355X against tests/tcp_close_reference.py (pinned on the CPU by
tests/test_tcp_close_model.py). Every call is compared whole: the output blob and every result array over canary fills,
the closer rows, the receive, send and delayed-ACK tables as bytes, and the batch's arrays unchanged."""
import numpy as np
import pytest

import tcp_close_cases as C
import tcp_close_reference as R
from demikernel_amd import Config, FrameBatch, RxEngine, RxResults, TcpSender, TcpTxResults
from demikernel_amd import _native as N
from demikernel_amd import tcp_close as TCL
from ctl_calls import run

pytestmark = pytest.mark.gpu

CANARY, FILL = 0xA5, 0x5A
FILL32, FILL16 = 0x5A5A5A5A, 0x5A5A
RX_KEYS = ("meta", "flow_id", "tcp_seq", "tcp_ack", "payload")
S1, S2, CL, TW, LA, CD, FT = (TCL.FIN_WAIT_1, TCL.FIN_WAIT_2, TCL.CLOSING, TCL.TIME_WAIT, TCL.LAST_ACK, TCL.CLOSED,
                              TCL.FAULT)


def up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def rx_device(rx: dict) -> RxResults:
    """Host result arrays as the device results of a receive call."""
    import torch

    r = RxResults(len(rx["meta"]), 1, device=torch.device("cuda", 0), tcp_fields=True, counts=False)
    for k in RX_KEYS:
        r.t[k].copy_(torch.from_numpy(np.ascontiguousarray(rx[k], np.uint32).view(np.int32)))
    return r


class Device:
    """The tables of a case on the device, and the model beside them."""

    def __init__(self, t: dict, with_dack: bool = True):
        self.t, self.nconns = t, t["nconns"]
        self.d_rows, self.d_rx, self.d_tx, self.d_links = up(t["rows"]), up(t["rx"]), up(t["tx"]), up(C.LINKS)
        self.d_dack = up(t["dack"]) if with_dack else None
        self.model = R.CloseModel(t["rows"], t["rx"], t["tx"], t["dack"] if with_dack else None)

    def compare_state(self):
        m = self.model
        pairs = [("rows", self.d_rows, m.rows), ("rx_conns", self.d_rx, m.rx), ("tx_conns", self.d_tx, m.tx)]
        if self.d_dack is not None:
            pairs.append(("dack", self.d_dack, m.dack))
        for name, d, h in pairs:
            g = d.cpu().numpy().view(h.dtype)
            if g.tobytes() != h.tobytes():
                bad = [c for c in range(self.nconns) if g[c].tobytes() != h[c].tobytes()]
                raise AssertionError(f"{name} {bad[:6]} differ: got {g[bad[0]]} expected {h[bad[0]]}")

    def process(self, segs, now=C.NOW, **kw):
        return run(self.process_steps(segs, now, **kw))

    def process_steps(self, segs, now=C.NOW, *, slot_stride=64, frame_lead=0, max_frames=None, max_done=None,
                      out_size=None, out_bytes=None, flags=0, action_in=True, stream=None, state=True):
        """process() in the three steps of ctl_calls.Call: the uploads and fills, the call (on `stream`), the wait and
        the comparison. state=False leaves the tables to a later call's comparison. The same for timers and start."""
        import torch

        n = len(segs)
        rx = C.rx_arrays(segs, self.nconns)
        r = rx_device(rx)
        max_frames = 2 * n if max_frames is None else max_frames
        max_done = n if max_done is None else max_done
        size = max(max_frames, 1) * slot_stride + 64 if out_size is None else out_size
        d_out = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda:0")
        res = TCL.CloseResults(n, max_frames, max_done, self.nconns, fill=FILL)
        ain = (np.arange(n) * 7 % 13).astype(np.uint8) if action_in else None
        d_ain = up(ain) if action_in else None
        ob = d_out.numel() if out_bytes is None else out_bytes
        yield
        TCL.close_process(r, self.d_rows, self.d_rx, self.d_tx, self.d_links, now, d_out, res, slot_stride=slot_stride,
                          frame_lead=frame_lead, flags=flags, dack=self.d_dack, action_in=d_ain, out_bytes=ob,
                          max_frames=max_frames, max_done=max_done, stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.process(rx, now, C.LINKS, slot_stride=slot_stride, frame_lead=frame_lead, flags=flags,
                                 max_frames=max_frames, out_bytes=ob, max_done=max_done, action_in=ain)
        got = res.to_numpy()
        after = r.to_numpy()
        for k in ("meta", "flow_id", "tcp_seq", "tcp_ack"):
            assert np.array_equal(after[k], rx[k]), f"the batch's {k} was written"
        if action_in:
            assert np.array_equal(d_ain.cpu().numpy(), ain)
        assert (got["n_frames"], got["n_done"]) == (exp["n_frames"], exp["n_done"])
        assert np.array_equal(got["status"], exp["status"]), (got["status"], exp["status"])
        if exp["fits"]:
            for k in ("action", "state_after", "ack_action", "reply_frame", "fin_frame"):
                if not np.array_equal(got[k], exp[k]):
                    bad = np.nonzero(got[k] != exp[k])[0][:8]
                    raise AssertionError(f"{k} differs at {bad}: got {got[k][bad]} expected {exp[k][bad]}")
        else:  # nothing else is written
            for k in ("action", "state_after", "ack_action"):
                assert (got[k] == FILL).all(), k
            assert (got["reply_frame"] == FILL32).all() and (got["fin_frame"] == FILL32).all()
        w, y = len(exp["frames"]), len(exp["done"])
        assert np.array_equal(got["off_out"][:w], np.arange(w, dtype=np.uint32) * slot_stride + frame_lead)
        assert (got["len_out"][:w] == 54).all()
        assert np.array_equal(got["frame_seg"][:w], np.array(exp["frame_seg"], np.uint32))
        for j in range(y):
            assert got["done"][j].tobytes() == exp["done"][j].tobytes(), (j, got["done"][j], exp["done"][j])
        assert (got["off_out"][w:] == FILL32).all() and (got["len_out"][w:] == FILL16).all()
        assert (got["frame_seg"][w:] == FILL32).all() and (got["done"][y:].view(np.uint8) == FILL).all()
        out = d_out.cpu().numpy()
        want = R.blob_of(exp["frames"], slot_stride, frame_lead, len(out), CANARY)
        if not np.array_equal(out, want):
            bad = np.nonzero(out != want)[0]
            raise AssertionError(f"{len(bad)} output bytes differ, first at {bad[:8]}: got {out[bad[:8]]} "
                                 f"expected {want[bad[:8]]}")
        if state:
            self.compare_state()
        return got, exp

    def timers(self, now, **kw):
        return run(self.timers_steps(now, **kw))

    def timers_steps(self, now, *, max_done=None, with_tx=True, stream=None, state=True):
        import torch

        max_done = self.nconns if max_done is None else max_done
        res = TCL.CloseResults(4, 4, max_done, self.nconns, fill=FILL)
        yield
        TCL.close_timers(self.d_rows, now, res, tx_conns=self.d_tx if with_tx else None, max_done=max_done, stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.timers(now, max_done=max_done, with_tx=with_tx)
        got = res.to_numpy()
        assert got["n_done"] == exp["n_done"] and np.array_equal(got["status"], exp["status"])
        y = len(exp["done"])
        for j in range(y):
            assert got["done"][j].tobytes() == exp["done"][j].tobytes(), (j, got["done"][j], exp["done"][j])
        assert (got["done"][y:].view(np.uint8) == FILL).all()
        for k in ("action", "state_after", "ack_action", "reply_frame", "off_out", "len_out", "frame_seg", "fin_frame"):
            assert (res.raw()[k] == FILL).all(), k
        if state:
            self.compare_state()
        return got, exp

    def start(self, close, **kw):
        return run(self.start_steps(close, **kw))

    def start_steps(self, close, fill=FILL, *, stream=None, state=True):
        import torch

        k = len(close)
        d_close = up(np.asarray(close, np.uint32)) if k else torch.zeros(4, dtype=torch.uint8, device="cuda:0")
        yield
        s = TCL.close_start(self.d_rows, self.d_rx, self.d_tx, d_close, nclose=k, fill=fill, stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.start(close)
        got = s.to_numpy()
        assert got["n_markers"] == exp["n_markers"]
        for f in ("status", "conn", "off", "len"):
            assert np.array_equal(got[f][:k], exp[f]), (f, got[f][:k], exp[f])
            assert (got[f][k:].view(np.uint8) == fill).all(), f"{f} was written past its {k} entries"
        if state:
            self.compare_state()
        return s, exp


# ---- the exhaustive batch -----------------------------------------------------------------------------------------------
def test_exhaustive_sequences():
    """Every sequence of 1 to 4 frames over {none, A, U, F, A+F, U+F} from each live state, 6,216 rows and 23,640 frames
    as one batch, a row's frames never adjacent."""
    t, segs = C.exhaustive()
    got, exp = Device(t).process(segs)
    assert exp["fits"] and exp["n_done"] > 4000 and exp["n_frames"] > 4000
    assert {int(s) for s in exp["state_after"]} == {S1, S2, CL, TW, LA, CD, FT}


# ---- shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", [1, 65, 257])
def test_row_counts(nrows):
    """1, 65 and 257 rows in every state, live and not, with two frames each and other traffic between."""
    states = [(S1, S2, CL, LA, TCL.IDLE, TW, CD, FT)[c % 8] for c in range(nrows)]
    t = C.table(states, seed=nrows)
    scripts = [[C.seg(t, c, C.KINDS[(c // 8 + j) % 6], j) for j in range(2)] for c in range(nrows)]
    got, exp = Device(t).process(C.interleave(scripts, pad_every=5))
    dead = [i for i, s in enumerate(C.interleave(scripts, pad_every=5)) if s is None or states[s[0]] not in C.LIVE]
    assert (exp["action"][dead] == 0).all() and (exp["reply_frame"][dead] == TCL.NONE).all()
    assert np.array_equal(exp["ack_action"][dead], (np.arange(len(exp["action"])) * 7 % 13).astype(np.uint8)[dead])


@pytest.mark.parametrize("m,at", [(1, 0), (2, 1), (3, 0), (70, 63), (70, 64), (70, 69), (300, 0), (300, 255), (300, 256),
                                  (300, 299), (300, None)])
def test_frames_per_row(m, at):
    """A row with 1, 2, 3, 70 and 300 frames (and one with none), the deciding frame first, last and at index 63 / 64 /
    255 / 256 of the row and of the batch; a second row changes state twice around it."""
    t = C.table([S1, S1, S2, LA], seed=m)
    for alone in (True, False):
        d = Device(t)
        main = C.long_row(t, 0, m, at, "AF", "U")
        if alone:  # the row's index is the batch's
            segs = main
        else:
            other = C.long_row(t, 1, m, 0 if m > 1 else None, "F", "none")
            if m > 2:
                other[m // 2] = C.seg(t, 1, "A")  # CLOSING, then TIME_WAIT
            segs = C.interleave([main, other])
        got, exp = d.process(segs)
        assert int(d.model.rows["state"][0]) == (S1 if at is None else TW)
        assert int(d.model.rows["state"][2]) == S2 and exp["fin_frame"][2] == TCL.NONE  # the row with no frame


def test_neighbouring_deciders_and_no_closing_row():
    t = C.table([S1, CL, S2, LA] * 2, seed=4)
    segs = [C.seg(t, 0, "none"), C.seg(t, 1, "U"), C.seg(t, 0, "AF"), C.seg(t, 1, "A"), C.seg(t, 2, "UF"),
            C.seg(t, 3, "A"), C.seg(t, 3, "A"), C.seg(t, 2, "A"), C.seg(t, 5, "F"), C.seg(t, 4, "F"), C.seg(t, 4, "AF")]
    got, exp = Device(t).process(segs)
    assert [int(x) for x in exp["state_after"]] == [S1, CL, TW, TW, TW, CD, CD, TW, FT, CL, FT]
    assert [int(d["row"]) for d in exp["done"]] == [0, 1, 2, 3, 5, 4]
    t = C.table([TCL.IDLE, TW, CD, FT], seed=5)
    d = Device(t)
    got, exp = d.process([C.seg(t, c, "AF") for c in range(4)] * 3 + [None] * 5)
    assert (exp["action"] == 0).all() and exp["n_frames"] == 0 and (exp["status"] == 0).all()
    got, exp = d.process([C.seg(t, 1, "A")], action_in=False)
    assert exp["ack_action"][0] == N.A["SKIP"]


@pytest.mark.parametrize("snd_nxt", [0xFFFFFFFF, 0, 0x7FFFFFFF])
def test_sequence_wrap(snd_nxt):
    """ack - snd_nxt of 0, 1, 2^31 - 1 (unsent), 2^31 and 2^32 - 1 (acceptable), with snd_nxt and RCV.NXT at the wrap."""
    deltas = [0, 1, (1 << 31) - 1, 1 << 31, 0xFFFFFFFF]
    t = C.table([LA] * len(deltas) + [S2] * len(deltas), seed=9, snd_nxt=[snd_nxt] * (2 * len(deltas)),
                rcv_nxt=[0xFFFFFFFF] * (2 * len(deltas)))
    segs = [(c, R.ACK | (R.FIN if c >= len(deltas) else 0), (snd_nxt + deltas[c % len(deltas)]) & R.M32, 5)
            for c in range(2 * len(deltas))]
    got, exp = Device(t).process(segs)
    ok = TCL.POPPED | TCL.ACK_OK
    assert [int(a) for a in exp["action"][:5]] == [ok, TCL.POPPED | TCL.ACK_UNSENT, TCL.POPPED | TCL.ACK_UNSENT, ok, ok]
    assert exp["n_frames"] == 2 + 5 + 2


# ---- row checks, capacity, layout ---------------------------------------------------------------------------------------
def test_row_checks_in_priority_order():
    n = 12
    t = C.table([S1] * n, seed=6)
    rx, tx = t["rx"], t["tx"]
    rx["state"][0] = N.DK_TCP_ESTABLISHED                      # E_RX_STATE
    tx["state"][1] = N.DK_TCP_CLOSED                           # E_STATE
    tx["link"][2] = 2                                          # E_LINK
    tx["rcv_wscale"][3] = 15                                   # E_WSCALE
    rx["buffer_size"][4] = 0x10000                             # E_WINDOW
    rx["state"][6], tx["state"][6], tx["link"][6] = N.DK_TCP_NONE, 0, 9    # E_RX_STATE first
    tx["state"][7], tx["link"][7], tx["rcv_wscale"][7] = 0, 9, 15          # E_STATE
    tx["link"][8], tx["rcv_wscale"][8] = 9, 15                             # E_LINK
    tx["rcv_wscale"][9], rx["buffer_size"][9] = 15, 0xFFFFFFFF             # E_WSCALE
    rx["buffer_size"][10], tx["rcv_wscale"][10] = 0x10000 << 3, 3          # E_WINDOW
    t["rows"]["state"][11] = TCL.IDLE
    rx["state"][11] = N.DK_TCP_ESTABLISHED                                 # not live: no check
    segs = [C.seg(t, c, "AF") for c in range(n)]
    got, exp = Device(t).process(segs)
    assert list(exp["status"]) == [TCL.E_RX_STATE, TCL.E_STATE, TCL.E_LINK, TCL.E_WSCALE, TCL.E_WINDOW, TCL.OK, TCL.E_RX_STATE,
                                   TCL.E_STATE, TCL.E_LINK, TCL.E_WSCALE, TCL.E_WINDOW, TCL.OK]
    assert [int(a) for a in exp["action"]] == [0] * 5 + [TCL.POPPED | TCL.ACK_OK | TCL.FIN] + [0] * 6
    got, exp = Device(t).process(segs, slot_stride=64, frame_lead=11)  # 11 + 54 > 64
    assert list(exp["status"][[4, 5, 11]]) == [TCL.E_WINDOW, TCL.E_SLOT, TCL.OK] and exp["n_frames"] == 0


def test_no_room():
    """By max_frames, by out_bytes and by max_done: nothing is written and the need is reported."""
    t = C.table([S1, S2, LA, CL, TCL.IDLE], seed=7)
    segs = [C.seg(t, 0, "UF"), None, C.seg(t, 1, "F"), C.seg(t, 2, "A"), C.seg(t, 4, "A"), C.seg(t, 0, "none")]
    d = Device(t)
    for kw in (dict(max_frames=2), dict(max_frames=3, out_bytes=191, out_size=400), dict(max_done=1), dict(max_done=0)):
        got, exp = d.process(segs, **kw)
        assert (exp["n_frames"], exp["n_done"], exp["fits"]) == (3, 2, False)
        assert list(exp["status"]) == [TCL.NO_ROOM] * 3 + [TCL.OK] * 2
    got, exp = d.process(segs, max_frames=3, out_bytes=192, out_size=400, max_done=2)
    assert exp["fits"] and [int(x) for x in d.model.rows["state"]] == [CL, TW, CD, CL, TCL.IDLE]


@pytest.mark.parametrize("slot_stride,frame_lead,flags", [(61, 3, 0), (77, 23, 0), (64, 0, N.DK_TX_OFFLOAD_TCP),
                                                          (55, 1, N.DK_TX_OFFLOAD_TCP)])
def test_frame_layout_and_offload(slot_stride, frame_lead, flags):
    """An unaligned frame_lead and an odd slot_stride; the offload flag writes the TCP checksum as 0."""
    t = C.table([S1, S2, LA, S1] * 5, seed=8, rcv_wscale=np.arange(20) % 5)
    scripts = [[C.seg(t, c, ("UF", "U", "F", "AF")[(c + j) % 4], j) for j in range(3)] for c in range(20)]
    got, exp = Device(t).process(C.interleave(scripts), slot_stride=slot_stride, frame_lead=frame_lead, flags=flags)
    assert exp["n_frames"] > 20
    if flags:
        assert all(f[50:52] == b"\0\0" for f in exp["frames"])


def test_without_dack_and_zero_sized_calls():
    import torch

    t = C.table([S1, LA], seed=3)
    d = Device(t, with_dack=False)
    d.process([C.seg(t, 0, "U"), C.seg(t, 1, "U")])
    res = TCL.CloseResults(0, 0, 0, 2, fill=FILL)
    r = rx_device(C.rx_arrays([None], 2))
    d_out = torch.full((64,), CANARY, dtype=torch.uint8, device="cuda:0")
    TCL.close_process(r, d.d_rows, d.d_rx, d.d_tx, d.d_links, 1, d_out, res, slot_stride=64, n=0)
    torch.cuda.synchronize()
    g = res.to_numpy()
    assert (g["n_frames"], g["n_done"]) == (0, 0) and list(g["status"]) == [0, 0] and list(g["fin_frame"]) == [TCL.NONE] * 2
    assert (d_out.cpu().numpy() == CANARY).all()
    d.compare_state()
    e = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    res = TCL.CloseResults(0, 0, 0, 0, fill=FILL)
    TCL.close_process(r, e[:0], e[:0], e[:0], d.d_links, 1, d_out, res, slot_stride=64, n=0)
    TCL.close_timers(e[:0], 5, res)
    s = TCL.close_start(e[:0], e[:0], e[:0], e[:0], fill=FILL)
    torch.cuda.synchronize()
    assert res.to_numpy()["n_done"] == 0 and s.to_numpy()["n_markers"] == 0


# ---- dk_tcp_close_start -------------------------------------------------------------------------------------------------
def start_table(n, seed=2):
    t = C.table([TCL.IDLE] * n, seed=seed)
    c = np.arange(n)
    t["rows"]["state"] = np.where(c % 11 == 5, S2, TCL.IDLE)
    t["rx"]["state"] = np.where(c % 7 == 3, N.DK_TCP_NONE, np.where(c % 3 == 1, N.DK_TCP_CLOSED, N.DK_TCP_ESTABLISHED))
    t["tx"]["state"] = np.where(c % 13 == 6, N.DK_TCP_CLOSED, N.DK_TCP_ESTABLISHED)
    return t


@pytest.mark.parametrize("nclose", [1, 65, 257, 700])
def test_close_start_statuses_and_markers(nclose):
    """E_ROW, E_ORDER (duplicates and descents), E_STATE and E_BADF among accepted entries; the padded marker list."""
    n = 2 * nclose
    d = Device(start_table(n))
    close = list(range(0, n, 2))
    if nclose > 4:
        close[3] = close[2]               # a duplicate
        close[nclose // 2] = 1            # a descent
        close[nclose - 1] = n + 5         # beyond the table
    s, exp = d.start(close)
    if nclose > 4:
        assert {TCL.OK, TCL.E_ROW, TCL.E_ORDER, TCL.E_BADF} <= {int(x) for x in exp["status"]}
    if nclose >= 65:
        assert TCL.E_STATE in exp["status"]
    assert 0 < exp["n_markers"] <= nclose


def test_markers_feed_tx_segment():
    """The padded marker list goes straight to dk_tcp_tx_segment: exactly the accepted rows get an ACK|FIN frame, and
    the call is tests/tx_segment_reference.py's over the model's list, byte for byte."""
    import torch

    import tx_segment_reference as M

    n, stride = 40, 1536
    t = start_table(n, seed=12)
    t["tx"]["snd_una"] = t["tx"]["snd_nxt"]
    d = Device(t)
    close = list(range(1, n, 2)) + [n + 1]
    s, exp = d.start(close)
    k = len(close)
    want = M.segment(np.zeros(16, np.uint8), exp["conn"], exp["off"], exp["len"], d.model.tx, C.LINKS,
                     np.full(k * stride, CANARY, np.uint8), slot_stride=stride, frame_lead=0, max_frames=k,
                     rx_conns=d.model.rx)
    sender = TcpSender(0)
    try:
        res = TcpTxResults(k, k)
        out = torch.full((k * stride,), CANARY, dtype=torch.uint8, device="cuda:0")
        src = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
        sender.segment(src, s.markers, d.d_tx, d.d_links, out, res, slot_stride=stride, rx_conns=d.d_rx)
        torch.cuda.synchronize()
        g = res.to_numpy()
    finally:
        sender.close()
    m = exp["n_markers"]
    assert m == 14 and g["n_frames"] == want["n_frames"] == m
    assert np.array_equal(g["status"], want["status"])
    assert list(g["status"]) == [N.DK_TCP_TX_SENT] * m + [N.DK_TCP_TX_E_CONN] * (k - m)
    blob = out.cpu().numpy()
    assert np.array_equal(blob, want["out"])
    tx = d.d_tx.cpu().numpy().view(N.TX_CONN_DTYPE)
    assert tx.tobytes() == want["tx_conns"].tobytes()
    for f, c in enumerate(exp["conn"][:m]):
        fr = blob[f * stride: f * stride + 54]
        assert fr[47] == (R.ACK | R.FIN) and int.from_bytes(fr[38:42].tobytes(), "big") == int(t["tx"]["snd_nxt"][c])
        assert tx["fin_sent"][c] == 1 and tx["snd_nxt"][c] == (int(t["tx"]["snd_nxt"][c]) + 1) & R.M32
    assert int(tx["fin_sent"].sum()) == m


# ---- dk_tcp_close_timers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", [7, 300, 1100])
def test_close_timers(nrows):
    """A deadline at now, now - 1 and now + 1; CLOSED rows retired exactly once; the tx_conns write; the capacity rule."""
    now = 1 << 41
    c = np.arange(nrows)
    t = C.table([(TW, TW, TW, CD, S1, TCL.IDLE, FT)[k % 7] for k in range(nrows)], seed=nrows)
    t["rows"]["deadline_ns"] = np.where(c % 7 == 0, now, np.where(c % 7 == 1, now - 1, now + 1))
    t["rows"]["flags"] = np.where(c % 21 == 3, TCL.RETIRED, 0)
    d = Device(t)
    need = d.model.timers(now, max_done=0)["n_done"]
    d.model = R.CloseModel(t["rows"], t["rx"], t["tx"], t["dack"])
    got, exp = d.timers(now, max_done=need - 1)
    assert not exp["fits"] and (exp["status"] == TCL.NO_ROOM).sum() == need
    got, exp = d.timers(now, max_done=need, with_tx=False)
    assert exp["fits"] and exp["n_done"] == need == len([k for k in range(nrows) if k % 7 in (0, 1) or (k % 7 == 3 and k % 21 != 3)])
    got, exp = d.timers(now, with_tx=True)
    assert exp["n_done"] == 0
    got, exp = d.timers(now + 1)
    assert exp["n_done"] == len([k for k in range(nrows) if k % 7 == 2])
    assert (d.model.tx["state"][c % 7 == 2] == N.DK_TCP_CLOSED).all() and (d.model.tx["state"][c % 7 == 0] != N.DK_TCP_CLOSED).all()


# ---- through the receive engine -----------------------------------------------------------------------------------------
def test_real_frames_through_the_receive_engine():
    """The same segments as frames (tests/frames.py) through dk_rx_process: its results drive dk_tcp_close_process
    exactly as the uploaded arrays do."""
    import torch

    import frames as F
    from demikernel_amd import synth

    t = C.table([S1, S2, CL, LA, TCL.IDLE, S1], seed=21)
    scripts = [[C.seg(t, c, k, j) for j, k in enumerate(ks)]
               for c, ks in enumerate((("U", "AF", "A"), ("UF", "A"), ("none", "A"), ("F", "U", "A"), ("AF",), ("F", "A")))]
    segs = C.interleave(scripts)
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    try:
        eng.set_sockets(t["flows"])
        blob, off, lens = F.pack([C.frame_of(t, s) for s in segs])
        rx = eng.results(len(segs), tcp_fields=True)
        eng.receive_batch(FrameBatch.from_numpy(blob, off, lens), rx)
        torch.cuda.synchronize()
        h = rx.to_numpy()
        want = C.rx_arrays(segs, t["nconns"])
        for k in ("flow_id", "tcp_seq", "tcp_ack"):
            assert np.array_equal(h[k], want[k]), k
        assert np.array_equal(h["meta"] & 0x00FF00FF, want["meta"] & 0x00FF00FF)
        d = Device(t)
        res = TCL.CloseResults(len(segs), 2 * len(segs), len(segs), t["nconns"], fill=FILL)
        d_out = torch.full((2 * len(segs) * 64,), CANARY, dtype=torch.uint8, device="cuda:0")
        TCL.close_process(rx, d.d_rows, d.d_rx, d.d_tx, d.d_links, C.NOW, d_out, res, slot_stride=64, dack=d.d_dack)
        torch.cuda.synchronize()
    finally:
        eng.close()
    exp = d.model.process(want, C.NOW, C.LINKS, slot_stride=64, max_frames=2 * len(segs), out_bytes=d_out.numel(),
                          max_done=len(segs))
    got = res.to_numpy()
    for k in ("action", "state_after", "ack_action", "reply_frame", "fin_frame", "status"):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(d_out.cpu().numpy(), R.blob_of(exp["frames"], 64, 0, d_out.numel(), CANARY))
    d.compare_state()
