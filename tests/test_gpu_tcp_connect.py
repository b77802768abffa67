"""dk_tcp_connect_start / _process / _timers on the MI355X against tests/tcp_connect_reference.py (pinned on the CPU by
tests/test_tcp_connect_model.py). The frames go through the receive engine first, so the per-frame arrays are the
engine's own. Every call is compared whole: the output blob and every result array over canary fills, the connector
rows and the ISN generator as bytes, and the batch's arrays unchanged."""
import errno

import numpy as np
import pytest

import frames as F
import tcp_connect_cases as C
import tcp_connect_reference as R
from demikernel_amd import Config, FrameBatch, RxEngine
from demikernel_amd import _native as N
from demikernel_amd import tcp_connect as TC
from ctl_calls import run

pytestmark = pytest.mark.gpu

CANARY, FILL = 0xA5, 0x5A
FILL32, FILL16 = 0x5A5A5A5A, 0x5A5A
RX_KEYS = ("meta", "src_ip", "ports", "payload", "flow_id", "tcp_seq", "tcp_ack", "tcp_win", "tcp_opts")
TIMEOUT = 3_000_000_000


class Device:
    """A client on the device: the receive engine, the connector rows, the ISN generator; and the model beside it."""

    def __init__(self, flows, rows, cmap, nonce=0, counter=0, local=C.BOB):
        self.eng = RxEngine(Config(local), device=0)
        self.eng.set_sockets(flows)
        self.d_rows, self.d_map, self.d_links = TC.to_device(rows), TC.to_device(cmap), TC.to_device(C.LINKS)
        self.d_gen = TC.to_device(TC.isn_gen(nonce, counter))
        self.cmap, self.nrows = cmap, len(rows)
        self.model = R.ConnectModel(rows, nonce, counter)

    def close(self):
        self.eng.close()

    def receive(self, frames):
        """The frames through the receive engine: its results with the TCP fields and option records."""
        blob, off, lens = F.pack(frames)
        rx = self.eng.results(len(frames), tcp_fields=True, tcp_opts=True)
        self.eng.receive_batch(FrameBatch.from_numpy(blob, off, lens), rx)
        return rx

    def patch(self, fields: dict):
        """The host writes row fields between calls: {row: {field: value}}."""
        rows = TC.rows_to_host(self.d_rows)
        for r, kv in fields.items():
            for k, v in kv.items():
                rows[r][k] = v
                self.model.rows[r][k] = v
        self.d_rows.copy_(TC.to_device(rows))

    def _out(self, max_frames, slot_stride, out_size):
        import torch

        size = max(max_frames, 1) * slot_stride + 64 if out_size is None else out_size
        return torch.full((size,), CANARY, dtype=torch.uint8, device="cuda:0")

    def _compare(self, got, exp, slot_stride, frame_lead, per_frame: bool, state: bool = True):
        assert (got["n_frames"], got["n_ready"]) == (exp["n_frames"], exp["n_ready"])
        assert np.array_equal(got["status"], exp["status"]), (got["status"], exp["status"])
        if per_frame and exp["fits"]:
            for k in ("action", "row", "reply_frame"):
                if not np.array_equal(got[k], exp[k]):
                    bad = np.nonzero(got[k] != exp[k])[0][:8]
                    raise AssertionError(f"{k} differs at {bad}: got {got[k][bad]} expected {exp[k][bad]}")
        else:  # nothing is written
            assert (got["action"] == FILL).all() and (got["row"] == FILL32).all() and (got["reply_frame"] == FILL32).all()
        w, y = (exp["n_frames"], exp["n_ready"]) if exp["fits"] else (0, 0)
        assert np.array_equal(got["off_out"][:w], np.arange(w, dtype=np.uint32) * slot_stride + frame_lead)
        assert np.array_equal(got["len_out"][:w], np.array([len(f) for f in exp["frames"]], np.uint16))
        assert np.array_equal(got["frame_seg"][:w], np.array(exp["frame_seg"], np.uint32))
        for j in range(y):
            assert got["ready"][j].tobytes() == exp["ready"][j].tobytes(), (j, got["ready"][j], exp["ready"][j])
        assert (got["off_out"][w:] == FILL32).all() and (got["len_out"][w:] == FILL16).all()
        assert (got["frame_seg"][w:] == FILL32).all() and (got["ready"][y:].view(np.uint8) == FILL).all()
        want = R.blob_of(exp["frames"], slot_stride, frame_lead, len(got["out"]), CANARY)
        if not np.array_equal(got["out"], want):
            bad = np.nonzero(got["out"] != want)[0]
            raise AssertionError(f"{len(bad)} output bytes differ, first at {bad[:8]}: got {got['out'][bad[:8]]} "
                                 f"expected {want[bad[:8]]}")
        if state:
            self.compare_state()

    def compare_state(self):
        g = TC.rows_to_host(self.d_rows)
        if g.tobytes() != self.model.rows.tobytes():
            bad = [r for r in range(self.nrows) if g[r].tobytes() != self.model.rows[r].tobytes()]
            raise AssertionError(f"rows {bad[:6]} differ: got {g[bad[0]]} expected {self.model.rows[bad[0]]}")
        gen = TC.isn_gen_to_host(self.d_gen)[0]
        assert (int(gen["nonce"]), int(gen["counter"]), int(gen["reserved"])) == (self.model.nonce, self.model.counter, 0)

    def start(self, start, now=C.NOW - 10, **kw):
        return run(self.start_steps(start, now, **kw))

    def start_steps(self, start, now=C.NOW - 10, *, slot_stride=64, frame_lead=0, max_frames=None, max_ready=None,
                    out_size=None, out_bytes=None, flags=0, stream=None, state=True):
        """start() in the three steps of ctl_calls.Call: the uploads and fills, the call (on `stream`), the wait and
        the comparison. state=False leaves the rows to a later call's comparison. The same for process and timers."""
        import torch

        ns = len(start)
        max_frames = ns if max_frames is None else max_frames
        max_ready = ns if max_ready is None else max_ready
        d_out = self._out(max_frames, slot_stride, out_size)
        res = TC.ConnectResults(4, max_frames, max_ready, ns, fill=FILL)
        d_start = TC.to_device(np.asarray(start, np.uint32)) if ns else torch.zeros(4, dtype=torch.uint8, device="cuda:0")
        ob = d_out.numel() if out_bytes is None else out_bytes
        yield
        TC.connect_start(self.d_rows, d_start, self.d_gen, self.d_links, now, d_out, res, slot_stride=slot_stride,
                         frame_lead=frame_lead, flags=flags, nstart=ns, out_bytes=ob, max_frames=max_frames,
                         max_ready=max_ready, stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.start(start, now, C.LINKS, slot_stride=slot_stride, frame_lead=frame_lead, flags=flags,
                               max_frames=max_frames, out_bytes=ob, max_ready=max_ready)
        got = res.to_numpy()
        got["out"] = d_out.cpu().numpy()
        self._compare(got, exp, slot_stride, frame_lead, per_frame=False, state=state)
        return got, exp

    def process(self, frames, now=C.NOW, **kw):
        return run(self.process_steps(frames, now, **kw))

    def process_steps(self, frames, now=C.NOW, *, slot_stride=64, frame_lead=0, max_frames=None, max_ready=None,
                      out_size=None, out_bytes=None, flags=0, link=None, stream=None, state=True):
        import torch

        n = len(frames)
        rx = self.receive(frames)
        torch.cuda.synchronize()
        before = rx.to_numpy()
        max_frames = n if max_frames is None else max_frames
        max_ready = n if max_ready is None else max_ready
        d_out = self._out(max_frames, slot_stride, out_size)
        res = TC.ConnectResults(n, max_frames, max_ready, self.nrows, fill=FILL)
        d_link = None if link is None else TC.to_device(np.asarray(link, np.uint32))
        ob = d_out.numel() if out_bytes is None else out_bytes
        yield
        TC.connect_process(rx, self.d_rows, self.d_map, self.d_links, now, d_out, res, slot_stride=slot_stride,
                           frame_lead=frame_lead, flags=flags, link=d_link, out_bytes=ob, max_frames=max_frames,
                           max_ready=max_ready, stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.process(before, self.cmap, now, C.LINKS, slot_stride=slot_stride, frame_lead=frame_lead,
                                 flags=flags, max_frames=max_frames, out_bytes=ob, max_ready=max_ready, link=link)
        got = res.to_numpy()
        got["out"] = d_out.cpu().numpy()
        after = rx.to_numpy()
        for k in RX_KEYS:
            assert before[k].tobytes() == after[k].tobytes(), f"the batch's {k} was written"
        self._compare(got, exp, slot_stride, frame_lead, per_frame=True, state=state)
        return got, exp

    def timers(self, now, **kw):
        return run(self.timers_steps(now, **kw))

    def timers_steps(self, now, *, slot_stride=64, frame_lead=0, max_frames=64, max_ready=64, out_size=None, flags=0,
                     stream=None, state=True):
        import torch

        d_out = self._out(max_frames, slot_stride, out_size)
        res = TC.ConnectResults(4, max_frames, max_ready, self.nrows, fill=FILL)
        yield
        TC.connect_timers(self.d_rows, self.d_links, now, d_out, res, slot_stride=slot_stride, frame_lead=frame_lead,
                          flags=flags, max_frames=max_frames, max_ready=max_ready, stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.timers(now, C.LINKS, slot_stride=slot_stride, frame_lead=frame_lead, flags=flags,
                                max_frames=max_frames, out_bytes=d_out.numel(), max_ready=max_ready)
        got = res.to_numpy()
        got["out"] = d_out.cpu().numpy()
        self._compare(got, exp, slot_stride, frame_lead, per_frame=False, state=state)
        return got, exp


@pytest.fixture
def dev_factory():
    made = []

    def make(*a, **kw):
        made.append(Device(*a, **kw))
        return made[-1]

    yield make
    for d in made:
        d.close()


def isn(d, r):
    return int(d.model.rows[r]["local_isn"])


# ---- the connect scripts, a frame per call and as one batch ----------------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True])
def test_scripts(dev_factory, batched):
    """connect-blocking.pkt (row 0), connect-early-reset.pkt (row 1: `R. seq 0 ack 1`, here acknowledging the device's
    own ISN) and connect-refused.pkt (row 2: five SYNs three seconds apart, then ECONNREFUSED)."""
    flows, rows, cmap = C.client(3)
    d = dev_factory(flows, rows, cmap, nonce=0x1234)
    T0 = 1_000
    if batched:
        got, exp = d.start([0, 1, 2], T0)
        assert exp["n_frames"] == 3
    else:
        for r in range(3):
            d.start([r], T0)
    fr = [C.seg(0, R.SYN | R.ACK, seq=0, ack=isn(d, 0) + 1, options=C.OPT_MSS_WS0),
          C.seg(1, R.RST | R.ACK, seq=0, ack=isn(d, 1) + 1, options=C.OPT_MSS_WS0)]
    if batched:
        got, exp = d.process(fr, T0 + 100)
        acts, ready = list(exp["action"]), exp["ready"]
    else:
        outs = [d.process([f], T0 + 100)[1] for f in fr]
        acts, ready = [int(o["action"][0]) for o in outs], [o["ready"][0] for o in outs]
    assert acts == [TC.ESTABLISHED, TC.REFUSED]
    assert (int(ready[0]["err"]), int(ready[0]["rcv_nxt"]), int(ready[0]["mss"])) == (0, 1, 1450)
    assert (int(ready[1]["err"]), int(ready[1]["cause"])) == (errno.ECONNREFUSED, TC.CAUSE_RST)
    sent = 1
    for k in range(1, 6):
        got, exp = d.timers(T0 + k * TIMEOUT)
        sent += exp["n_frames"]
        assert (exp["n_frames"], exp["n_ready"]) == ((1, 0) if k < 5 else (0, 1))
    assert sent == 5 and int(exp["ready"][0]["err"]) == errno.ECONNREFUSED and int(exp["ready"][0]["row"]) == 2
    assert [int(s) for s in d.model.rows["state"]] == [TC.ESTAB, TC.FAILED, TC.FAILED]


# ---- the mixed batch ---------------------------------------------------------------------------------------------------------
def mixed_device(dev_factory):
    flows, rows, cmap, nonce, counter, patch, frames = C.mixed_batch()
    d = dev_factory(flows, rows, cmap, nonce, counter)
    got, exp = d.start(list(range(140)))
    assert exp["n_frames"] == 140 and d.model.counter == (counter + 140) & 0xFFFF < counter  # the counter wrapped
    d.patch({r: {"state": st} for r, st in patch.items()})
    return d, frames


def test_mixed_batch(dev_factory):
    d, frames = mixed_device(dev_factory)
    link = (np.arange(len(frames)) % 3).astype(np.uint32)  # 2 is out of range: the row's link
    got, exp = d.process(frames, link=link, slot_stride=80, frame_lead=6)
    assert set(int(a) for a in exp["action"]) == set(range(7)) and exp["n_ready"] >= 40
    assert set(int(s) for s in d.model.rows["state"]) == set(range(5))
    d2, frames = mixed_device(dev_factory)  # odd placement and the offload flag
    d2.process(frames, slot_stride=67, frame_lead=1, flags=N.DK_TX_OFFLOAD_TCP)


# ---- several frames for one row in one batch ----------------------------------------------------------------------------------
def test_many_frames_per_row(dev_factory):
    """EAGAIN frames up to and past syns_left (0, 1, 3), an accept after k EAGAINs with k at and one past the budget,
    FORWARD and ORPHANED tails, a refusal in the middle; and two rows that own 130 frames each, spread over a batch of
    more than two workgroups, so their ranks straddle the rank walk's 64-frame step and the 256-frame block."""
    budgets = (0, 1, 3)
    retries = [s + 1 for s in budgets for _ in range(4)] + [200, 65]
    flows, rows, cmap = C.client(len(retries), handshake_retries=retries)
    d = dev_factory(flows, rows, cmap, nonce=77, counter=5)
    d.start(list(range(len(retries))))
    scripts = []
    stray = lambda r: C.seg(r, R.ACK, seq=3, ack=isn(d, r) + 2)            # noqa: E731
    synack = lambda r: C.seg(r, R.SYN | R.ACK, seq=9, ack=isn(d, r) + 1)   # noqa: E731
    data = lambda r: C.seg(r, R.ACK | R.PSH, seq=10, ack=isn(d, r) + 1, payload=b"tail")  # noqa: E731
    for j, s in enumerate(budgets):
        r = 4 * j
        scripts.append([stray(r)] * (s + 2))                                  # up to and past the budget
        scripts.append([stray(r + 1)] * s + [synack(r + 1), data(r + 1), data(r + 1)])      # k = syns_left: FORWARD tail
        scripts.append([stray(r + 2)] * (s + 1) + [synack(r + 2), data(r + 2)])             # one past: ORPHANED tail
        scripts.append([stray(r + 3)] * s + [C.seg(r + 3, R.RST | R.ACK, ack=isn(d, r + 3) + 1), synack(r + 3)])
    big, big2 = len(retries) - 2, len(retries) - 1
    scripts.append([stray(big)] * 129 + [synack(big)])     # 129 retries of 199, then established
    scripts.append([stray(big2)] * 130)                    # 64 retries, exhausted, 65 orphans
    frames, pos = [], [0] * len(scripts)
    while any(p < len(s) for p, s in zip(pos, scripts)):   # round robin, each row's own order kept
        for si, s in enumerate(scripts):
            if pos[si] < len(s):
                frames.append(s[pos[si]])
                pos[si] += 1
                if si >= len(scripts) - 2:  # other traffic between the long rows' frames
                    frames.append(C.OTHER[len(frames) % len(C.OTHER)])
    assert len(frames) > 2 * 256
    got, exp = d.process(frames, 9_000_000_000)
    rows_after = d.model.rows
    assert rows_after[big]["state"] == TC.ESTAB and rows_after[big]["syns_left"] == 199 - 129
    assert rows_after[big2]["state"] == TC.FAILED and rows_after[big2]["syns_left"] == 0
    a2 = exp["action"][exp["row"] == big2]
    assert list(a2) == [TC.RETRY_SYN] * 64 + [TC.EXHAUSTED] + [TC.ORPHANED] * 65
    for j, s in enumerate(budgets):
        r = 4 * j
        assert list(exp["action"][exp["row"] == r]) == [TC.RETRY_SYN] * s + [TC.EXHAUSTED, TC.ORPHANED]
        assert list(exp["action"][exp["row"] == r + 1]) == [TC.RETRY_SYN] * s + [TC.ESTABLISHED, TC.FORWARD, TC.FORWARD]
        assert list(exp["action"][exp["row"] == r + 2]) == [TC.RETRY_SYN] * s + [TC.EXHAUSTED, TC.ORPHANED, TC.ORPHANED]
        assert list(exp["action"][exp["row"] == r + 3]) == [TC.RETRY_SYN] * s + [TC.REFUSED, TC.ORPHANED]
    # the same batch again: every row is past its handshake now
    got, exp = d.process(frames[:300], 9_000_000_001)
    assert set(int(a) for a in exp["action"]) == {TC.SKIP, TC.FORWARD, TC.ORPHANED}


# ---- options -------------------------------------------------------------------------------------------------------------------
def test_negotiation(dev_factory):
    flows, rows, cmap = C.client(4, window_scale=[14, 3, 3, 14], receive_window_size=[65535, 100, 100, 65535])
    d = dev_factory(flows, rows, cmap)
    d.start([0, 1, 2, 3])
    a = [isn(d, r) + 1 for r in range(4)]
    fr = [C.seg(0, R.SYN | R.ACK, seq=9, ack=a[0], win=65535, options=bytes([3, 3, 14])),   # window_scale 14, window 65535
          C.seg(1, R.SYN | R.ACK, seq=9, ack=a[1], win=7),                                   # none: 536, scales 0
          C.seg(2, R.SYN | R.ACK, seq=9, ack=a[2], win=7, options=bytes([3, 3, 15])),        # wscale 15 is taken as 14
          C.seg(3, R.SYN | R.ACK, seq=0xFFFFFFFF, ack=a[3], win=2, options=bytes([2, 4, 1, 0, 2, 4, 2, 0]))]  # last MSS
    got, exp = d.process(fr)
    y = got["ready"]
    assert [(int(r["mss"]), int(r["local_wscale"]), int(r["remote_wscale"])) for r in y[:4]] == \
        [(536, 14, 14), (536, 0, 0), (536, 3, 14), (512, 0, 0)]
    assert [(int(r["local_window"]), int(r["remote_window"])) for r in y[:4]] == \
        [(65535 << 14, 65535 << 14), (100, 7), (800, 7 << 14), (65535, 2)]
    assert int(y[3]["rcv_nxt"]) == 0


# ---- the ISN -------------------------------------------------------------------------------------------------------------------
def test_isn_counter_crc_wrap_duplicates_and_zero_retries(dev_factory):
    flows, rows, cmap = C.client(8, handshake_retries=[5, 5, 0, 1, 5, 5, 5, 5])
    nonce = 0xDEADBEEF
    crc = C.find_row_with_big_crc(rows, nonce)
    flows[len(C.EXTRA)]["remote_ip"], flows[len(C.EXTRA)]["remote_port"] = rows[0]["remote_ip"], rows[0]["remote_port"]
    d = dev_factory(flows, rows, cmap, nonce=nonce, counter=0xFFFD)
    start = [1, 2, 3, 0, 4, 1, 5]  # the counter goes 0xFFFD, 0xFFFE, 0xFFFF, 0, 1, 2, 3; row 1 is named twice
    got, exp = d.start(start)
    assert list(exp["status"]) == [TC.OK] * 5 + [TC.E_STATE, TC.OK] and d.model.counter == 4
    assert isn(d, 0) == crc and crc > 0xFFFF0000              # the fourth entry: the counter has wrapped to 0
    assert isn(d, 3) == R.crc_isn(rows[3], nonce, 0xFFFF) and isn(d, 5) == R.crc_isn(rows[5], nonce, 3)
    assert (exp["n_frames"], exp["n_ready"]) == (5, 1) and int(exp["ready"][0]["row"]) == 2  # handshake_retries 0
    assert d.model.rows[3]["syns_left"] == 0                   # handshake_retries 1: the one SYN is out
    got, exp = d.timers(C.NOW - 10 + TIMEOUT, max_frames=8, max_ready=8)
    assert int(d.model.rows[3]["state"]) == TC.FAILED and exp["n_frames"] == 4
    d2 = dev_factory(flows, rows, cmap, nonce=nonce, counter=0xFFFF)
    d2.start([0])
    assert isn(d2, 0) == (crc + 0xFFFF) & R.M32 < 0xFFFF       # crc + counter wrapped 2^32
    fr = F.tcp_frame(src=int(rows[0]["remote_ip"]), dst=C.BOB, sport=int(rows[0]["remote_port"]), dport=C.lport(0),
                     tcp_kw=dict(seq=5, ack=(isn(d2, 0) + 1) & R.M32, flags=R.SYN | R.ACK, window=100))
    got, exp = d2.process([fr])                                # the answer acknowledges the wrapped ISN
    assert exp["action"][0] == TC.ESTABLISHED


# ---- the row checks and the empty calls -------------------------------------------------------------------------------------------
def test_row_checks(dev_factory):
    flows, rows, cmap = C.client(8, window_scale=[0, 15, 0, 0, 0, 0, 0, 0], link=[0, 0, 9, 0, 0, 0, 0, 0])
    rows["state"][5] = TC.CLOSED
    d = dev_factory(flows, rows, cmap, nonce=1, counter=2)
    got, exp = d.start([0, 1, 2, 99, 3, 0, 4, 5, 6])
    assert list(exp["status"]) == [TC.OK, TC.E_WSCALE, TC.E_LINK, TC.E_ROW, TC.OK, TC.E_STATE, TC.OK, TC.E_STATE, TC.OK]
    got, exp = d.start([7], slot_stride=61)
    assert list(exp["status"]) == [TC.E_SLOT] and int(d.model.rows[7]["state"]) == TC.IDLE
    # a host that breaks a CONNECTING row: its frames are SKIP, its timer does not run, nothing of it changes
    d.patch({0: {"link": 9}, 3: {"window_scale": 15}})
    fr = [C.seg(r, R.SYN | R.ACK, seq=1, ack=isn(d, r) + 1) for r in (0, 3, 4)]
    got, exp = d.process(fr)
    assert list(exp["action"]) == [TC.SKIP, TC.SKIP, TC.ESTABLISHED]
    assert [int(exp["status"][r]) for r in (0, 3, 4, 6)] == [TC.E_LINK, TC.E_WSCALE, TC.OK, TC.OK]
    got, exp = d.timers(C.NOW + 10 * TIMEOUT)
    assert exp["frame_seg"] == [6] and [int(exp["status"][r]) for r in (0, 3)] == [TC.E_LINK, TC.E_WSCALE]
    got, exp = d.process([C.seg(6, R.SYN | R.ACK, seq=1, ack=isn(d, 6) + 1)], slot_stride=60)
    assert int(exp["status"][6]) == TC.E_SLOT and exp["action"][0] == TC.SKIP and got["n_frames"] == 0
    got, exp = d.timers(C.NOW + 20 * TIMEOUT, slot_stride=61)
    assert int(exp["status"][6]) == TC.E_SLOT and got["n_frames"] == 0


def test_empty_calls(dev_factory):
    flows, rows, cmap = C.client(2)
    d = dev_factory(flows, rows, cmap)
    got, exp = d.start([])
    assert (got["n_frames"], got["n_ready"]) == (0, 0)
    got, exp = d.timers(C.NOW)
    got, exp = d.process([C.OTHER[0], C.OTHER[1]])      # no frame for any row
    assert list(got["action"]) == [TC.SKIP] * 2
    e = dev_factory(flows, rows[:0], TC.conn_of_flow(len(flows), rows[:0]))  # nrows == 0
    got, exp = e.start([0])
    assert list(got["status"]) == [TC.E_ROW] and e.model.counter == 1
    got, exp = e.process([C.seg(0, R.SYN | R.ACK)])
    assert list(got["action"]) == [TC.SKIP]
    e.timers(C.NOW)


# ---- capacity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["max_frames", "out_bytes", "max_ready"])
def test_capacity_one_short(dev_factory, short):
    flows, rows, cmap, nonce, counter, patch, frames = C.mixed_batch()
    d = dev_factory(flows, rows, cmap, nonce, counter)
    # start: 140 SYNs and no record; the record limit is tried with a row of no retries
    d.patch({139: {"handshake_retries": 0}})
    kw = dict(max_frames=139, max_ready=1, out_size=139 * 64 + 64, out_bytes=139 * 64)
    kw[short] -= 1
    before = TC.rows_to_host(d.d_rows).tobytes()
    got, exp = d.start(list(range(140)), **kw)
    assert not exp["fits"] and (got["n_frames"], got["n_ready"]) == (139, 1) and set(got["status"]) == {TC.NO_ROOM}
    assert TC.rows_to_host(d.d_rows).tobytes() == before and d.model.counter == counter
    kw[short] += 1
    got, exp = d.start(list(range(140)), **kw)
    assert exp["fits"] and set(got["status"]) == {TC.OK}
    d.patch({r: {"state": st} for r, st in patch.items()})
    # process
    probe = R.ConnectModel(d.model.rows)
    need = probe.process(C.oracle_rx(frames, flows), cmap, C.NOW, C.LINKS, slot_stride=64, max_frames=1 << 20,
                         out_bytes=1 << 30, max_ready=1 << 20)
    nf, nr = need["n_frames"], need["n_ready"]
    kw = dict(max_frames=nf, max_ready=nr, out_size=nf * 64 + 64, out_bytes=nf * 64)
    kw[short] -= 1
    before = TC.rows_to_host(d.d_rows).tobytes()
    got, exp = d.process(frames, **kw)
    assert not exp["fits"] and (got["n_frames"], got["n_ready"]) == (nf, nr)
    assert set(got["status"]) == {TC.OK, TC.NO_ROOM} and TC.rows_to_host(d.d_rows).tobytes() == before
    kw[short] += 1
    got, exp = d.process(frames, **kw)  # exactly enough room
    assert exp["fits"] and set(got["status"]) == {TC.OK}
    # timers: what is still CONNECTING resends or gives up
    probe = R.ConnectModel(d.model.rows)
    need = probe.timers(C.NOW + 2 * TIMEOUT, C.LINKS, slot_stride=64, max_frames=1 << 20, out_bytes=1 << 30, max_ready=1 << 20)
    nf, nr = need["n_frames"], need["n_ready"]
    assert nf > 3 and nr > 3
    kw = dict(max_frames=nf, max_ready=nr, out_size=nf * 64 + 64)
    if short == "out_bytes":
        kw["out_size"] = nf * 64 - 1
    else:
        kw[short] -= 1
    before = TC.rows_to_host(d.d_rows).tobytes()
    got, exp = d.timers(C.NOW + 2 * TIMEOUT, **kw)
    assert not exp["fits"] and (got["n_frames"], got["n_ready"]) == (nf, nr) and TC.NO_ROOM in set(got["status"])
    assert TC.rows_to_host(d.d_rows).tobytes() == before
    got, exp = d.timers(C.NOW + 2 * TIMEOUT, max_frames=nf, max_ready=nr, out_size=nf * 64)
    assert exp["fits"]


# ---- timers ---------------------------------------------------------------------------------------------------------------------
def test_timers(dev_factory):
    T0 = 1_000_000
    n = 70  # more than a wave of rows
    flows, rows, cmap = C.client(n, handshake_retries=1 + np.arange(n) % 3, handshake_timeout_ns=1000 + np.arange(n) % 2)
    d = dev_factory(flows, rows, cmap, nonce=9)
    got, exp = d.start(list(range(0, n, 2)), T0 - 1)      # even rows: deadline T0 + 999
    first = bytes(got["out"][:TC.SYN_BYTES])
    d.start(list(range(1, n, 2)), T0)                     # odd rows: deadline T0 + 1001
    got, exp = d.timers(T0 + 998)
    assert (exp["n_frames"], exp["n_ready"]) == (0, 0)
    now = T0 + 999                                        # the even rows' deadline equals now
    got, exp = d.timers(now, max_frames=n, max_ready=n)
    even = list(range(0, n, 2))
    assert exp["frame_seg"] == [r for r in even if r % 3] and [int(y["row"]) for y in exp["ready"]] == [r for r in even if r % 3 == 0]
    assert bytes(got["out"][:TC.SYN_BYTES]) != first       # row 2's SYN; row 0 gave up
    got, exp = d.timers(now)                               # nothing is due
    assert (exp["n_frames"], exp["n_ready"]) == (0, 0)
    seen = 0
    for step in range(1, 5):                               # resend until exhausted, ascending row order each time
        got, exp = d.timers(now + step * 1001, max_frames=n, max_ready=n)
        assert exp["frame_seg"] == sorted(exp["frame_seg"])
        rr = [int(y["row"]) for y in exp["ready"]]
        assert rr == sorted(rr) and all(int(y["frame"]) == TC.NONE for y in exp["ready"])
        seen += len(rr)
    assert (d.model.rows["state"] == TC.FAILED).all() and seen == n - len([r for r in even if r % 3 == 0])
    got, exp = d.process([C.seg(1, R.SYN | R.ACK, ack=isn(d, 1) + 1)], now + 9000)  # a failed socket swallows its frames
    assert exp["action"][0] == TC.ORPHANED
