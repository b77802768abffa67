"""dk_arp_process / _query_start / _timers / _lookup on the MI355X against tests/arp_reference.py (pinned on the CPU by
tests/test_arp_model.py). The frames go through the receive engine first, so the per-frame arrays are the engine's own.
Every call is compared whole: the output blob and every result array over canary fills, the table as a map from ip to
(mac, expiration), the query rows and links[] as bytes, and the batch's arrays unchanged.

dk_arp_process has one kernel form for every batch size (one lane per frame, sender, slot and row), so there is no form
override to run the cases under; the 257-frame case crosses the workgroup boundary of that one form."""
import numpy as np
import pytest

import arp_cases as C
import arp_reference as R
import frames as F
from demikernel_amd import Config, FrameBatch, RxEngine, ipv4, synth
from demikernel_amd import _native as N
from demikernel_amd import arp as ARP
from ctl_calls import run

pytestmark = pytest.mark.gpu

CANARY, FILL = 0xA5, 0x5A
FILL32, FILL16 = 0x5A5A5A5A, 0x5A5A
RX_KEYS = ("meta", "src_ip", "dst_ip", "ports", "payload", "flow_id")


class Device:
    """A peer on the device: the receive engine, the table, the query rows and links; and the model beside it."""

    def __init__(self, case: C.Case):
        self.case = case
        self.eng = RxEngine(Config(case.local), device=0)
        self.eng.set_sockets(synth.make_flows(4))
        cfg = ARP.arp_cfg(ipv4(case.local), C.MACS[case.local], cache_ttl_ns=case.ttl, request_timeout_ns=case.timeout,
                          retry_count=case.retries, disabled=case.disabled)
        self.table = ARP.ArpTable(case.cap, cfg)
        self.model = case.model()
        if case.initial:
            self.table.insert([(ipv4(a), m) for a, m in case.initial], case.initial_clock)
        self.d_rows = None if case.rows is None else ARP.to_device(case.rows)
        self.d_links = None if case.links is None else ARP.to_device(case.links)
        self.compare_state()

    def close(self):
        self.table.close()
        self.eng.close()

    def _out(self, max_frames, slot_stride):
        import torch

        return torch.full((max(max_frames, 1) * slot_stride + 64,), CANARY, dtype=torch.uint8, device="cuda:0")

    def compare_state(self):
        assert self.table.as_map() == self.model.table()
        if self.d_rows is not None:
            g = ARP.rows_to_host(self.d_rows)
            if g.tobytes() != self.model.rows.tobytes():
                bad = [r for r in range(len(g)) if g[r].tobytes() != self.model.rows[r].tobytes()]
                raise AssertionError(f"rows {bad[:6]} differ: got {g[bad[0]]} expected {self.model.rows[bad[0]]}")
        if self.d_links is not None:
            assert self.d_links.cpu().numpy().tobytes() == self.model.links.tobytes(), "links[] differ"

    def _compare(self, got, exp, slot_stride, frame_lead, per_frame, state=True):
        assert (got["n_frames"], got["n_ready"], got["n_entries"]) == (exp["n_frames"], exp["n_ready"], exp["n_entries"])
        assert np.array_equal(got["status"], exp["status"]), (got["status"], exp["status"])
        if per_frame and exp["fits"]:
            for k in ("action", "reply_frame"):
                if not np.array_equal(got[k], exp[k]):
                    bad = np.nonzero(got[k] != exp[k])[0][:8]
                    raise AssertionError(f"{k} differs at {bad}: got {got[k][bad]} expected {exp[k][bad]}")
        else:  # nothing is written
            assert (got["action"] == FILL).all() and (got["reply_frame"] == FILL32).all()
        w, y = (exp["n_frames"], exp["n_ready"]) if exp["fits"] else (0, 0)
        assert np.array_equal(got["off_out"][:w], np.arange(w, dtype=np.uint32) * slot_stride + frame_lead)
        assert (got["len_out"][:w] == 42).all()
        assert np.array_equal(got["frame_seg"][:w], np.array(exp["frame_seg"][:w], np.uint32))
        for j in range(y):
            assert got["ready"][j].tobytes() == exp["ready"][j].tobytes(), (j, got["ready"][j], exp["ready"][j])
        assert (got["off_out"][w:] == FILL32).all() and (got["len_out"][w:] == FILL16).all()
        assert (got["frame_seg"][w:] == FILL32).all() and (got["ready"][y:].view(np.uint8) == FILL).all()
        want = R.blob_of(exp["frames"] if exp["fits"] else [], slot_stride, frame_lead, len(got["out"]), CANARY)
        if not np.array_equal(got["out"], want):
            bad = np.nonzero(got["out"] != want)[0]
            raise AssertionError(f"{len(bad)} output bytes differ, first at {bad[:8]}: got {got['out'][bad[:8]]} "
                                 f"expected {want[bad[:8]]}")
        if state:
            self.compare_state()

    def process(self, frames, clock, **kw):
        return run(self.process_steps(frames, clock, **kw))

    def process_steps(self, frames, clock, *, slot_stride=64, frame_lead=0, max_frames=None, max_ready=None,
                      out_bytes=None, stream=None, state=True):
        """process() in the three steps of ctl_calls.Call: the uploads and fills, the call (on `stream`), the wait and
        the comparison. state=False leaves the table, rows and links to a later call's comparison. The same for start
        and timers."""
        import torch

        n = len(frames)
        blob, off, lens = F.pack([C.raw(f) for f in frames])
        batch = FrameBatch.from_numpy(blob, off, lens)
        rx = self.eng.results(n)
        if n:
            self.eng.receive_batch(batch, rx)
        torch.cuda.synchronize()
        before = rx.to_numpy()
        mf = C.model_frames(frames)
        for i, f in enumerate(mf):  # the engine's own arrays are what the model's frames say
            assert ((int(before["meta"][i]) & 0xFF) == N.V["ARP"]) == f.covered
            if f.covered:
                assert (int(before["meta"][i]) >> 16, int(before["src_ip"][i]), int(before["dst_ip"][i])) == (f.op, f.spa, f.tpa)
        max_frames = n if max_frames is None else max_frames
        max_ready = (0 if self.d_rows is None else len(self.model.rows)) if max_ready is None else max_ready
        d_out = self._out(max_frames, slot_stride)
        ob = d_out.numel() if out_bytes is None else out_bytes
        res = ARP.ArpResults(n, max_frames, max_ready, 1, fill=FILL)
        yield
        ARP.arp_process(self.table, batch, rx, self.d_rows, self.d_links, clock, d_out, res, slot_stride=slot_stride,
                        frame_lead=frame_lead, n=n, out_bytes=ob, max_frames=max_frames, max_ready=max_ready,
                        stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.process(mf, clock, slot_stride=slot_stride, frame_lead=frame_lead, max_frames=max_frames,
                                 out_bytes=ob, max_ready=max_ready)
        got = res.to_numpy()
        got["out"] = d_out.cpu().numpy()
        after = rx.to_numpy()
        for k in RX_KEYS:
            assert before[k].tobytes() == after[k].tobytes(), f"the batch's {k} was written"
        assert np.array_equal(batch.blob.cpu().numpy(), blob) and np.array_equal(batch.off.cpu().numpy().view(np.uint32), off)
        self._compare(got, exp, slot_stride, frame_lead, per_frame=True, state=state)
        return got, exp

    def start(self, start, now, **kw):
        return run(self.start_steps(start, now, **kw))

    def start_steps(self, start, now, *, slot_stride=64, frame_lead=0, max_frames=None, max_ready=None, out_bytes=None,
                    stream=None, state=True):
        import torch

        ns = len(start)
        max_frames = ns if max_frames is None else max_frames
        max_ready = ns if max_ready is None else max_ready
        d_out = self._out(max_frames, slot_stride)
        ob = d_out.numel() if out_bytes is None else out_bytes
        res = ARP.ArpResults(4, max_frames, max_ready, max(ns, 1), fill=FILL)
        d_start = ARP.to_device(np.asarray(start, np.uint32)) if ns else torch.zeros(4, dtype=torch.uint8, device="cuda:0")
        yield
        ARP.arp_query_start(self.table, self.d_rows, d_start, self.d_links, now, d_out, res, slot_stride=slot_stride,
                            frame_lead=frame_lead, nstart=ns, out_bytes=ob, max_frames=max_frames, max_ready=max_ready,
                            stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.start(start, now, slot_stride=slot_stride, frame_lead=frame_lead, max_frames=max_frames,
                               out_bytes=ob, max_ready=max_ready)
        got = res.to_numpy()
        got["out"] = d_out.cpu().numpy()
        if ns == 0:
            assert (got["status"] == FILL32).all()
            got["status"] = got["status"][:0]
        self._compare(got, exp, slot_stride, frame_lead, per_frame=False, state=state)
        return got, exp

    def timers(self, now, **kw):
        return run(self.timers_steps(now, **kw))

    def timers_steps(self, now, *, slot_stride=64, frame_lead=0, max_frames=64, max_ready=64, out_bytes=None, stream=None,
                     state=True):
        import torch

        d_out = self._out(max_frames, slot_stride)
        ob = d_out.numel() if out_bytes is None else out_bytes
        res = ARP.ArpResults(4, max_frames, max_ready, 1, fill=FILL)
        yield
        ARP.arp_timers(self.table, self.d_rows, self.d_links, now, d_out, res, slot_stride=slot_stride,
                       frame_lead=frame_lead, out_bytes=ob, max_frames=max_frames, max_ready=max_ready, stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.timers(now, slot_stride=slot_stride, frame_lead=frame_lead, max_frames=max_frames, out_bytes=ob,
                                max_ready=max_ready)
        got = res.to_numpy()
        got["out"] = d_out.cpu().numpy()
        self._compare(got, exp, slot_stride, frame_lead, per_frame=False, state=state)
        return got, exp

    def lookup(self, ips, link=None, stream=None, state=True):
        found, macs = ARP.arp_lookup(self.table, [ipv4(a) for a in ips], self.d_links, link, stream=stream, fill=FILL)
        efound, emacs = self.model.lookup([ipv4(a) for a in ips], link)
        assert np.array_equal(found, efound) and np.array_equal(macs, emacs), (found, efound, macs, emacs)
        if state:
            self.compare_state()
        return found, macs

    def run(self):
        outs = []
        for st in self.case.steps:
            if st[0] == "process":
                outs.append(self.process(st[1], st[2], **st[3]))
            elif st[0] == "start":
                outs.append(self.start(st[1], st[2], **st[3]))
            elif st[0] == "timers":
                outs.append(self.timers(st[1], **st[2]))
            elif st[0] == "lookup":
                outs.append(self.lookup(st[1], st[2]))
            elif st[0] == "insert":
                self.table.insert([(ipv4(a), m) for a, m in st[1]], st[2])
                self.model.insert_initial([(ipv4(a), m) for a, m in st[1]], st[2])
                self.compare_state()
                outs.append(None)
        return outs


@pytest.fixture
def dev_factory():
    made = []

    def make(case):
        made.append(Device(case))
        return made[-1]

    yield make
    for d in made:
        d.close()


@pytest.mark.parametrize("make", C.MODEL_CASES + C.DEVICE_CASES, ids=lambda f: getattr(f, "__name__", "shape"))
def test_case_against_the_model(dev_factory, make):
    case = make()
    outs = dev_factory(case).run()
    assert len(outs) == len(case.steps)


def test_cases_have_the_shapes_they_claim(dev_factory):
    """The properties the shapes exist for, on the device's own results."""
    d = dev_factory(C.second_wave(False))
    (got, exp), _ = d.run()
    assert list(got["action"][63:65]) == [R.LEARNED | R.INSERTED | R.REPLY, R.HIT | R.INSERTED] and got["n_frames"] == 64
    assert bytes(ARP.rows_to_host(d.d_rows)[0]["mac"]) == C.mac_of(63)
    assert d.table.as_map()[ipv4(C.host(500))][0] == C.mac_of(64)
    d = dev_factory(C.second_wave(True))
    (got, exp), _ = d.run()
    assert list(got["action"][:64]) == [R.DROPPED] * 64 and got["action"][64] == R.LEARNED | R.INSERTED
    assert (got["n_frames"], got["n_ready"], got["n_entries"]) == (0, 1, 1)
    d = dev_factory(C.many_waiters())
    ((got, exp),) = d.run()
    order = [(int(y["frame"]), int(y["row"])) for y in got["ready"][:got["n_ready"]]]
    assert order == [(0, 71), (1, 70), (1, 73)] + [(3, r) for r in list(range(70)) + [72]]
    d = dev_factory(C.interleaved())
    (got, exp), _ = d.run()
    assert (got["action"][0::2] == ARP.SKIP).all() and (got["action"][1::2] != ARP.SKIP).all()


def test_chain_that_wraps_with_a_tombstone_in_the_middle(dev_factory):
    """cap 4, three keys whose walk starts at slot 3: LIVE at 3, a tombstone at 0, LIVE at 1. A lookup walks across the
    tombstone; at the clock where the entry at 1 expires, an insert of a fourth key of the chain claims slot 0."""
    keys = [ip for ip in range(1, 4000) if ARP.home(4, ip) == 3][:4]
    k1, k3, k4, k5 = keys
    a = lambda ip: ".".join(str(b) for b in ip.to_bytes(4, "little"))  # noqa: E731
    d = dev_factory(C.Case("chain", cap=4))
    rows = np.zeros(4, ARP.SLOT_DTYPE)
    rows[3]["ip"], rows[3]["state"], rows[3]["mac"], rows[3]["expiration_ns"] = k1, ARP.LIVE, list(C.mac_of(1)), 100 * C.TTL
    rows[0]["state"] = ARP.TOMBSTONE
    rows[1]["ip"], rows[1]["state"], rows[1]["mac"], rows[1]["expiration_ns"] = k3, ARP.LIVE, list(C.mac_of(3)), 50
    d.table.write(rows)
    d.model.cache.d = {k1: (C.mac_of(1), 100 * C.TTL), k3: (C.mac_of(3), 50)}
    assert d.table.consumed() == 3
    found, _ = d.lookup([a(k3), a(k1), a(k4)])
    assert list(found) == [1, 1, 0]
    got, exp = d.process([C.rep(a(k4), C.ALICE, sha=C.mac_of(4))], 50)
    assert got["n_entries"] == 2 and got["status"][0] == ARP.OK
    after = d.table.rows()
    assert [int(s) for s in after["state"]] == [ARP.LIVE, ARP.TOMBSTONE, ARP.FREE, ARP.LIVE]
    assert (int(after[0]["ip"]), bytes(after[0]["mac"]), int(after[0]["expiration_ns"])) == (k4, C.mac_of(4), 50 + C.TTL)
    assert d.table.consumed() == 3  # the claimed slot was a tombstone
    found, _ = d.lookup([a(k3), a(k1), a(k4), a(k5)])
    assert list(found) == [0, 1, 1, 0]
    got, exp = d.process([C.rep(a(k5), C.ALICE)], 60)  # a third LIVE entry does not fit cap / 2
    assert got["n_entries"] == 3 and got["status"][0] == ARP.NO_ROOM and not exp["fits"]
    assert np.array_equal(d.table.rows(), after)


def test_start_row_errors_and_duplicates(dev_factory):
    rows = np.concatenate([C.idle([C.BOB, C.CARRIE, C.host(1), C.host(2)], links=[0, 1, 7, R.NO_LINK]), C.waiting([C.host(3)])])
    d = dev_factory(C.Case("start_errors", initial=[(C.BOB, C.BOB_MAC)], rows=rows, links=C.links_of(2)))
    got, exp = d.start([1, 9, 1, 4, 2, 0, 3, 0], 77)
    assert list(got["status"]) == [R.OK, R.E_ROW, R.E_STATE, R.E_STATE, R.E_LINK, R.OK, R.OK, R.E_STATE]
    assert (got["n_frames"], got["n_ready"]) == (2, 1) and list(got["frame_seg"][:2]) == [0, 6]
    got, exp = d.start([1], 78)
    assert list(got["status"]) == [R.E_STATE]
    d2 = dev_factory(C.Case("start_slot", initial=[(C.BOB, C.BOB_MAC)], rows=C.idle([C.BOB, C.CARRIE])))
    got, exp = d2.start([0, 1], 5, slot_stride=64, frame_lead=23)
    assert list(got["status"]) == [R.E_SLOT, R.E_SLOT] and (got["n_frames"], got["n_ready"]) == (0, 0)
    got, exp = d2.start([0, 1], 5, slot_stride=64, frame_lead=22)
    assert list(got["status"]) == [R.OK, R.OK] and (got["n_frames"], got["n_ready"]) == (1, 1)
    got, exp = d2.timers(5 + C.SEC, slot_stride=41)
    assert got["status"][0] == R.E_SLOT and got["n_frames"] == 1


def test_timers_to_etimedout_with_the_deadline_as_boundary(dev_factory):
    d = dev_factory(C.Case("expiries", retries=2, rows=C.idle([C.CARRIE, C.host(1)], links=[0, R.NO_LINK]), links=C.links_of(1)))
    got, _ = d.start([0, 1], 0)
    assert got["n_frames"] == 2
    sent = 1
    for k in (1, 2):
        got, _ = d.timers(k * C.SEC - 1)  # one tick before the deadline: nothing
        assert (got["n_frames"], got["n_ready"]) == (0, 0)
        got, _ = d.timers(k * C.SEC)      # deadline_ns == now_ns
        sent += 1
        assert (got["n_frames"], got["n_ready"]) == (2, 0)
        assert list(ARP.rows_to_host(d.d_rows)["sent"]) == [sent, sent]
    got, _ = d.timers(3 * C.SEC)
    assert (got["n_frames"], got["n_ready"]) == (0, 2) and [int(y["err"]) for y in got["ready"][:2]] == [110, 110]
    assert list(ARP.rows_to_host(d.d_rows)["state"]) == [R.FAILED, R.FAILED]
    got, _ = d.timers(9 * C.SEC)
    assert (got["n_frames"], got["n_ready"]) == (0, 0)


def test_each_capacity_limit_one_short(dev_factory):
    """max_frames, out_bytes, max_ready and cap / 2, each one short: the three words report the need and nothing else is
    written (the harness compares every array, the table, the rows and links with their state before the call)."""
    fr = [C.req(C.host(1), C.ALICE), C.rep(C.host(2), C.ALICE), C.req(C.host(3), C.ALICE)]

    def fresh(cap=64):
        return dev_factory(C.Case("room", cap=cap, rows=C.waiting([C.host(2), C.host(3), C.host(9)], links=[0, 1, 0]),
                                  links=C.links_of(2)))

    for kw in ({"max_frames": 1}, {"out_bytes": 2 * 64 - 1}, {"max_ready": 1}):
        d = fresh()
        got, exp = d.process(fr, 4, **kw)
        assert not exp["fits"] and got["status"][0] == R.NO_ROOM
        assert (got["n_frames"], got["n_ready"], got["n_entries"]) == (2, 2, 3)
        got, exp = d.process(fr, 4)  # with room the same call goes through
        assert exp["fits"] and got["status"][0] == R.OK
    d = fresh(cap=4)
    got, exp = d.process(fr, 4)
    assert not exp["fits"] and got["status"][0] == R.NO_ROOM and got["n_entries"] == 3 and d.table.as_map() == {}
    got, exp = d.process(fr[:2], 4)
    assert exp["fits"] and got["n_entries"] == 2
    # start and timers
    d = dev_factory(C.Case("room_start", initial=[(C.BOB, C.BOB_MAC)], rows=C.idle([C.BOB, C.CARRIE, C.host(1)])))
    for kw in ({"max_frames": 1}, {"out_bytes": 2 * 64 - 1}, {"max_ready": 0}):
        got, exp = d.start([0, 1, 2], 0, **kw)
        assert not exp["fits"] and list(got["status"]) == [R.NO_ROOM] * 3 and (got["n_frames"], got["n_ready"]) == (2, 1)
    got, exp = d.start([0, 1, 2], 0)
    assert exp["fits"]
    for kw in ({"max_frames": 1}, {"out_bytes": 2 * 64 - 1}):
        got, exp = d.timers(C.SEC, **kw)
        assert not exp["fits"] and got["status"][0] == R.NO_ROOM and got["n_frames"] == 2
    got, exp = d.timers(C.SEC)
    assert exp["fits"] and got["n_frames"] == 2
