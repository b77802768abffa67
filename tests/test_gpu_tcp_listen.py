"""dk_tcp_listen_process / _timers / _release on the MI355X against tests/tcp_listen_reference.py (pinned on the CPU by
tests/test_tcp_listen_model.py). The frames go through the receive engine first, so the per-frame arrays are the
engine's own. Every call is compared whole: the output blob and every result array over canary fills, the table as a map
from key to fields (slot numbers are never compared: a slot only has to hold the key it is reported for), the listener
rows as bytes, and the batch's arrays unchanged."""
import errno

import numpy as np
import pytest

import frames as F
import tcp_listen_cases as C
import tcp_listen_reference as R
from demikernel_amd import Config, FrameBatch, RxEngine
from demikernel_amd import _native as N
from demikernel_amd import tcp_listen as TL
from demikernel_amd.rx import Fail
from ctl_calls import run

pytestmark = pytest.mark.gpu

CANARY, FILL = 0xA5, 0x5A
FILL32, FILL16 = 0x5A5A5A5A, 0x5A5A
SLOT_FIELDS = ("state", "err", "remote_isn", "local_isn", "syn_window", "mss", "remote_wscale", "retries_left",
               "deadline_ns")
RX_KEYS = ("meta", "src_ip", "ports", "payload", "flow_id", "tcp_seq", "tcp_ack", "tcp_win")


def receive(eng, frames):
    """The frames through a receive engine: (its results with the TCP fields and option records, the batch)."""
    blob, off, lens = F.pack(frames)
    batch = FrameBatch.from_numpy(blob, off, lens)
    rx = eng.results(len(frames), tcp_fields=True, tcp_opts=True)
    eng.receive_batch(batch, rx)
    return rx, batch


class Device:
    """A server on the device: the receive engine, the listeners, the table; and the model beside it."""

    def __init__(self, flows, L, lsn, cap=1024, isn=R.crc_isn):
        self.eng = RxEngine(Config(C.BOB), device=0)
        self.eng.set_sockets(flows)
        self.table = TL.ListenTable(cap)
        self.d_L, self.d_lsn, self.d_links = TL.to_device(L), TL.to_device(lsn), TL.to_device(C.LINKS)
        self.lsn, self.nl = lsn, len(L)
        self.model = R.ListenModel(L, cap, isn)
        self.backlog_sum = int(L["max_backlog"].astype(np.uint64).sum())

    def close(self):
        self.table.close()
        self.eng.close()

    def receive(self, frames):
        return receive(self.eng, frames)

    def _out(self, max_frames, slot_stride, out_size):
        import torch

        size = max(max_frames, 1) * slot_stride + 64 if out_size is None else out_size
        return torch.full((size,), CANARY, dtype=torch.uint8, device="cuda:0")

    def process(self, frames, now=C.NOW, **kw):
        """One dk_tcp_listen_process call on `frames`, compared whole with the model's."""
        return run(self.process_steps(frames, now, **kw))

    def process_steps(self, frames, now=C.NOW, *, slot_stride=64, frame_lead=0, max_frames=None, max_ready=None,
                      out_size=None, out_bytes=None, flags=0, link=None, compare=True, stream=None, state=True,
                      released=()):
        """process() in the three steps of ctl_calls.Call: the uploads and fills, the call (on `stream`), the wait and
        the comparison. state=False leaves the tables to a later call's comparison; `released` are keys a later call
        has taken out of the table by then."""
        import torch

        n = len(frames)
        rx, batch = self.receive(frames)
        torch.cuda.synchronize()
        before = rx.to_numpy()
        max_frames = n if max_frames is None else max_frames
        max_ready = n if max_ready is None else max_ready
        d_out = self._out(max_frames, slot_stride, out_size)
        res = TL.ListenResults(n, max_frames, max_ready, self.nl, fill=FILL)
        d_link = None if link is None else TL.to_device(np.asarray(link, np.uint32))
        ob = d_out.numel() if out_bytes is None else out_bytes
        yield
        TL.listen_process(self.table, rx, self.d_L, self.d_lsn, self.d_links, now, d_out, res, slot_stride=slot_stride,
                          frame_lead=frame_lead, flags=flags, backlog_sum=self.backlog_sum, link=d_link, out_bytes=ob,
                          max_frames=max_frames, max_ready=max_ready, stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.process(before, self.lsn, now, C.LINKS, slot_stride=slot_stride, frame_lead=frame_lead,
                                 flags=flags, max_frames=max_frames, out_bytes=ob, max_ready=max_ready, link=link)
        got = res.to_numpy()
        got["out"] = d_out.cpu().numpy()
        after = rx.to_numpy()
        for k in RX_KEYS + ("tcp_opts",):
            assert before[k].tobytes() == after[k].tobytes(), f"the batch's {k} was written"
        if compare:
            self.compare_process(got, exp, n, max_frames, max_ready, slot_stride, frame_lead, released)
            if state:
                self.compare_state()
        return got, exp

    def compare_process(self, got, exp, n, max_frames, max_ready, slot_stride, frame_lead, released=()):
        assert (got["n_frames"], got["n_ready"]) == (exp["n_frames"], exp["n_ready"])
        assert np.array_equal(got["status"], exp["status"]), (got["status"], exp["status"])
        rows = self.table.rows()
        if not exp["fits"]:  # nothing is written
            assert (got["action"] == FILL).all() and (got["slot"] == FILL32).all() and (got["reply_frame"] == FILL32).all()
            w = y = 0
        else:
            if not np.array_equal(got["action"], exp["action"]):
                bad = np.nonzero(got["action"] != exp["action"])[0][:8]
                raise AssertionError(f"action differs at {bad}: got {got['action'][bad]} expected {exp['action'][bad]}")
            assert np.array_equal(got["reply_frame"], exp["reply_frame"])
            for i in range(n):  # the slot holds the key, or there is none
                k = exp["keys"][i]
                if k is None:
                    assert got["slot"][i] == TL.NONE, i
                elif k in released:
                    assert int(rows[got["slot"][i]]["key"]) == TL.KEY_TOMBSTONE, i
                else:
                    assert got["slot"][i] < len(rows) and int(rows[got["slot"][i]]["key"]) == k, (i, TL.ACTIONS[exp["action"][i]])
            w, y = exp["n_frames"], exp["n_ready"]
            assert np.array_equal(got["off_out"][:w], np.arange(w, dtype=np.uint32) * slot_stride + frame_lead)
            assert np.array_equal(got["len_out"][:w], np.array([len(f) for f in exp["frames"]], np.uint16))
            assert np.array_equal(got["frame_seg"][:w], np.array(exp["frame_seg"], np.uint32))
            for j in range(y):
                g, e = got["ready"][j].copy(), exp["ready"][j].copy()
                want_key = TL.KEY_TOMBSTONE if exp["ready_keys"][j] in released else exp["ready_keys"][j]
                assert int(rows[g["slot"]]["key"]) == want_key, j
                g["slot"] = e["slot"] = 0
                assert g.tobytes() == e.tobytes(), (j, g, e)
        assert (got["off_out"][w:] == FILL32).all() and (got["len_out"][w:] == FILL16).all()
        assert (got["frame_seg"][w:] == FILL32).all()
        assert (got["ready"][y:].view(np.uint8) == FILL).all()
        want = R.blob_of(exp["frames"], slot_stride, frame_lead, len(got["out"]), CANARY)
        if not np.array_equal(got["out"], want):
            bad = np.nonzero(got["out"] != want)[0]
            raise AssertionError(f"{len(bad)} output bytes differ, first at {bad[:8]}: got {got['out'][bad[:8]]} "
                                 f"expected {want[bad[:8]]}")

    def compare_state(self):
        got, exp = self.table.as_map(), self.model.table_rows()
        assert set(got) == set(exp), (sorted(set(got) ^ set(exp))[:4], len(got), len(exp))
        for k, e in exp.items():
            for f in SLOT_FIELDS:
                assert int(got[k][f]) == int(e[f]), (hex(k), f, int(got[k][f]), int(e[f]))
        rows = self.table.rows()
        for r in rows:  # FREE and TOMBSTONE slots hold nothing else
            if r["state"] in (TL.FREE, TL.TOMBSTONE):
                assert int(r["key"]) == (TL.KEY_FREE if r["state"] == TL.FREE else TL.KEY_TOMBSTONE)
                z = r.copy()
                z["key"], z["state"] = 0, 0
                assert not z.tobytes().strip(b"\0")
        assert self.table.consumed() == int((rows["state"] != TL.FREE).sum())
        gl = TL.listeners_to_host(self.d_L)
        assert gl.tobytes() == self.model.listeners.tobytes(), [(a, b) for a, b in zip(gl, self.model.listeners) if a != b][:2]

    def timers(self, now, **kw):
        return run(self.timers_steps(now, **kw))

    def timers_steps(self, now, *, slot_stride=64, frame_lead=0, max_frames=64, max_ready=64, out_size=None, flags=0,
                     stream=None):
        import torch

        d_out = self._out(max_frames, slot_stride, out_size)
        res = TL.ListenResults(0, max_frames, max_ready, self.nl, fill=FILL)
        yield
        TL.listen_timers(self.table, self.d_L, self.d_links, now, d_out, res, slot_stride=slot_stride,
                         frame_lead=frame_lead, flags=flags, backlog_sum=self.backlog_sum, max_frames=max_frames,
                         max_ready=max_ready, stream=stream)
        yield
        torch.cuda.synchronize()
        exp = self.model.timers(now, C.LINKS, slot_stride=slot_stride, frame_lead=frame_lead, flags=flags,
                                max_frames=max_frames, out_bytes=d_out.numel(), max_ready=max_ready)
        got = res.to_numpy()
        out = d_out.cpu().numpy()
        assert (got["n_frames"], got["n_ready"]) == (exp["n_frames"], exp["n_ready"])
        assert np.array_equal(got["status"], exp["status"])
        w, y = (exp["n_frames"], exp["n_ready"]) if exp["fits"] else (0, 0)
        rows = self.table.rows()
        # frames and records follow slot order, which is unspecified: both sides are sorted by key
        assert np.array_equal(got["off_out"][:w], np.arange(w, dtype=np.uint32) * slot_stride + frame_lead)
        assert (got["len_out"][:w] == TL.SYNACK_BYTES).all()
        gf = {int(rows[got["frame_seg"][f]]["key"]): out[f * slot_stride + frame_lead:][:TL.SYNACK_BYTES].tobytes()
              for f in range(w)}
        assert gf == dict(zip(exp["frame_seg"], exp["frames"]))
        mask = np.ones(len(out), bool)
        for f in range(w):
            mask[f * slot_stride + frame_lead:f * slot_stride + frame_lead + TL.SYNACK_BYTES] = False
        assert (out[mask] == CANARY).all()
        gr = {}
        for j in range(y):
            g = got["ready"][j].copy()
            k = int(rows[g["slot"]]["key"])
            g["slot"] = 0
            gr[k] = g.tobytes()
        assert gr == {k: e.tobytes() for k, e in zip(exp["ready_keys"], exp["ready"])}
        assert (got["off_out"][w:] == FILL32).all() and (got["ready"][y:].view(np.uint8) == FILL).all()
        self.compare_state()
        return got, exp, gf

    def release(self, keys, stream=None):
        found = TL.listen_release(self.table, self.d_L, keys, stream=stream)
        assert [int(x) for x in found] == self.model.release(keys)
        self.compare_state()
        return found


@pytest.fixture
def dev_factory():
    made = []

    def make(*a, **kw):
        made.append(Device(*a, **kw))
        return made[-1]

    yield make
    for d in made:
        d.close()


# ---- the accept scripts, a frame per call and as one batch --------------------------------------------------------------
def script_frames(rem, port):
    A, S, RS, P = R.ACK, R.SYN, R.RST, R.PSH
    o = C.OPT_MSS_WS0
    return [C.seg(rem, port, A, seq=0, ack=1, options=o), C.seg(rem, port, P, options=o), C.seg(rem, port, RS, options=o),
            C.seg(rem, port, P | A, options=o), C.seg(rem, port, RS | A, options=o), C.seg(rem, port, S | A, options=o),
            C.seg(rem, port, S, options=o, payload=b"d" * 1000), C.seg(rem, port, A, seq=1, ack=1, options=C.OPT_NOP)]


@pytest.mark.parametrize("batched", [False, True])
def test_scripts_zero_isn_sequence(dev_factory, batched):
    """The refuse scripts' lines and the data-carrying SYN, replayed with a nonce-free listener; the handshake ACK
    acknowledges the device's own ISN."""
    flows, L, lsn = C.server([80], max_backlog=1)
    d = dev_factory(flows, L, lsn, cap=64)
    rem = C.remote(1)
    fr = script_frames(rem, 80)
    fr[-1] = C.seg(rem, 80, R.ACK, seq=1, ack=C.isn_of(L[0], rem, 0) + 1, options=C.OPT_NOP)
    if batched:
        got, exp = d.process(fr)
        acts = list(exp["action"])
    else:
        acts = [int(d.process([f])[1]["action"][0]) for f in fr]
    assert acts == [TL.RST_FLAGS] * 6 + [TL.SYN_ACCEPTED, TL.ESTABLISHED]
    assert d.model.listeners[0]["inflight"] == 1


# ---- the mixed batch ------------------------------------------------------------------------------------------------------
def test_mixed_batch(dev_factory):
    flows, L, lsn, warm, frames = C.mixed_batch()
    d = dev_factory(flows, L, lsn)
    d.process(warm, C.NOW - 10)
    link = (np.arange(len(frames)) % 3).astype(np.uint32)  # 2 is out of range: the listener's link
    got, exp = d.process(frames, link=link, slot_stride=80, frame_lead=6, flags=0)
    assert set(int(a) for a in exp["action"]) == set(range(9)) and exp["n_ready"] >= 8
    # odd placement and the offload flag
    d2 = dev_factory(flows, L, lsn)
    d2.process(warm, C.NOW - 10)
    d2.process(frames, slot_stride=67, frame_lead=1, flags=N.DK_TX_OFFLOAD_TCP)


def test_scan_tile_boundary_and_rank_tiles(dev_factory):
    """A batch a few frames over the rank pass's tile (1,024 frames) and over the scan's tile, candidates of two
    listeners on both sides of the boundaries, room running out beyond the first tile."""
    n = 2 * 1024 + 9
    flows, L, lsn = C.server([80, 81], max_backlog=[600, 300], isn_counter=[0xFF00, 3])
    d = dev_factory(flows, L, lsn, cap=2048)
    fr = []
    for i in range(n):
        k = i // 2 if i % 5 else i // 3  # repeats: later SYNs of a key are handshake segments
        fr.append(C.seg(C.remote(k), 80 + (k & 1), R.SYN if i % 7 else R.ACK, seq=i))
    got, exp = d.process(fr)
    acc = np.nonzero(exp["action"] == TL.SYN_ACCEPTED)[0]
    assert acc.min() < 1024 < acc.max() and (exp["action"] == TL.RST_BACKLOG).any()
    assert 300 < int(d.model.listeners["inflight"][0]) < 600 and int(d.model.listeners["inflight"][1]) == 300
    assert int(d.model.listeners["isn_counter"][0]) < 0xFF00  # the counter crossed 0xFFFF inside the batch


# ---- the backlog ------------------------------------------------------------------------------------------------------------
def test_backlog_room(dev_factory):
    flows, L, lsn = C.server([80, 81, 82], max_backlog=[2, 1, 3], inflight=[2, 0, 0])  # room 0, 1, 3
    d = dev_factory(flows, L, lsn, cap=64)
    fr = [C.seg(C.remote(0), 80, R.SYN), C.seg(C.remote(1), 81, R.SYN), C.seg(C.remote(2), 81, R.SYN),
          C.seg(C.remote(3), 82, R.SYN), C.seg(C.remote(4), 82, R.SYN), C.seg(C.remote(3), 82, R.SYN),
          C.seg(C.remote(5), 82, R.SYN), C.seg(C.remote(6), 82, R.SYN), C.seg(C.remote(6), 82, R.SYN),
          C.seg(C.remote(4), 82, R.ACK, ack=5), C.seg(C.remote(2), 81, R.SYN)]
    got, exp = d.process(fr)
    T = TL
    assert list(exp["action"]) == [T.RST_BACKLOG, T.SYN_ACCEPTED, T.RST_BACKLOG, T.SYN_ACCEPTED, T.SYN_ACCEPTED, T.BAD_ACK,
                                   T.SYN_ACCEPTED, T.RST_BACKLOG, T.RST_BACKLOG, T.BAD_ACK, T.RST_BACKLOG]
    assert [int(x) for x in d.model.listeners["inflight"]] == [2, 1, 3]


# ---- the ISN ------------------------------------------------------------------------------------------------------------------
def test_isn_counter_and_crc_wrap(dev_factory):
    flows, L, lsn = C.server([80], max_backlog=16, isn_counter=0xFFFD, nonce=0xDEADBEEF)
    big = C.find_remote_with_big_crc(L[0])
    d = dev_factory(flows, L, lsn, cap=64)
    fr = [C.seg(C.remote(k), 80, R.SYN, seq=k) for k in range(3)] + [C.seg(big, 80, R.SYN)] + \
         [C.seg(C.remote(k), 80, R.SYN, seq=k) for k in range(3, 6)]
    got, exp = d.process(fr)
    assert (exp["action"] == TL.SYN_ACCEPTED).all() and int(d.model.listeners[0]["isn_counter"]) == 4
    e = d.model.conns[TL.key(0, *big)]
    crc = R.crc32_cksum(R.isn_bytes(L[0], *big))
    assert crc > 0xFFFF0000 and e["local_isn"] == crc  # the fourth SYN: the counter has wrapped to 0
    assert d.model.conns[TL.key(0, *C.remote(2))]["local_isn"] == (R.crc32_cksum(R.isn_bytes(L[0], *C.remote(2))) + 0xFFFF) & R.M32
    d2 = dev_factory(flows, TL.listener_table(1, **{k: L[k] for k in ("flow_id", "local_ip", "local_port", "nonce")},
                                              max_backlog=4, isn_counter=0xFFFF), lsn, cap=64)
    d2.process([C.seg(big, 80, R.SYN)])
    assert d2.model.conns[TL.key(0, *big)]["local_isn"] < 0xFFFF  # crc + 0xFFFF wrapped 2^32


# ---- the table ----------------------------------------------------------------------------------------------------------------
def test_table_collisions_wrap_tombstones(dev_factory):
    cap = 64
    flows, L, lsn = C.server([80], max_backlog=32)
    homes = [5, 62, 63]  # chains from 62 and 63 run across the wrap-around
    rem = C.colliding_remotes(cap, 0, homes, 9)
    d = dev_factory(flows, L, lsn, cap=cap)
    first = [r for h in homes for r in rem[h][:8]]  # 24 keys on three home slots, concurrently inserted
    d.process([C.seg(r, 80, R.SYN, seq=j) for j, r in enumerate(first)])
    assert len(d.table.as_map()) == 24 and d.table.consumed() == 24
    # every key is found again: their handshake ACKs are wrong on purpose for half of them
    d.process([C.seg(r, 80, R.ACK, ack=(d.model.conns[TL.key(0, *r)]["local_isn"] + 1 + (j & 1)))
               for j, r in enumerate(first)])
    # release the head of each chain and an absent key; lookups behind them walk across the tombstones
    heads = [TL.key(0, *rem[h][0]) for h in homes]
    absent = TL.key(0, *C.remote(77))
    found = d.release(heads + [absent])
    assert [int(x) for x in found] == [1, 1, 1, 0] and int(d.model.listeners[0]["inflight"]) == 21
    d.process([C.seg(rem[h][7], 80, R.ACK | R.PSH, payload=b"x") for h in homes])  # FORWARD / ORPHANED across tombstones
    # re-insert a released key, and a ninth colliding key: tombstones are claimed, nothing new is consumed
    d.process([C.seg(rem[homes[0]][0], 80, R.SYN, seq=9), C.seg(rem[homes[1]][8], 80, R.SYN, seq=10)])
    assert d.table.consumed() == 24 and len(d.table.as_map()) == 23
    assert not d.release([absent])[0]
    # the rows copied out and in again: the same table, the consumed count recounted from them
    rows = d.table.rows()
    d.table.write(rows)
    d.compare_state()
    assert d.table.rows().tobytes() == rows.tobytes()
    d.process([C.seg(rem[homes[2]][3], 80, R.ACK)])  # still found


def test_backlog_rule_and_arguments(dev_factory):
    flows, L, lsn = C.server([80, 81], max_backlog=[16, 17])  # 2 x 33 > 64
    d = dev_factory(flows, L, lsn, cap=64)
    with pytest.raises(Fail) as e:
        d.process([C.seg(C.remote(0), 80, R.SYN)], compare=False)
    assert e.value.errno == errno.EINVAL
    d.backlog_sum = 32  # a host that states a wrong sum: the device adds the rows up itself
    got, exp = d.process([C.seg(C.remote(0), 80, R.SYN)])
    assert list(got["status"]) == [TL.E_TABLE] * 2 and got["action"][0] == TL.SKIP and got["n_frames"] == 0


def test_listener_checks_and_closed(dev_factory):
    flows, L, lsn = C.server([80, 81, 82, 83], window_scale=[15, 0, 0, 0], link=[0, 9, 0, 0],
                             state=[1, 1, N.DK_TCP_LSN_CLOSED, 1])
    d = dev_factory(flows, L, lsn, cap=64)
    got, exp = d.process([C.seg(C.remote(k), 80 + k % 4, R.SYN) for k in range(8)])
    assert list(exp["status"]) == [TL.E_WSCALE, TL.E_LINK, TL.OK, TL.OK]
    assert list(exp["action"]) == [0, 0, 0, TL.SYN_ACCEPTED] * 2
    got, exp = d.process([C.seg(C.remote(9), 83, R.SYN)], slot_stride=61)
    assert list(exp["status"])[3] == TL.E_SLOT and got["n_frames"] == 0


# ---- capacity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["max_frames", "out_bytes", "max_ready"])
def test_capacity_one_short(dev_factory, short):
    flows, L, lsn, warm, frames = C.mixed_batch()
    d = dev_factory(flows, L, lsn)
    d.process(warm, C.NOW - 10)
    probe = R.ListenModel(d.model.listeners, 1024)
    probe.conns = dict(d.model.conns)
    rows_before, l_before = d.table.rows().tobytes(), TL.listeners_to_host(d.d_L).tobytes()
    need = probe.process(C.oracle_rx(frames, flows), lsn, C.NOW, C.LINKS, slot_stride=64, max_frames=1 << 20,
                         out_bytes=1 << 30, max_ready=1 << 20)
    nf, nr = need["n_frames"], need["n_ready"]
    kw = dict(max_frames=nf, max_ready=nr, out_size=nf * 64 + 64, out_bytes=nf * 64)
    kw[short] -= 1
    got, exp = d.process(frames, **kw)
    assert not exp["fits"] and (got["n_frames"], got["n_ready"]) == (nf, nr) and set(got["status"]) == {TL.NO_ROOM}
    assert d.table.rows().tobytes() == rows_before and TL.listeners_to_host(d.d_L).tobytes() == l_before
    kw[short] += 1
    got, exp = d.process(frames, **kw)  # exactly enough room
    assert exp["fits"] and set(got["status"]) == {TL.OK}


# ---- timers -----------------------------------------------------------------------------------------------------------------
def test_timers(dev_factory):
    T0 = 1_000_000
    flows, L, lsn = C.server([80, 81], max_backlog=8, handshake_retries=[1, 0], handshake_timeout_ns=[1000, 1001])
    d = dev_factory(flows, L, lsn, cap=64)
    got, exp = d.process([C.seg(C.remote(0), 80, R.SYN, seq=5)], T0 - 1)        # deadline T0 + 999
    first = bytes(got["out"][:TL.SYNACK_BYTES])
    d.process([C.seg(C.remote(1), 80, R.SYN, seq=6)], T0)                       # deadline T0 + 1000
    d.process([C.seg(C.remote(2), 80, R.SYN, seq=7)], T0 + 1)                   # deadline T0 + 1001
    d.process([C.seg(C.remote(3), 81, R.SYN, seq=8)], T0 - 1)                   # deadline T0 + 1000, no retries
    d.process([C.seg(C.remote(4), 80, R.SYN), C.seg(C.remote(4), 80, R.ACK, ack=1)], T0 - 500)  # FAILED: no timer
    now = T0 + 1000  # deadlines at now - 1, now, now + 1
    got, exp, frames = d.timers(now)
    assert (exp["n_frames"], exp["n_ready"]) == (2, 1) and exp["ready"][0]["err"] == errno.ETIMEDOUT
    assert frames[TL.key(0, *C.remote(0))] == first  # the retried SYN+ACK equals the first byte for byte
    assert d.model.conns[TL.key(0, *C.remote(0))]["retries_left"] == 0
    assert d.model.conns[TL.key(0, *C.remote(2))]["retries_left"] == 1
    got, exp, _ = d.timers(now)  # nothing is due
    assert (exp["n_frames"], exp["n_ready"]) == (0, 0)
    got, exp, _ = d.timers(now + 1000, max_frames=1, max_ready=1)  # remote 2 resends, 0 and 1 time out: one short
    assert not exp["fits"] and (got["n_frames"], got["n_ready"]) == (1, 2) and got["status"][0] == TL.NO_ROOM
    got, exp, _ = d.timers(now + 1000, max_frames=1, max_ready=2, slot_stride=62, out_size=62)
    assert exp["fits"] and {int(r["err"]) for r in exp["ready"]} == {errno.ETIMEDOUT}
    # a timed-out entry swallows its remote's frames
    got, exp = d.process([C.seg(C.remote(0), 80, R.ACK, ack=1)], now + 2000)
    assert exp["action"][0] == TL.ORPHANED
