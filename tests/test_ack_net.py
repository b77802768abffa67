"""tests/ack_net.py on the CPU: the all-host run of every case finishes inside CALL_CAP and passes T1-T6, the cases
recorded what they were built for (the GPU tests replay the same recordings, so they inherit it), the numpy
append_frames restates UnackedQueue.append_frames's arithmetic on a hand-made queue, and AckChecker rejects deliberately
wrong ACK processors: tcp_ack_reference with one rule broken, run on a recorded call's inputs."""
import contextlib

import numpy as np
import pytest

import ack_net as AN
import tcp_ack_reference as R
from demikernel_amd import _native as N

NAMES = list(AN.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_host_run_finishes_and_passes_the_checker(name):
    tr = AN.trace(name)
    assert tr.done and len(tr.calls) <= AN.CALL_CAP, (tr.done, len(tr.calls))
    chk = AN.check_trace(tr)
    chk.finish(tr.final["tx"], tr.final["ak"], tr.peer_got, tr.peer_fin)
    print(name, len(tr.rounds), "rounds", len(tr.calls), "calls", tr.stats, chk.seen)
    # what every case has to have recorded
    assert tr.stats["timer_rtx"] >= 1 and tr.stats["fast_rtx"] >= 1, tr.stats
    assert chk.seen["inside"] >= 1, "no ACK landed inside an entry"
    assert chk.seen["trimmed"] >= 1 and chk.seen["trimmed_again"] >= 1, "no ACK for an already trimmed entry"
    assert chk.seen["old"] >= 1 and chk.seen["dup"] >= 3 and chk.seen["samples"] >= 1, chk.seen
    if tr.case.fin_lost:
        assert tr.stats["fin_rtx"] >= tr.case.nconns, tr.stats
    status = np.concatenate([r.ack.exp["status"][:tr.case.nconns] for r in tr.calls])
    assert (status == R.OK).all()
    wrapped = (tr.final["tx"]["snd_una"] < tr.isn)[:tr.case.nconns]
    assert wrapped[::3].all(), "every third connection's SND.UNA goes through 2^32"
    assert len({int(w) for w in tr.ak0["snd_wscale"]}) == min(len(tr.ak0), int(tr.ak0["snd_wscale"].max()) + 1)


def test_shapes_the_cases_were_built_for():
    """dk_tcp_ack_process's rule (tcp_ack_kernels.hip): the chip form from 1,024 frames per table row, one wave per
    connection from 8, one lane below. one_long has calls of the chip form's shape, a later one larger than every one
    before it (the scratch grows); few has the wave form's; many and wide_300 stay below 8 frames per row; wide_300
    has 301 rows (the radix sort)."""
    one = [len(r.ack.off) for r in AN.trace("one_long").calls]
    chip = [n for n in one if n >= 1024]
    assert len(chip) >= 2 and any(n // 64 > max(chip[:k]) // 64 for k, n in enumerate(chip) if k), one
    assert min(one) < 8
    few = [len(r.ack.off) for r in AN.trace("few").calls]
    assert sum(8 * 7 <= n < 1024 * 7 for n in few) >= 10, few
    assert all(len(r.ack.off) < 8 * 40 for r in AN.trace("many").calls)
    wide = AN.trace("wide_300")
    assert len(wide.tx0) == 301 and all(len(r.ack.off) < 8 * 301 for r in wide.calls)
    for name in ("few", "piggy"):  # B's own data: A's receive side delivers, stores and sees duplicates
        seen = np.zeros(16, np.int64)
        for r in AN.trace(name).calls:
            seen += np.bincount(r.ack.rx_out["action"], minlength=16)
        assert all(seen[N.A[k]] for k in ("DELIVERED", "STORED", "DUPLICATE", "ACK_UNSENT")), (name, seen)
    total = sum(len(r.ack.off) for name in NAMES for r in AN.trace(name).calls)
    assert total <= 40_000, total


def test_append_frames_by_hand():
    """Two connections, capacity 4: connection 0 has two live entries at 2 and 3, connection 1 none. Two frames of
    connection 0's one buffer and a FIN of connection 1 are appended at time 77."""
    ak = AN.ack_conn_table(2, q_first=[2, 4], q_count=[2, 0])
    ak["rtx_armed"][0], ak["rtx_base_ns"][0] = 1, 5
    pool = {"off": np.arange(8, dtype=np.uint32) + 100, "len": np.arange(8, dtype=np.uint32) + 10,
            "tx_time": np.arange(8, dtype=np.uint64) + 1000}
    push = (np.array([0, 1]), np.array([500, 900]), np.array([15, 0]))
    seg = dict(frame_buf=np.array([0, 0, 1]), len_out=np.array([54 + 10, 54 + 5, 54]), first_frame=np.array([0, 2]))
    conn, off, ln = AN.sent_entries(push, seg)
    assert (list(conn), list(off), list(ln)) == ([0, 0, 1], [500, 510, 900], [10, 5, 0])
    AN.append_frames(ak, pool, 4, conn, off, ln, 77)
    assert list(pool["off"]) == [102, 103, 500, 510, 900, 0, 0, 0] and list(pool["len"]) == [12, 13, 10, 5, 0, 0, 0, 0]
    assert list(pool["tx_time"]) == [1002, 1003, 77, 77, 77, 0, 0, 0]
    assert list(ak["q_first"]) == [0, 4] and list(ak["q_count"]) == [4, 1]
    assert list(ak["rtx_armed"]) == [1, 1] and list(ak["rtx_base_ns"]) == [5, 77]  # an armed timer is left alone
    with pytest.raises(AssertionError, match="capacity"):
        AN.append_frames(ak, pool, 4, np.array([0]), np.array([0]), np.array([1]), 78)


# ---- the checker has teeth -------------------------------------------------------------------------------------------
class Wrong(R.Sender):
    """Sender.process_ack (tcp_ack_reference.py) with one rule broken, named by `kind`."""
    kind = ""

    def process_ack(self, seq, ack, win, now):
        k = self.kind
        nbytes = (ack - self.una) & R.M32
        if ack == self.una:
            self.dup_acks += 1
        new = R.seq_lt(self.una, ack)
        if new and nbytes == 0x80000000 and self.una == self.nxt:
            new = False
        if k == "window_from_any_ack" and not new and self.wl1 == seq and R.seq_le(self.wl2, ack):
            self.wnd = (win << self.wscale) & R.M32
        if not new:
            return nbytes
        self.new_acks += 1
        remaining = nbytes
        while remaining != 0:
            if not self.queue:
                if k == "unsent_ack_processed":
                    break  # (a processor that takes such an ACK does not miss the bytes either)
                raise R.Dry()
            e = self.queue.popleft()
            self.popped += 1
            if e[2] != R.NONE or k == "sample_from_none":
                self.rto.add_sample_ns(max(now - e[2], 0) if e[2] != R.NONE else 0)
                self.samples += 1
            if e[1] > remaining:
                e[0], e[1] = (e[0] + remaining) & R.M32, e[1] - remaining
                if k != "trim_keeps_time":
                    e[2] = R.NONE
                self.queue.appendleft(e)
                self.popped -= 1
                break
            if e[1] == 0:
                remaining = 0
                if k == "marker_stays":
                    self.queue.appendleft(e)
                    self.popped -= 1
            remaining -= e[1]
        self.una = ack
        if R.seq_lt(self.wl1, seq) or (self.wl1 == seq and R.seq_le(self.wl2, ack)):
            self.wnd = (win << self.wscale) & R.M32
            self.wl1, self.wl2 = seq, ack
        if k == "stale_base":
            self.armed = int(bool(self.queue))
        elif self.queue:
            self.armed, self.base = 1, (self.queue[0][2] if self.queue[0][2] != R.NONE else now)
        else:
            self.armed, self.base = 0, 0
        if k == "q_first_stays":
            self.popped = 0
        if k == "rto_without_sample":
            self.rto.rto = AN.clamp_rto(self.rto.srtt, self.rto.rttvar)
        return nbytes


@contextlib.contextmanager
def wrong_processor(kind: str):
    sender, processed = R.Sender, R.PROCESSED
    try:
        R.Sender = type("Wrong_" + kind, (Wrong,), {"kind": kind})
        if kind == "unsent_ack_processed":
            R.PROCESSED = processed + (N.A["ACK_UNSENT"],)
        yield
    finally:
        R.Sender, R.PROCESSED = sender, processed


MUTANTS = {  # kind -> (the case that has what it needs, the rule that must catch it)
    "sample_from_none": ("fin_lost", "T4"),
    "trim_keeps_time": ("fin_lost", "T4"),
    "q_first_stays": ("fin_lost", "T2"),
    "window_from_any_ack": ("many", "T1: the window"),
    "marker_stays": ("fin_lost", "T2"),
    "stale_base": ("fin_lost", "T5: timer"),
    "rto_without_sample": ("fin_lost", "T5: the RTO state changed without a sample"),
    "unsent_ack_processed": ("piggy", "T1|T3: acked set on a frame that was not ACK-processed"),
}


@pytest.mark.parametrize("kind", list(MUTANTS))
def test_checker_rejects_a_wrong_processor(kind):
    """The recorded calls are fed unchanged up to the first one on which the wrong processor, started from that call's
    recorded state and inputs, gives another result than the reference; the checker must reject that result by the
    rule named."""
    name, rule = MUTANTS[kind]
    tr = AN.trace(name)
    chk = AN.AckChecker(tr)
    for r in tr.rounds:
        chk.host(r)
        a = r.ack
        if a is None:
            continue
        e, s = a.exp, a.start
        with wrong_processor(kind):
            try:
                w = R.ack_process(a.h["flow_id"], a.rx_out["action"], a.h["tcp_seq"], a.h["tcp_ack"], a.h["tcp_win"],
                                  a.rx_after, s["tx"], s["ak"], s["pool"], a.now)
            except Exception as exc:  # a wrong processor may also fall over: that is no rejection by the checker
                raise AssertionError(f"{kind} raised {exc!r} instead of returning a wrong result")
        same = all(np.array_equal(w[k], e[k]) for k in e if k != "pool") and \
            all(np.array_equal(w["pool"][k], e["pool"][k]) for k in e["pool"])
        if same:
            chk.feed(a, a.rx_out["action"], e, e["tx_conns"], e["ack_conns"], e["pool"])
            continue
        with pytest.raises(AssertionError, match=rule):
            chk.feed(a, a.rx_out["action"], w, w["tx_conns"], w["ack_conns"], w["pool"])
        return
    raise AssertionError(f"no call of {name} has what {kind} needs")


def test_checker_rejects_an_unfinished_transfer():
    tr = AN.trace("fin_lost")
    chk = AN.AckChecker(tr)
    last = None
    for r in tr.rounds[:-3]:
        chk.host(r)
        if r.ack is not None:
            e = last = r.ack.exp
            chk.feed(r.ack, r.ack.rx_out["action"], e, e["tx_conns"], e["ack_conns"], e["pool"])
    with pytest.raises(AssertionError, match="T6"):
        chk.finish(last["tx_conns"], last["ack_conns"], tr.peer_got, tr.peer_fin)
    chk = AN.check_trace(tr)
    with pytest.raises(AssertionError, match="T6"):
        chk.finish(tr.final["tx"], tr.final["ak"], tr.peer_got, tr.peer_fin, cap=len(tr.calls) - 1)
