"""tests/stream_net.py on the CPU: StreamChecker raises on every hand-made corruption of a valid result, the oracle
chain (OraclePeer.process on the real frames, then tcp_process, the handle rewrite between calls) passes S1-S5 on every
case, and the cases reach what they were built for (the guards, computed from the oracle's run, so the GPU tests that replay
the same traces inherit them)."""
import numpy as np
import pytest

import stream_net as SN
from demikernel_amd import _native as N

HOST_CASES = list(SN.CASES)  # (the device-sender case of test_gpu_tcp_streams.py needs the GPU to build its frames)


# ---- the checker has teeth -------------------------------------------------------------------------------------------
def slots(call, c):
    s = int(call.exp["deliv_start"][c])
    return np.arange(s, s + int(call.exp["deliv_count"][c]))


def corrupt(name, find, match):
    """The first call of case `name` for which find(call, out, table) corrupts the copies it is given (returns True);
    the checker, fed the calls before it unchanged, must raise on it."""
    tr = SN.trace(name)
    chk = SN.StreamChecker(tr.irs, tr.case.stream, tr.table0)
    for call in tr.calls:
        out, table = {k: v.copy() for k, v in call.exp.items()}, call.exp_table.copy()
        args = (call.blob, call.off, call.lens, call.gidx, call.pay_off, call.pay_len)
        if find(call, out, table):
            with pytest.raises(AssertionError, match=match):
                chk.feed(out, table, *args)
            return
        chk.feed(out, table, *args)
    raise AssertionError("no call of the case has what this corruption needs")


def data_runs(call, out, k=2, handle=False):
    """(connection, slots) of connections with >= k deliveries of >= 8 bytes in a row (the first a handle, if asked)."""
    for c in np.nonzero(out["deliv_count"] >= k)[0]:
        s = slots(call, c)
        d = out["deliv"][s]
        ok = (d["ref"] != SN.EOF) & (d["len"] >= 8)
        for j in range(len(s) - k + 1):
            if ok[j:j + k].all() and (not handle or d["ref"][j] >= SN.HANDLE):
                yield c, s[j:j + k]


def last_data(call, out):
    """(connection, slot) of connections whose last delivery of the call is data of >= 8 bytes."""
    for c, s in data_runs(call, out, 1):
        if s[-1] == slots(call, c)[-1]:
            yield c, s[-1]


def test_teeth_view_off_shifted():
    def f(call, out, table):
        for c, s in data_runs(call, out, 1):
            out["deliv"]["off"][s[0]] -= 1  # still inside the frame (its headers): only the bytes tell
            return True
    corrupt("many_reordered", f, "S1: view .* does not hold the stream")


def test_teeth_len_shortened():
    def f(call, out, table):
        for c, s in last_data(call, out):
            out["deliv"]["len"][s] -= 1
            return True
    corrupt("many_reordered", f, "S2: RCV.NXT - IRS")


def test_teeth_deliveries_swapped():
    def f(call, out, table):
        for c, s in data_runs(call, out, 2):
            out["deliv"][s] = out["deliv"][s[::-1]]
            return True
    corrupt("many_reordered", f, "S1: view .* does not hold the stream")


def test_teeth_delivery_dropped():
    def f(call, out, table):
        for c, s in last_data(call, out):
            out["deliv_count"][c] -= 1
            return True
    corrupt("many_reordered", f, "S2: RCV.NXT - IRS")


def test_teeth_delivery_dropped_in_the_middle():
    def f(call, out, table):
        for c, s in data_runs(call, out, 2):
            allc = slots(call, c)
            keep = allc[allc != s[0]]
            out["deliv"][allc[:len(keep)]] = out["deliv"][keep]
            out["deliv_count"][c] -= 1
            return True
    corrupt("many_reordered", f, "S1: view .* does not hold the stream")


def test_teeth_ooo_start_off_by_one():
    def f(call, out, table):
        c = np.nonzero((table["ooo_count"] > 0) & (table["ooo"]["len"][:, 0] >= 8))[0]
        if len(c):
            table["ooo_start"][c[0], 0] += 1
            return True
    corrupt("many_reordered", f, "S3: view .* does not hold the stream")


def test_teeth_receive_next_off_by_one():
    def f(call, out, table):
        if not call.lossy:
            table["receive_next"][3] += 1
            return True
    corrupt("many_reordered", f, "S2: RCV.NXT - IRS")


def test_teeth_receive_next_backwards():
    def f(call, out, table):
        if not call.lossy:
            table["receive_next"][3] -= 1
            return True
    corrupt("many_reordered", f, "S2: RCV.NXT moved backwards")


def test_teeth_handle_taken_as_batch_index():
    def f(call, out, table):
        for c, s in data_runs(call, out, 1, handle=True):
            out["deliv"]["ref"][s[0]] &= ~np.uint32(SN.HANDLE)
            return True
    corrupt("many_reordered", f, "S1")


def test_teeth_view_outside_payload():
    def f(call, out, table):
        i = np.nonzero(out["action"] == N.A["DELIVERED"])[0]
        if len(i):
            out["view"]["off"][i[0]] -= 1  # S4 alone sees it: the delivery list is untouched
            return True
    corrupt("many_reordered", f, "S4")


def test_teeth_unfinished_stream():
    tr = SN.trace("tiny_window")
    chk = SN.StreamChecker(tr.irs, tr.case.stream, tr.table0)
    for call in tr.calls[:-1]:
        chk.feed(call.exp, call.exp_table, call.blob, call.off, call.lens, call.gidx, call.pay_off, call.pay_len)
    with pytest.raises(AssertionError, match="S5"):
        chk.finish(tr.calls[-2].exp_table, tr.final_snd_nxt, tr.exempt)


# ---- the oracle chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HOST_CASES)
def test_oracle_chain_delivers_the_streams(name):
    tr = SN.trace(name)
    assert tr.done and len(tr.calls) <= SN.CALL_CAP, (tr.done, len(tr.calls))
    chk = SN.check_trace(tr)
    chk.finish(tr.final_table, tr.final_snd_nxt, tr.exempt)
    if tr.case.strays:  # the resets landed mid-stream, and the rows that are no open connection were left alone
        for c in SN.RESET_AT:
            assert tr.final_table["state"][c] == N.DK_TCP_CLOSED and 0 < chk.delivered[c] < tr.case.stream
        rest = slice(tr.case.nconns, None)
        assert tr.final_table[rest].tobytes() == tr.table0[rest].tobytes()


def test_every_frame_layout_is_built():
    """Payload offsets 54 (no options), 66 (TCP timestamps), 58 and 94 (IPv4 options, IHL 6 and 15), frames padded to
    60 bytes, blob slots at 0 and 2 mod 16 — and the receive chain takes every one of them as a good TCP segment."""
    tr = SN.trace("few_windowed")
    offs, padded, slots16 = set(), 0, set()
    for call in tr.calls:
        offs |= set(np.unique(call.pay_off).tolist())
        padded += int(((call.lens == 60) & (call.pay_off + call.pay_len < 60)).sum())
        slots16 |= set(np.unique(call.off % 16).tolist())
        assert (call.exp["action"] != N.A["SKIP"]).all()
    assert offs == {54, 58, 66, 94} and slots16 == {0, 2}
    assert padded or any(((c.lens == 60) & (c.pay_off + c.pay_len < 60)).any() for c in SN.trace("tiny_window").calls)


def test_duplicates_are_repeated_descriptors():
    tr = SN.trace("many_reordered")
    call = tr.calls[0]
    pairs = np.stack([call.off, call.lens.astype(np.uint32)], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs) and len(np.unique(call.gidx)) == len(np.unique(pairs, axis=0))


# ---- coverage guards -------------------------------------------------------------------------------------------------
def test_guards():
    total = dict(store=0, stale=0, fin_pending=0, unread=0, zero_window=0, segments=0, wrapped=0)
    actions = np.zeros(len(N.TCP_ACTIONS), np.int64)
    via_handle = 0
    for name in HOST_CASES:
        tr = SN.trace(name)
        g = SN.guards(tr)
        print(name, {k: v for k, v in g.items() if k != "actions"})
        assert g["calls"] <= SN.CALL_CAP and tr.done
        for k in total:
            total[k] += g[k]
        actions += g["actions"]
        via_handle += SN.check_trace(tr).via_handle
    print("matrix", total, dict(zip(N.TCP_ACTIONS, actions.tolist())), "deliveries through a handle", via_handle)
    for k in ("store", "stale", "fin_pending", "unread"):
        assert total[k] >= 10, (k, total)
    assert total["zero_window"] >= 1 and total["wrapped"] >= 1 and via_handle >= 1
    assert (actions > 0).all(), dict(zip(N.TCP_ACTIONS, actions.tolist()))  # STORE_DUP among them
    assert total["segments"] <= 100_000


def test_shapes_the_cases_were_built_for():
    """one_long reaches the scan walk's envelope (>= 1,024 segments of one connection in a call) and calls below the
    wave walk's (< 8); the wide cases stay under 8 segments per connection; the window end binds in few_windowed; the
    store fills in many_reordered; the stalled reader of tiny_window sees a zero window."""
    n = [len(c.off) for c in SN.trace("one_long").calls]
    assert max(n) >= 1024 and min(n) < 1024
    for name in ("wide_254", "wide_300"):
        tr = SN.trace(name)
        assert all(len(c.off) < 8 * len(tr.table0) for c in tr.calls)
    assert len(SN.trace("wide_254").table0) == 255 and len(SN.trace("wide_300").table0) == 301
    g = SN.guards(SN.trace("few_windowed"))
    assert g["actions"][N.A["OUT_OF_WINDOW"]] > 0
    assert max(int(c.exp_table["ooo_count"].max()) for c in SN.trace("many_reordered").calls) == SN.OOO_MAX
    assert SN.guards(SN.trace("tiny_window"))["zero_window"] >= 1
