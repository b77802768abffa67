"""The crafted-batch builder (tests/tcp_batches.py) against the TCP oracle, on the CPU: for every key layout the GPU
ordering tests use (tests/test_gpu_tcp_order.py), at their 25-tile size, the oracle answers exactly what the builder
promises, stated here as a stable sort by flow id in numpy; and an arrival order changed in one place changes the
oracle's answer, so a bit-exact comparison with it notices an unstable or misplaced sort."""
import numpy as np
import pytest

import tcp_batches as B
from demikernel_amd import _native as N
from oracle import oracle as O

ROWS = 255
NSEG = 24 * 8192 + 777  # 25 tiles of 8,192 segments


@pytest.fixture(scope="module", params=B.LAYOUTS)
def built(request):
    """One layout's batch, the oracle's answer on it and the table afterwards; shared, never written to."""
    table, rx, f, stray = B.case(request.param, NSEG, ROWS)
    after = table.copy()
    out = O.tcp_process(after, rx)
    return table, rx, f, stray, after, out


def test_builder_keeps_its_promises(built):
    table, rx, f, stray, _, _ = built
    assert (table["state"][[7, 100]] == N.DK_TCP_NONE).all() and (table["state"] == N.DK_TCP_ESTABLISHED).sum() == 253
    for k in ("receive_next", "reader_next", "send_next"):
        assert (table[k] == 1).all()
    assert (table["buffer_size"] == 1 << 26).all()
    assert np.array_equal(rx["flow_id"], np.asarray(f, np.int64).astype(np.uint32))  # ids >= rows unchanged
    assert (rx["meta"] == (6 << 8 | B.ACK << 16 | 0x50 << 24)).all() and (rx["tcp_ack"] == 1).all()
    assert (rx["payload"] == (54 | 10 << 16)).all()
    for c in (0, 7, 254, ROWS + 1, N.DK_FLOW_NONE):  # a live row, a NONE row, the last row, unowned ids
        at = np.nonzero(f == c)[0]
        live = ~stray[at]
        rank = np.cumsum(live) - live
        assert np.array_equal(rx["tcp_seq"][at], 1 + 10 * rank + np.where(live, 0, (1 << 26) + 12345)), c
    assert 0.04 < stray.mean() < 0.06


def test_oracle_agrees_with_numpy_statement(built):
    table, rx, f, stray, after, out = built
    want = B.promised(table, f, stray)
    assert np.array_equal(out["action"], want["action"])
    n = len(f)
    assert np.array_equal(out["view"]["ref"], np.arange(n)) and (out["view"]["off"] == 54).all()
    assert (out["view"]["len"] == 10).all()
    assert np.array_equal(out["deliv_count"], want["deliv_count"])
    assert np.array_equal(after["receive_next"], want["receive_next"])
    for c in range(ROWS):
        s, idx = int(out["deliv_start"][c]), want["deliv_idx"][c]
        d = out["deliv"][s:s + len(idx)]
        assert np.array_equal(d["ref"], idx) and (d["off"] == 54).all() and (d["len"] == 10).all(), c
    # nothing else of the table moves: in-order streams leave no out-of-order store and no row closes
    rest = after.copy()
    rest["receive_next"] = table["receive_next"]
    assert np.array_equal(rest.view(np.uint8), table.view(np.uint8))
    hist = np.bincount(out["action"], minlength=len(N.TCP_ACTIONS))
    for a in ("DELIVERED", "OUT_OF_WINDOW"):
        assert hist[N.A[a]] > 0, (a, hist)
    assert hist[N.A["SKIP"]] > 0 or (np.asarray(f) == ROWS - 1).all()  # last_row_only: every segment owned


def differing(a: dict, b: dict) -> int:
    return int((a["action"] != b["action"]).sum() + (a["deliv"] != b["deliv"]).sum() +
               (a["deliv_count"] != b["deliv_count"]).sum())


def exchanged(rx: dict, i: int, j: int) -> dict:
    """The batch with the segments at arrival places i and j exchanged."""
    rx = {k: v.copy() for k, v in rx.items()}
    for v in rx.values():
        v[[i, j]] = v[[j, i]]
    return rx


def test_oracle_notices_a_changed_order(built):
    """Two consecutive non-stray segments of one connection exchanged (what an unstable sort would hand the walk), then
    a segment put among another connection's (a misplaced one): the actions or the deliveries differ."""
    table, rx, f, stray, _, out = built
    want = B.promised(table, f, stray)
    c = int(np.argmax(want["deliv_count"]))
    idx = want["deliv_idx"][c]
    i, j = int(idx[len(idx) // 2]), int(idx[len(idx) // 2 + 1])
    swapped = O.tcp_process(table.copy(), exchanged(rx, i, j))
    assert differing(swapped, out) > 0
    # into another connection's place: the segment handed to the next live row's walk
    c2 = next(r % ROWS for r in range(c + 1, c + ROWS) if table["state"][r % ROWS] == N.DK_TCP_ESTABLISHED)
    moved = {k: v.copy() for k, v in rx.items()}
    moved["flow_id"][i] = c2
    assert differing(O.tcp_process(table.copy(), moved), out) > 0
