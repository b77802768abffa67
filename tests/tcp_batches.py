"""Crafted dk_tcp batches whose expected result can be stated in a few lines of numpy (no test in here: the builder's
own checks are tests/test_tcp_batches.py, its GPU users tests/test_gpu_tcp_order.py).

synth.tcp_streams spreads its segments evenly over the flows, so every sort key shows up in every tile in similar
numbers. crafted() takes the per-segment flow array as given, so a test decides which keys a tile holds (one key only,
three of 255, almost nothing but the "no connection" bucket, ...), and the streams it builds are so plain that what
dk_tcp_rx_process must answer follows from a stable sort by flow id: every segment of a live row is delivered in
arrival order, except the marked strays, which lie past the window end.
"""
import numpy as np

from demikernel_amd import _native as N
from oracle import oracle as O

ACK = 0x10
HDR, PAYLOAD = 54, 10  # payload offset (Ethernet + IPv4 + TCP, no options) and bytes of every segment
# Receive buffer of every row: below the key kernel's 0x40000000 bound on order-independent classification, and room
# for 400k ten-byte segments on one row (4 MB of stream) without the window filling.
BUFFER_SIZE = 1 << 26
STRAY_SHIFT = BUFFER_SIZE + 12345  # past the window end wherever RCV.NXT stands: OUT_OF_WINDOW, sort key 2c + 1
LAYOUTS = ("uniform", "last_row_only", "unowned_mostly", "row_per_tile", "zipf")
TILE = 8192  # tcp_kernels.hip kSortTile, for the row_per_tile layout


def crafted(f, rows: int, *, none_rows=(), stray=None):
    """(table, rx) for the per-segment flow ids `f` over a table of `rows` rows.

    Rows: ESTABLISHED, receive_next = reader_next = send_next = 1, buffer_size = BUFFER_SIZE; `none_rows` are
    DK_TCP_NONE. Segments: verdict OK_TCP, flags ACK, tcp_ack = 1, PAYLOAD bytes at HDR, tcp_seq = 1 + PAYLOAD * (the
    segment's rank among its flow id's non-stray segments, in arrival order), so each row's stream is in order and
    gap-free. A segment marked in the boolean `stray` sits STRAY_SHIFT past its place and takes no stream bytes. Flow
    ids >= rows (DK_FLOW_NONE among them) are passed through unchanged: no row owns them (sort key 2 rows)."""
    f = np.asarray(f, np.int64).astype(np.uint32)
    n = len(f)
    stray = np.zeros(n, bool) if stray is None else np.asarray(stray, bool)
    assert stray.shape == (n,)
    table = np.zeros(rows, O.TCP_CONN_DTYPE)
    table["state"] = N.DK_TCP_ESTABLISHED
    table["receive_next"] = table["reader_next"] = table["send_next"] = 1
    table["buffer_size"] = BUFFER_SIZE
    table["state"][list(none_rows)] = N.DK_TCP_NONE
    order = np.argsort(f, kind="stable")  # by flow id, arrival order within one
    fs, live = f[order], ~stray[order]
    before = np.cumsum(live) - live  # non-stray segments ahead in the sorted order
    first = np.ones(n, bool)
    first[1:] = fs[1:] != fs[:-1]
    rank = np.empty(n, np.int64)
    rank[order] = before - np.maximum.accumulate(np.where(first, before, 0))  # minus the count at its id's start
    assert n == 0 or int(rank.max()) * PAYLOAD + PAYLOAD < BUFFER_SIZE
    rx = {"meta": np.full(n, 6 << 8 | ACK << 16 | 0x50 << 24, np.uint32), "flow_id": f,
          "tcp_seq": (1 + PAYLOAD * rank + np.where(stray, STRAY_SHIFT, 0)).astype(np.uint32),
          "tcp_ack": np.ones(n, np.uint32), "payload": np.full(n, HDR | PAYLOAD << 16, np.uint32)}
    return table, rx


def layout(name: str, n: int, rows: int, seed: int = 0) -> np.ndarray:
    """Per-segment flow ids (int64[n]) of the named key layout."""
    rng = np.random.default_rng([seed, n, rows, LAYOUTS.index(name)])
    if name == "uniform":  # every key in every tile; a few segments (ids rows .. rows + 2) unowned
        return rng.integers(0, rows + 3, n)
    if name == "last_row_only":  # one key: every other key's range is empty
        return np.full(n, rows - 1, np.int64)
    if name == "unowned_mostly":  # the top bucket 2 rows holds 99 %
        return np.where(rng.random(n) < 0.99, N.DK_FLOW_NONE, rng.integers(0, rows, n))
    if name == "row_per_tile":  # three rows per tile, other rows from tile to tile: counts isolated among zeros
        i = np.arange(n)
        return ((i // TILE) * 11 + i % 3) % rows
    if name == "zipf":  # heavy head, long tail
        return np.minimum(rng.zipf(1.3, n) - 1, rows - 1)
    raise KeyError(name)


def strays(n: int, fraction: float = 0.05, seed: int = 0) -> np.ndarray:
    return np.random.default_rng([seed, n, 977]).random(n) < fraction


def case(name: str, n: int, rows: int, none_rows=(7, 100), seed: int = 0):
    """(table, rx, f, stray) of the named layout with 5 % strays; the rows of `none_rows` the table has are NONE."""
    f = layout(name, n, rows, seed)
    stray = strays(n, 0.05, seed)
    table, rx = crafted(f, rows, none_rows=[r for r in none_rows if r < rows], stray=stray)
    return table, rx, f, stray


def promised(table: np.ndarray, f, stray) -> dict:
    """What crafted() promises of its batch, stated without the oracle: per-segment actions, each row's delivered
    views in order (a stable sort by flow id of the delivered segments' indices) and its RCV.NXT afterwards."""
    f, rows = np.asarray(f, np.int64), len(table)
    owned = f < rows
    owned[owned] = table["state"][f[owned]] != N.DK_TCP_NONE
    delivered = owned & ~np.asarray(stray, bool)
    action = np.full(len(f), N.A["SKIP"], np.uint8)
    action[owned] = N.A["OUT_OF_WINDOW"]
    action[delivered] = N.A["DELIVERED"]
    idx = np.nonzero(delivered)[0]
    idx = idx[np.argsort(f[idx], kind="stable")]
    count = np.bincount(f[idx], minlength=rows)[:rows]
    return {"action": action, "deliv_idx": np.split(idx, np.cumsum(count)[:-1]), "deliv_count": count,
            "receive_next": (1 + PAYLOAD * count).astype(np.uint32)}


def stream_rx(tr) -> dict:
    """The dk_rx result arrays of a synth.tcp_streams Traffic whose frames are all well-formed TCP."""
    return {"meta": (6 << 8 | tr.flags.astype(np.uint32) << 16 | 0x50 << 24).astype(np.uint32),
            "flow_id": tr.flow.astype(np.uint32), "tcp_seq": tr.seq, "tcp_ack": tr.ack,
            "payload": (54 | (tr.ip_len.astype(np.uint32) - 40) << 16).astype(np.uint32)}
