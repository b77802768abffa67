"""GPU parity of dk_tcp_rx_process's ordering stage (tcp_kernels.hip: dk_tcp_sort_count_kernel, dk_tcp_sort_scan_kernel,
dk_tcp_sort_scatter_kernel, and the rule that picks the sort and the walk) with the CPU restatement
(oracle/dk_tcp_oracle.cpp), on batches whose key layout the test decides (tests/tcp_batches.py): the scan's second and
third loop iteration (its carried total, its reuse of LDS, ranges written from a later iteration), tiles of one key,
count tables that are nearly all zeros, a crowded "no connection" bucket, crowded classified keys 2c + 1, and the sizes
and row counts at which the code takes another path.

Every case compares the actions, the views, deliv_start, deliv_count, the used deliv slots and the whole connection
table bit for bit, once under the engine's rule and once with the radix sort forced, each with a fresh context, and
asserts which sort ran (dk_diag_tcp_last_sort). What a changed order does to these outputs is shown on the CPU
(tests/test_tcp_batches.py::test_oracle_notices_a_changed_order)."""
import functools

import numpy as np
import pytest

import tcp_batches as B
from demikernel_amd import synth
from demikernel_amd.tcp import TcpReceiver
from oracle import oracle as O
from test_gpu_tcp import assert_same, gpu_process, rx_device

pytestmark = pytest.mark.gpu

SORT_TILE = 8192          # tcp_kernels.hip kSortTile: segments per tile of the counting pass
SCAN_ITERATION = 12288    # kSortScanBlock * kSortScanPer: entries dk_tcp_sort_scan_kernel scans per loop iteration
SORT_MAX_ROWS = 255       # kSortMaxRows: the counting pass up to here, the radix sort above


def scan_entries(n: int, rows: int) -> int:
    """Entries of the count table H the scan kernel goes over: one per key (2 rows + 1) and tile."""
    return (2 * rows + 1) * -(-n // SORT_TILE)


def scan_iterations(n: int, rows: int) -> int:
    return -(-scan_entries(n, rows) // SCAN_ITERATION)


@functools.lru_cache(maxsize=2)
def crafted_case(name: str, n: int, rows: int, none_rows=(7, 100)):
    """A crafted batch and the oracle's answer, computed once per case and left unchanged."""
    table, rx, _, _ = B.case(name, n, rows, none_rows)
    exp_t = table.copy()
    exp = O.tcp_process(exp_t, rx)
    return table, rx, exp_t, exp


def both_sorts(table, rx, exp_t, exp, ctx, *, walk=None, want_walk=None):
    """The batch through a fresh context under the rule and through one with the radix sort forced: outputs exact,
    the sort that ran as the rule says, and the walk where the case states one."""
    r = rx_device(rx)
    rule = "counting" if 0 < len(table) <= SORT_MAX_ROWS and len(rx["meta"]) else "radix"
    for radix in (False, True):
        tcp = TcpReceiver(0, walk=walk, radix_sort=radix)
        assert tcp.last_sort is None and tcp.last_walk is None
        got_t, got = gpu_process(tcp, table.copy(), r)
        sort, ran = tcp.last_sort, tcp.last_walk
        tcp.close()
        assert sort == ("radix" if radix else rule), (ctx, radix, sort)
        if want_walk is not None:
            assert ran == want_walk, (ctx, radix, ran)
        assert_same(got_t, got, exp_t, exp, f"{ctx} radix {radix} ({ran} walk)")


# ---- B1: the scan's loop iterations at 255 rows (511 keys) ---------------------------------------------------------


@pytest.mark.parametrize("name", B.LAYOUTS)
@pytest.mark.parametrize("tiles,iterations", [(24, 1), (25, 2), (49, 3)])
def test_scan_iterations(tiles, iterations, name):
    """511 keys over 24, 25 and 49 tiles of 8,192 segments (kSortTile): 12,264 entries are the last size one loop
    iteration of dk_tcp_sort_scan_kernel takes (12,288 = kSortScanBlock * kSortScanPer), 12,775 need a second (base >
    0, carry != 0, range[] written from it), 25,039 a third. Rows 7 and 100 are DK_TCP_NONE, 5 % of the segments
    strays (keys 2c + 1). An entry count that is an exact multiple of 12,288 is left out: 12,288 has no odd divisor
    but 1 and 3, so it takes 1 row and 4,096 tiles, 33.5M segments."""
    rows, n = SORT_MAX_ROWS, (tiles - 1) * SORT_TILE + 777
    entries = scan_entries(n, rows)
    assert entries == 511 * tiles and scan_iterations(n, rows) == iterations
    assert (iterations - 1) * SCAN_ITERATION < entries <= iterations * SCAN_ITERATION
    if tiles == 24:  # one more tile would not fit the iteration
        assert entries + (2 * rows + 1) > SCAN_ITERATION
    both_sorts(*crafted_case(name, n, rows), f"{name} {tiles} tiles")


# ---- B2: the benchmark's shape ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("reorder", [0.0, 3.0])
def test_scan_second_iteration_at_64_flows(reorder):
    """bench.py's 64-connection stream at the smallest tile count that reaches a second scan iteration: 65 rows (the
    listener's too), 131 keys, 94 tiles of 8,192 (kSortTile), 12,314 entries > 12,288 (kSortScanBlock *
    kSortScanPer), so the ranges (every 94th entry, no power of two) are written on both sides of the boundary."""
    n = 93 * SORT_TILE + 777
    _, tr, table = synth.tcp_streams(n, 64, 1500, buffer_size=1 << 24, reorder=reorder)
    assert len(table) == 65 and scan_entries(n, 65) == 131 * 94 == 12314 and scan_iterations(n, 65) == 2
    assert scan_iterations(n - SORT_TILE, 65) == 1  # 93 tiles would not
    rx = B.stream_rx(tr)
    exp_t = table.copy()
    exp = O.tcp_process(exp_t, rx)
    both_sorts(table, rx, exp_t, exp, f"64 flows reorder {reorder}")


# ---- B3: size edges, one context -------------------------------------------------------------------------------------


def test_size_edges_on_one_context():
    """n at the edges of a wave's round (64), a wave's share of a tile (1,024) and a tile (8,192), through one context
    per sort, growing, then back to 65: the scratch (count table included) is reused at every size. 23 rows, row 7
    DK_TCP_NONE."""
    import torch

    rows = 23
    sizes = [1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 65]
    ctxs = {radix: TcpReceiver(0, radix_sort=radix) for radix in (False, True)}
    for n in sizes:
        table, rx, exp_t, exp = crafted_case("uniform", n, rows)
        r = rx_device(rx)
        for radix, tcp in ctxs.items():
            got_t, got = gpu_process(tcp, table.copy(), r)
            assert tcp.last_sort == ("radix" if radix else "counting"), (n, radix)
            assert_same(got_t, got, exp_t, exp, f"n {n} radix {radix} ({tcp.last_walk} walk)")
    torch.cuda.synchronize()
    for tcp in ctxs.values():
        tcp.close()


def test_last_sort_without_an_ordering():
    """dk_diag_tcp_last_sort is -1 (None) before the first call and after a call that orders nothing by connection:
    no segments, or no table rows (every segment SKIP); a call with work in between reports its sort again."""
    tcp = TcpReceiver(0)
    seen = [tcp.last_sort]
    for n, rows in ((5, 3), (0, 3), (5, 3), (4, 0)):
        table, rx, exp_t, exp = crafted_case("uniform", n, rows, ())
        got_t, got = gpu_process(tcp, table.copy(), rx_device(rx))
        seen.append(tcp.last_sort)
        assert_same(got_t, got, exp_t, exp, f"n {n} rows {rows}")
    tcp.close()
    assert seen == [None, "counting", None, "counting", None]


# ---- B4: key-count edges ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["uniform", "last_row_only"])
@pytest.mark.parametrize("rows", [1, 7, 8])
def test_key_count_edges(rows, name):
    """3 keys (2 bits), 15 keys (4 bits: the last count that goes by key group, kSortGroupBits) and 17 keys (5 bits: one
    add per segment) over 4 tiles, the last partial. Row 3 is DK_TCP_NONE where the table has one."""
    n = 3 * SORT_TILE + 777
    assert (2 * rows).bit_length() == {1: 2, 7: 4, 8: 5}[rows]  # bits of the largest key, 2 rows
    both_sorts(*crafted_case(name, n, rows, (3,)), f"{name} {rows} rows")


# ---- B5: the rule's boundaries ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("rows,n,walk", [(40, 8 * 40 - 1, "lane"), (40, 8 * 40, "wave"), (40, 1024 * 40 - 1, "wave"),
                                         (40, 1024 * 40, "scan"), (256, 1024 * 256, "scan"),
                                         (257, 1024 * 257, "wave")])
def test_rule_boundaries(rows, n, walk):
    """pick_walk's thresholds on a fresh context, no walk forced: below kWaveWalkMinSegs (8) segments per row a lane
    per connection, from it a wave, from kScanMinSegs (1,024) per row the scan walk, up to DK_TCP_SCAN_MAX_CONNS (256)
    rows. No DK_TCP_NONE rows; above 255 rows the rule's sort is the radix sort too."""
    both_sorts(*crafted_case("uniform", n, rows, ()), f"{rows} rows n {n}", want_walk=walk)


@pytest.mark.parametrize("rows", [2048, 2049])
def test_wave_walk_both_instantiations(rows):
    """dk_tcp_wave_walk_kernel<true> up to kDeepAheadMaxConns (2,048) rows, <false> above; the wave walk forced."""
    both_sorts(*crafted_case("uniform", 64 * rows, rows, ()), f"{rows} rows", walk="wave", want_walk="wave")


def test_forced_scan_walk_falls_back_above_65535_rows():
    """The scan walk's grids have a row per connection: forced at 65,536 rows the relay walk runs instead."""
    both_sorts(*crafted_case("uniform", 100000, 65536, ()), "65536 rows", walk="scan", want_walk="relay")
