"""The socket demux on crafted hash collisions, probe chains and wrap-around: every case of tests/demux_keys.py through
the four receive families (the general lookup site and the small-frame kernel's own) with the LDS Active table allowed
and forced off, and the UDP cases through the small-frame kernel's compact bind table and the port table. Every launch
has two checks: all result arrays and both counter arrays bit-exact against the CPU oracle, and flow id and verdict
equal to the dict model of demux_keys (no hashing of ours, independent of the oracle). The host's debug line says which
structure a launch read, so a case cannot silently run on the other one. tests/test_demux_keys.py proves on the CPU
that each case sits where it claims and that a wrong lookup would be caught."""
import functools

import numpy as np
import pytest

import demux_keys as D
import test_gpu_parity as P
from demikernel_amd import Config, FrameBatch, RxEngine, synth
from demikernel_amd import _native as N

pytestmark = pytest.mark.gpu

FAMILIES = ["unstaged", "staged", "split", "small"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def reference(name, small):
    """The case's frames with the oracle's results and the model's (flow id, verdict): computed once, never written."""
    f = D.frames(name, small)
    exp = P.run_oracle(f.blob, f.off, f.lens, D.case(name).flows)
    for v in exp.values():
        v.setflags(write=False)
    return f, exp, D.expected(name, small)


def launch(eng, name, small, ctx):
    """One launch of the case on an engine that holds its socket table, with both checks."""
    import torch

    f, exp, (fid, verdict) = reference(name, small)
    b = FrameBatch.from_numpy(f.blob.copy(), f.off.copy(), f.lens.copy(), device=0)
    r = eng.results(f.n, tcp_fields=True)
    eng.receive_batch(b, r)
    torch.cuda.synchronize()
    got = r.to_numpy()
    P.assert_same(got, exp, ctx)
    bad = np.nonzero((got["flow_id"] != fid) | (got["meta"] & 0xFF != verdict))[0]
    assert bad.size == 0, (ctx, "model", bad[:10], got["flow_id"][bad[:10]], fid[bad[:10]],
                           [N.VERDICTS[m & 0xFF] for m in got["meta"][bad[:10]]],
                           [D.rows(D.case(name).targets[f.idx[bad[:10]]])])
    return got


def run(name, fam, tune, ctx):
    eng = RxEngine(Config(synth.BOB_IPV4), device=0, tuning={**P.family(fam), "debug": 1, **tune})
    eng.set_sockets(D.case(name).flows)
    try:
        return launch(eng, name, fam == "small", ctx)
    finally:
        eng.close()


def debug_words(capfd, key):
    used = [int(w.split("=")[1]) for w in capfd.readouterr().err.split() if w.startswith(key + "=")]
    assert used, "no debug line"
    return used


def check_lds_path(used, name, fam, lds, ctx):
    """What the debug line must say about the LDS Active table. Off when asked, in the small-frame kernel (it has no
    copy) and where the builder refuses (one_hash). Else, as test_lds_active_table: whether a table fits depends on the
    device's LDS and the kernel's static LDS, so the key count is asserted for tables of up to 7 keys and 0 or the key
    count for the larger ones (16 at most here)."""
    lt = D.tables(name).lds
    if lds == 0 or fam == "small" or lt is None:
        assert used == [0] * len(used), (ctx, used)
    elif lt.n <= 7:
        assert used == [lt.n] * len(used), (ctx, used)
    else:
        assert all(u in (0, lt.n) for u in used), (ctx, used)


@pytest.mark.parametrize("lds", [-1, 0])
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("name", D.CASES)
def test_crafted_tables(torch_cuda, capfd, name, fam, lds):
    """Every case in every family, the LDS Active table by the host's rule and forced off: 4,096 frames (64 bytes for
    the small-frame kernel, 64..1514 for the others), hits and misses of every depth drawn at random, then whole waves
    that all hit at depth 0, all hit the chain's last entry and all miss through the full chain."""
    ctx = f"{name} {fam} lds_table={lds}"
    got = run(name, fam, {"lds_table": lds}, ctx)
    check_lds_path(debug_words(capfd, "lds_table"), name, fam, lds, ctx)
    seen = {N.VERDICTS[m & 0xFF] for m in got["meta"]}
    assert {"OK_TCP", "TCP_NOSOCK"} <= seen <= {"OK_TCP", "TCP_NOSOCK", "OK_UDP", "UDP_NOSOCK"}, (ctx, seen)


@pytest.mark.parametrize("udp_table", [1, 0])
@pytest.mark.parametrize("name", D.UDP_CASES)
def test_bind_table_small_family(torch_cuda, capfd, name, udp_table):
    """The UDP cases in the small-frame kernel with the compact bind table wherever it fits (1) and forced off (0):
    udp_seed (placed under seed 3 only, unbound ports that share both buckets with a bound one) and the last flow id
    the table takes. At index 0xFFFE the table is built and read; at 0xFFFF the builder refuses and the port table
    answers even with the knob at 1. The other families read the port table (test_crafted_tables)."""
    ctx = f"{name} small udp_table={udp_table}"
    got = run(name, "small", {"udp_table": udp_table}, ctx)
    modes = set(debug_words(capfd, "udp_table"))
    assert modes == {1 if udp_table == 1 and D.tables(name).ub is not None else 0}, (ctx, modes)
    assert (D.tables(name).ub is None) == (name == "udp_fid_edge_ffff")
    c = D.case(name)
    if name.startswith("udp_fid_edge"):
        assert (got["flow_id"] == c.facts.index).sum() > D.WAVE  # the bind at the edge is found, at its own flow id
    seen = {N.VERDICTS[m & 0xFF] for m in got["meta"]}
    assert seen == {"OK_TCP", "TCP_NOSOCK", "OK_UDP", "UDP_NOSOCK"}, (ctx, seen)


@pytest.mark.parametrize("fam", FAMILIES)
def test_table_replacement(torch_cuda, capfd, fam):
    """set_sockets again and again on one engine: wrap (128 slots, 12 LDS keys), udp_seed (32 slots, 4 LDS keys, bind
    table under seed 3), full_hash_miss (128 slots, 16 LDS keys, no bind table), same_slot_one_field (a bind table
    under seed 0), each launched and checked. A mask, LDS word count or seed left over from the table before would send
    lookups to the wrong slot."""
    eng = RxEngine(Config(synth.BOB_IPV4), device=0, tuning={**P.family(fam), "udp_table": 1, "debug": 1})
    try:
        for name in ("wrap", "udp_seed", "full_hash_miss", "same_slot_one_field"):
            eng.set_sockets(D.case(name).flows)
            ctx = f"replacement {fam}: {name}"
            launch(eng, name, fam == "small", ctx)
            err = capfd.readouterr().err.split()
            used = [int(w.split("=")[1]) for w in err if w.startswith("lds_table=")]
            assert used, "no debug line"
            check_lds_path(used, name, fam, -1, ctx)
            modes = {int(w.split("=")[1]) for w in err if w.startswith("udp_table=")}
            assert modes == {1 if fam == "small" and D.tables(name).ub is not None else 0}, (ctx, modes)
    finally:
        eng.close()
