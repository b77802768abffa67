"""The crafted demux tables of tests/demux_keys.py keep their promises (CPU only): every property a case was built for
is stated here through the restated placements as slot numbers, chain depths, displacements and seeds; the CPU oracle
agrees with the dict model on every frame; and eleven deliberately wrong lookups over the restated tables each disagree
with the model somewhere in the catalogue (a mutation that survived would mean a missing case). The host's real builders
are compared with the restatements in tests/test_host_asan.py."""
import random

import numpy as np
import pytest

import demux_keys as D
from demikernel_amd import _native as N
from oracle.oracle import OraclePeer

CFG = D.CFG


def key(row):
    return row[2], row[3] | row[4] << 16


def where(slots, row):
    """The slot that holds the row's key."""
    return next(k for k, s in enumerate(slots) if s is not None and s[1:] == (row[1],) + key(row))


def stored(name):
    c = D.case(name)
    return D.rows(c.flows)[c.first: c.first + c.nstored]


def targets(name):
    return D.rows(D.case(name).targets)


def lds_slot(lt, row):
    h = D.key_hash(row)
    return D.lt_slot(h, lt.disp[D.lt_bucket(h, lt.nb)], lt.n)


# ---------------------------------------------------------------------------------------------------------------------
# the restatements themselves
# ---------------------------------------------------------------------------------------------------------------------
def test_ports_for_inverts_flow_hash():
    rng = random.Random(1)
    for _ in range(1000):
        kind, lip, rip, tg = rng.choice((1, 2, 3)), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(32)
        p = D.ports_for(kind, lip, rip, tg)
        assert 0 <= p <= D.M32 and D.flow_hash(kind, lip, rip, p) == tg
    # and flow_hash is injective in ports: two different ports words never share a hash
    assert len({D.flow_hash(1, CFG, 7, p) for p in range(5000)}) == 5000


def test_capacity_rule():
    nact = (0, 1, 2, 3, 8, 12, 16, 17, 1 << 23, (1 << 23) + 1, 1 << 25, (1 << 25) + 1)
    assert [D.table_capacity(k) for k in nact] == \
        [16, 16, 16, 32, 64, 128, 128, 256, 1 << 26, 1 << 26, 1 << 26, 1 << 27]


def test_catalogue_rows_are_sendable():
    """Every target's source address passes the IPv4 source checks (not 0.0.0.0, broadcast or multicast), stored keys
    are distinct, absent keys are absent, and every case has a listener on every second absent TCP key's port."""
    for name in D.CASES:
        c = D.case(name)
        flows, tg = D.rows(c.flows), targets(name)
        assert len(set(tg)) == len(tg), name
        for t in tg:
            if t[0] == D.ACTIVE or t[2]:
                assert 1 <= t[2] & 255 <= 223, (name, t)
        absent = [t for t in tg if t[0] == D.ACTIVE and t not in flows]
        assert absent, name
        for k, t in enumerate(absent):
            if k % 2 == 0:
                assert (D.PASSIVE, CFG, 0, t[3], 0) in flows, (name, t)
        assert len(c.flows) <= 64 or name.startswith("udp_fid_edge")


# ---------------------------------------------------------------------------------------------------------------------
# builder promises
# ---------------------------------------------------------------------------------------------------------------------
def test_wrap_chain_is_last_slot_then_zero_to_ten():
    c, t = D.case("wrap"), D.tables("wrap")
    cap = len(t.slots)
    assert cap == 128
    assert [k for k, s in enumerate(t.slots) if s is not None] == list(range(11)) + [cap - 1]
    for depth, row in enumerate(stored("wrap")):
        assert D.key_hash(row) & 0x3FFFFFF == 0x3FFFFFF  # the last slot of any table of up to 2^26 slots
        assert where(t.slots, row) == (cap - 1 + depth) % cap
        assert D.global_lookup(t.slots, CFG, *key(row)) == (depth, depth)  # flow id = insertion order = depth
    walks = sorted(c.facts.walk.values())
    assert walks.count(12) == 8 and walks.count(8) == 8 and {0, 1, 3, 6, 11} <= set(walks)
    rips = {r[2] for r in stored("wrap")}
    for row, steps in c.facts.walk.items():
        assert D.global_lookup(t.slots, CFG, *key(row)) == (None, steps), row
        if steps == 12:  # the full-chain misses differ from a stored key in the ports alone
            assert row[2] in rips and D.key_hash(row) & 0x3FFFFFF == 0x3FFFFFF
        if steps == 8:
            assert D.key_hash(row) & 0x3FFFFFF == 3
    # the hashes are distinct, so the LDS copy builds as well
    assert t.lds is not None and t.lds.n == 12


def test_one_hash_is_eight_keys_with_one_hash():
    c, t = D.case("one_hash"), D.tables("one_hash")
    st = stored("one_hash")
    assert len(st) == 8 and len(set(st)) == 8 and {D.key_hash(r) for r in st} == {c.facts.H}
    assert len(c.facts.same) == 8 and {D.key_hash(r) for r in c.facts.same} == {c.facts.H}
    assert not set(c.facts.same) & set(st)
    assert t.lds is None  # the host's rule: two keys with one hash are never separable
    cap = len(t.slots)
    assert cap == 64 and [where(t.slots, r) for r in st] == [61, 62, 63, 0, 1, 2, 3, 4]
    for r in c.facts.same:
        assert D.global_lookup(t.slots, CFG, *key(r)) == (None, 8)


def test_same_slot_one_field_lands_on_k():
    c, t = D.case("same_slot_one_field"), D.tables("same_slot_one_field")
    K, lt = c.facts.K, t.lds
    assert len(stored("same_slot_one_field")) == 16 and K in stored("same_slot_one_field")
    home = D.key_hash(K) & (len(t.slots) - 1)
    assert where(t.slots, K) == home
    assert len(c.facts.other_ip) == 3
    for r in c.facts.other_ip:  # another remote address, the same ports: K's slot in both structures
        assert r[3:] == K[3:] and r[2] != K[2]
        assert D.key_hash(r) & (len(t.slots) - 1) == home
        assert D.lt_bucket(D.key_hash(r), lt.nb) == D.lt_bucket(D.key_hash(K), lt.nb)
        assert lds_slot(lt, r) == lds_slot(lt, K) == lt.slot_of[key(K)]
    near = c.facts.one_bit  # the same remote address, one bit of one port flipped
    assert len(near) == 32 and all(r[2] == K[2] for r in near)
    assert sorted(bin((r[3] | r[4] << 16) ^ (K[3] | K[4] << 16)).count("1") for r in near) == [1] * 32
    on_k = [r for r in near if lds_slot(lt, r) == lds_slot(lt, K)]
    print(f"\n{len(on_k)} of 32 one-bit neighbours land on K's LDS slot; all 32 land on a stored key's slot")
    assert on_k
    assert c.facts.swapped == K[:3] + (K[4], K[3]) and c.facts.swapped not in D.rows(c.flows)
    d = dict(zip(targets("same_slot_one_field"), D.depths("same_slot_one_field")))
    assert d[c.facts.as_udp[0]][0] == "udp_nosock" and d[c.facts.as_udp[1]][0] == "bind"
    assert all(u[0] == D.UDP and (D.ACTIVE,) + u[1:] in D.rows(c.flows) for u in c.facts.as_udp)


def test_full_hash_miss_shares_every_hash():
    c, t = D.case("full_hash_miss"), D.tables("full_hash_miss")
    assert len(c.facts.twin) == 16 and t.lds is not None and t.lds.n == 16
    for absent, st in c.facts.twin.items():
        assert D.key_hash(absent) == D.key_hash(st) and absent[2] != st[2] and absent not in D.rows(c.flows)
        assert lds_slot(t.lds, absent) == t.lds.slot_of[key(st)]
        assert D.global_lookup(t.slots, CFG, *key(absent))[0] is None
    # lanes of one wave need different walk depths: the random keys give chains by themselves
    assert len({s for o, s in D.depths("full_hash_miss")}) >= 3


def test_crowded_bucket_needs_more_than_sixteen_bits():
    t = D.tables("crowded_bucket")
    st = stored("crowded_bucket")
    assert len(st) == 14 and all(D.key_hash(r) < 1 << 30 for r in st)
    assert (t.lds.n, t.lds.nb) == (14, 4) and all(D.lt_bucket(D.key_hash(r), 4) == 0 for r in st)
    print(f"\ncrowded_bucket displacements {t.lds.disp}")
    assert t.lds.disp[0] >= 65536 and t.lds.disp[1:] == [0, 0, 0]
    buckets = [D.lt_bucket(D.key_hash(r), 4) for r in targets("crowded_bucket") if r not in st]
    assert {b: buckets.count(b) for b in range(4)} == {0: 6, 1: 2, 2: 2, 3: 2}


def test_tiny_tables_are_sixteen_slots():
    for name, occupied in (("tiny1", [9]), ("tiny2", [0, 15])):
        c, t = D.case(name), D.tables(name)
        assert len(t.slots) == 16 and [k for k, s in enumerate(t.slots) if s is not None] == occupied
        assert t.lds is not None and t.lds.n == len(occupied)
        for row, steps in c.facts.walk.items():
            assert D.global_lookup(t.slots, CFG, *key(row)) == (None, steps), (name, row)
        assert max(c.facts.walk.values()) == len(occupied) and 0 in c.facts.walk.values()
    assert [D.global_lookup(D.tables("tiny2").slots, CFG, *key(r)) for r in stored("tiny2")] == [(0, 0), (1, 1)]


def test_udp_seed_forces_seed_three():
    c, t = D.case("udp_seed"), D.tables("udp_seed")
    ports, ub = c.facts.ports, t.ub
    assert len(ports) == 16 and ports[-1] == 65535 and min(ports) >= 1024 and len(set(ports)) == 16
    for g in (0, 1, 2):  # group g: five ports, one pair of two different buckets under seed g
        pairs = {D.ub_buckets(p, g, 15) for p in ports[5 * g: 5 * g + 5]}
        assert len(pairs) == 1 and len(set(next(iter(pairs)))) == 2, (g, pairs)
        assert D.udp_build(D.udp_local_words(c.flows), seeds=[g]) is None
    print(f"\nudp_seed: mask {ub.mask} seed {ub.seed} after {ub.failed}; {c.facts.colliding} unbound ports share both "
          f"buckets with a bound one")
    assert ub.mask == 15 and ub.failed == [0, 1, 2] and ub.seed == 3
    bound = {D.ub_buckets(p, ub.seed, ub.mask) for p in ports}
    assert len(c.facts.sample) == 48 and c.facts.colliding > 1000
    assert all(q not in ports and D.ub_buckets(q, ub.seed, ub.mask) in bound for q in c.facts.sample)
    out = [o for o, _ in D.depths("udp_seed")]
    assert (out.count("bind"), out.count("any"), out.count("udp_nosock")) == (16, 16, 32)
    # some bind sits in its second bucket, so a lookup has to read both
    second = [p for p in ports if D.ub_lookup(ub.words, ub.mask, ub.seed, p, first_only=True) is None]
    assert second


def test_udp_fid_edge_indices():
    for name, index, built in (("udp_fid_edge_fffe", 0xFFFE, True), ("udp_fid_edge_ffff", 0xFFFF, False)):
        c, t = D.case(name), D.tables(name)
        port = c.facts.port
        assert D.rows(c.flows[index: index + 1]) == [(D.UDP, CFG, 0, port, 0)]
        assert all(r[0] == D.UDP and r[1] == D.ELSEWHERE for r in D.rows(c.flows[:index]))
        local = D.udp_local_words(c.flows)
        assert np.nonzero(local != D.NONE)[0].tolist() == [port] and local[port] == index
        assert (t.ub is not None) == built
        if built:
            assert D.ub_lookup(t.ub.words, t.ub.mask, t.ub.seed, port) == 0xFFFE
            assert D.ub_lookup(t.ub.words, t.ub.mask, t.ub.seed, 65535) is None
        assert (D.UDP, CFG, 0, 65535, 0) in targets(name)  # unbound: an empty word's low half


# ---------------------------------------------------------------------------------------------------------------------
# model, oracle, restated lookups
# ---------------------------------------------------------------------------------------------------------------------
WANT = {"active": ("OK_TCP", True), "listener": ("OK_TCP", True), "tcp_nosock": ("TCP_NOSOCK", False),
        "bind": ("OK_UDP", True), "any": ("OK_UDP", True), "udp_nosock": ("UDP_NOSOCK", False)}


@pytest.mark.parametrize("small", [True, False], ids=["64B", "mixed"])
@pytest.mark.parametrize("name", D.CASES)
def test_oracle_agrees_with_model(name, small):
    """OraclePeer against the dict model on flow id and verdict for every frame, and every outcome the case was built
    for is there: in the random draw (lanes of one wave differ) and as whole waves of one kind."""
    c, f = D.case(name), D.frames(name, small)
    fid, v = D.expected(name, small)
    peer = OraclePeer(CFG)
    peer.set_flows(c.flows)
    exp = peer.process(f.blob, f.off, f.lens)
    assert np.array_equal(exp["meta"] & 0xFF, v) and np.array_equal(exp["flow_id"], fid)
    assert f.n == 4096 and f.lens.min() >= 64 and f.lens.max() <= (64 if small else 1514)
    d = D.depths(name)
    for k in range(f.n):
        verdict, found = WANT[d[f.idx[k]][0]]
        assert v[k] == N.V[verdict] and (fid[k] != D.NONE) == found, (name, k)
    seen = {d[i][0] for i in f.idx[: f.n - 3 * D.WAVE]}
    want = {"active", "listener", "tcp_nosock"} | ({"bind", "any", "udp_nosock"} if name in D.UDP_CASES else set())
    if name == "same_slot_one_field":
        want |= {"bind", "udp_nosock"}
    assert want <= seen, (name, seen)
    tail = f.idx[f.n - 3 * D.WAVE:].reshape(3, D.WAVE)
    for w, group in zip(tail, D.wave_groups(name)):
        assert set(w.tolist()) <= set(group), (name, group)
    if name in D.TCP_CASES:
        kinds = [{d[i][0] for i in w} for w in tail]
        assert kinds[0] == kinds[1] == {"active"} and kinds[2] <= {"listener", "tcp_nosock"}
        steps = [{d[i][1] for i in w} for w in tail]
        deepest = max(s for o, s in d if o == "active")
        assert steps[0] == {0} and steps[1] == {deepest} and steps[2] == {max(s for o, s in d if o != "active")}
    else:
        assert [{d[i][0] for i in w} for w in tail] == [{"bind"}, {"any"}, {"udp_nosock"}]


@pytest.mark.parametrize("name", D.CASES)
def test_restated_lookups_agree_with_model(name):
    """The unmutated lookups over every restated structure the case has give the model's answer on every frame."""
    t = D.tables(name)
    for small in (True, False):
        fid, v = D.expected(name, small)
        for active in ("global",) + (("lds",) if t.lds else ()):
            for binds in ("port",) + (("compact",) if t.ub else ()):
                g = D.restated_demux(name, small, active=active, binds=binds)
                assert np.array_equal(g[0], fid) and np.array_equal(g[1], v), (name, small, active, binds)


MUTATIONS = {
    "probe stops at the last slot": dict(active="global", wrap=False),
    "probe gives up after 4 steps": dict(active="global", max_steps=4),
    "global compare without remote_ip": dict(active="global", cmp_rip=False),
    "global compare without ports": dict(active="global", cmp_ports=False),
    "LDS compare without remote_ip": dict(active="lds", cmp_rip=False),
    "LDS compare without ports": dict(active="lds", cmp_ports=False),
    "LDS lookup compares nothing": dict(active="lds", compare=False),
    "LDS displacement as 16 bits": dict(active="lds", disp_bits=16),
    "bind lookup with seed 0": dict(binds="compact", seed=0),
    "bind lookup reads the first bucket only": dict(binds="compact", first_only=True),
    "bind lookup accepts flow id 0xFFFF": dict(binds="compact", accept_ffff=True),
}


@pytest.mark.parametrize("small", [True, False], ids=["64B", "mixed"])
@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_mutations_are_caught(mutation, small):
    """Each deliberately wrong lookup disagrees with the model on at least one frame of the catalogue, in the 64-byte
    frames and in the mixed ones (the four families see the same keys)."""
    kw = MUTATIONS[mutation]
    caught = {}
    for name in D.CASES:
        t = D.tables(name)
        if (kw.get("active") == "lds" and t.lds is None) or (kw.get("binds") == "compact" and t.ub is None):
            continue
        fid, v = D.expected(name, small)
        g = D.restated_demux(name, small, **kw)
        bad = int(((g[0] != fid) | (g[1] != v)).sum())
        if bad:
            caught[name] = bad
    print(f"\n{mutation}: frames that differ from the model, per case: {caught}")
    assert caught, mutation


def test_each_mutation_is_caught_by_the_case_built_for_it():
    """Not just somewhere: the wrap catches the probes that stop, the one-field misses the weakened compares, the
    crowded bucket the short displacement, the forced seed and the flow-id edge the bind-table mutations."""
    built_for = {
        "probe stops at the last slot": ["wrap", "one_hash", "tiny2"],
        "probe gives up after 4 steps": ["wrap", "one_hash"],
        "global compare without remote_ip": ["same_slot_one_field"],
        "global compare without ports": ["wrap"],
        "LDS compare without remote_ip": ["same_slot_one_field"],
        "LDS compare without ports": ["same_slot_one_field"],
        "LDS lookup compares nothing": ["wrap", "same_slot_one_field", "full_hash_miss", "crowded_bucket", "tiny1",
                                        "tiny2"],
        "LDS displacement as 16 bits": ["crowded_bucket"],
        "bind lookup with seed 0": ["udp_seed"],
        "bind lookup reads the first bucket only": ["udp_seed"],
        "bind lookup accepts flow id 0xFFFF": ["udp_fid_edge_fffe"],
    }
    for mutation, names in built_for.items():
        for name in names:
            fid, v = D.expected(name, False)
            g = D.restated_demux(name, False, **MUTATIONS[mutation])
            assert ((g[0] != fid) | (g[1] != v)).any(), (mutation, name)
