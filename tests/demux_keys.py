"""TEST INFRASTRUCTURE ONLY: crafted socket tables for the 4-tuple demux, with an independent model of the answer.

The receive path finds a frame's socket in three structures (rx_common.h): the global Active table (open addressing,
linear probing), its LDS copy (a minimal perfect hash) and the small-frame kernel's compact UDP bind table (a two-choice
cuckoo table). With the keys synth.make_flows produces, none of them is ever far off its first probe. `flow_hash` is a
bijection of `ports` once kind, local_ip and remote_ip are fixed, so `ports_for` builds a key for any target hash, and
the catalogue below puts keys exactly where the lookups are hardest: a probe chain that runs off the last slot, eight
keys with one 32-bit hash, misses that differ from a stored key in one field and land on its slot in both structures,
a bucket whose displacement needs more than 16 bits, a bind table no seed below 3 can place, and the last flow id the
bind table takes.

Three kinds of code live here and nothing else:
  - the hashes of rx_common.h and the host's three placements (dk_rx_flow_table_set, build_lds_table,
    build_udp_table of lds_table.h) restated in Python: they only say where a crafted key sits, so that the CPU tests
    can assert each crafted property as slot numbers, depths, displacements and seeds;
  - `model`: the expected flow id and verdict of a frame from plain dicts, none of our hashing;
  - the catalogue and its frames.
The lookups over the restated tables take switches that make them wrong on purpose (tests/test_demux_keys.py: every
such mutation must disagree with `model` somewhere in the catalogue)."""
from __future__ import annotations

import functools
import zlib
from types import SimpleNamespace

import numpy as np

from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd.rx import ipv4

M32 = 0xFFFFFFFF
ACTIVE, PASSIVE, UDP = N.DK_FLOW_TCP_ACTIVE, N.DK_FLOW_TCP_PASSIVE, N.DK_FLOW_UDP
NONE = N.DK_FLOW_NONE
FLOW_DTYPE = N.FLOW_DTYPE
CFG = ipv4(synth.BOB_IPV4)
ELSEWHERE = ipv4("10.9.9.9")  # a local address no lookup ever asks for
UB_EMPTY = 0xFFFFFFFF
N_FRAMES = 4096
WAVE = 64


# ---------------------------------------------------------------------------------------------------------------------
# rx_common.h, restated
# ---------------------------------------------------------------------------------------------------------------------
def h2(kind, lip, rip):
    """flow_hash's state just before `ports` is mixed in (the rest is a bijection of h2 ^ ports)."""
    h = (kind * 0x9E3779B1) & M32
    h ^= lip
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h ^= rip
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def flow_hash(kind, lip, rip, ports):
    h = h2(kind, lip, rip) ^ ports
    h = (h * 0x27D4EB2F) & M32
    h ^= h >> 15
    return h


_INV_27D4EB2F = pow(0x27D4EB2F, -1, 1 << 32)


def ports_for(kind, lip, rip, target_hash):
    """The `ports` word (local_port | remote_port << 16) that gives (kind, lip, rip, ports) the hash `target_hash`:
    flow_hash's last three steps undone."""
    x = target_hash
    x ^= x >> 15
    x ^= x >> 30
    x = (x * _INV_27D4EB2F) & M32
    return x ^ h2(kind, lip, rip)


def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def mulhi(a, b):
    return (int(a) * int(b)) >> 32


def lt_bucket(h, nb):
    return mulhi(h, nb)


def lt_slot(h, d, n):
    return mulhi(fmix32(h ^ ((d * 0x9E3779B1 + 0x7F4A7C15) & M32)), n)


def lt_lookup(words, n, nb, lip, rip, ports, compare=True, disp_bits=32, cmp_rip=True, cmp_ports=True):
    """rx_kernels.hip lt_lookup over the LDS table's words. compare=False, disp_bits=16, cmp_rip=False,
    cmp_ports=False: deliberately wrong."""
    h = flow_hash(ACTIVE, lip, rip, ports)
    d = int(words[3 * n + lt_bucket(h, nb)]) & ((1 << disp_bits) - 1)
    sl = lt_slot(h, d, n)
    if not compare or ((not cmp_rip or int(words[sl]) == rip) and (not cmp_ports or int(words[n + sl]) == ports)):
        return int(words[2 * n + sl])
    return None


def ub_hash(port, seed):
    return fmix32((port * 0x9E3779B1 + seed) & M32)


def ub_lookup(words, mask, seed, port, first_only=False, accept_ffff=False):
    """rx_common.h ub_pick over the words of the port's two buckets. first_only, accept_ffff: deliberately wrong."""
    h = ub_hash(port, seed)
    b1, b2 = h & mask, (h >> 16) & mask
    es = [int(words[2 * b1]), int(words[2 * b1 + 1])]
    if not first_only:
        es += [int(words[2 * b2]), int(words[2 * b2 + 1])]
    for e in es:
        if (e ^ port) & 0xFFFF == 0 and (accept_ffff or e >> 16 != 0xFFFF):
            return e >> 16
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the host's placements, restated
# ---------------------------------------------------------------------------------------------------------------------
def _pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def table_capacity(nact):
    """dk_rx_flow_table_set: load <= 1/8 up to 2^26 slots, never above 1/2, 16 slots at least."""
    nact = max(nact, 1)
    return max(16, _pow2(min(8 * nact, 1 << 26)), _pow2(2 * nact))


def rows(flows):
    """FLOW_DTYPE rows as plain tuples (kind, local_ip, remote_ip, local_port, remote_port)."""
    return [tuple(int(x) for x in r) for r in np.asarray(flows, FLOW_DTYPE).tolist()]


def global_place(flows):
    """The Active table's slots as the host fills them: a list of None or (flow id, lip, rip, ports), every Active row
    in table order by linear probing from flow_hash & mask; a repeated key overwrites its slot (the last wins)."""
    act = [(i, r) for i, r in enumerate(rows(flows)) if r[0] == ACTIVE]
    cap = table_capacity(len(act))
    slots = [None] * cap
    for i, (_, lip, rip, lp, rp) in act:
        key = (lip, rip, lp | rp << 16)
        h = flow_hash(ACTIVE, *key) & (cap - 1)
        while slots[h] is not None and slots[h][1:] != key:
            h = (h + 1) & (cap - 1)
        slots[h] = (i,) + key
    return slots


def global_lookup(slots, lip, rip, ports, wrap=True, max_steps=None, cmp_rip=True, cmp_ports=True):
    """probe_slot / probe_finish over the restated slots: (flow id or None, occupied slots visited before the answer).
    wrap=False, max_steps, cmp_rip=False, cmp_ports=False: deliberately wrong."""
    cap = len(slots)
    h = flow_hash(ACTIVE, lip, rip, ports) & (cap - 1)
    for step in range(cap + 1):
        s = slots[h]
        if s is None or (max_steps is not None and step >= max_steps):
            return None, step
        if s[1] == lip and (not cmp_rip or s[2] == rip) and (not cmp_ports or s[3] == ports):
            return s[0], step
        if not wrap and h == cap - 1:
            return None, step + 1
        h = (h + 1) & (cap - 1)
    return None, cap + 1


def slot_words(slots):
    """The slots as the u32[cap][4] the host builds (x = kind << 24 | flow id, 0 empty)."""
    w = np.zeros((len(slots), 4), np.uint32)
    for k, s in enumerate(slots):
        if s is not None:
            w[k] = (ACTIVE << 24 | s[0], s[1], s[2], s[3])
    return w


def _fmix_np(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    return h ^ (h >> np.uint64(16))


def _first_displacement(hs, taken, n, limit=1 << 20):
    """The smallest d < limit that puts every hash of hs on its own free slot (lt_slot), searched a block of d at a
    time; None when there is none."""
    hs = np.asarray(hs, np.uint64)
    d0, step = 0, 256
    while d0 < limit:
        d = np.arange(d0, min(d0 + step, limit), dtype=np.uint64)
        salt = (d * np.uint64(0x9E3779B1) + np.uint64(0x7F4A7C15)) & np.uint64(M32)
        sl = (_fmix_np(hs[None, :] ^ salt[:, None]) * np.uint64(n)) >> np.uint64(32)
        ok = ~taken[sl].any(axis=1)
        if len(hs) > 1:
            srt = np.sort(sl, axis=1)
            ok &= (srt[:, 1:] != srt[:, :-1]).all(axis=1)
        hit = np.nonzero(ok)[0]
        if len(hit):
            return int(d[hit[0]])
        d0 += step
        step = min(step * 4, 1 << 16)
    return None


def lds_build(slots, cfg_ip=CFG, max_keys=4096):
    """build_lds_table (lds_table.h) over the restated slots: None when the host refuses (no key on cfg_ip, more than
    4,096, two keys with one 32-bit hash, no displacement below 2^20), else n, nb, the table's words, each bucket's
    displacement and each key's slot ({(rip, ports): slot})."""
    keys = [(flow_hash(ACTIVE, cfg_ip, s[2], s[3]), s[2], s[3], s[0])
            for s in slots if s is not None and s[1] == cfg_ip]
    n = len(keys)
    if n == 0 or n > max_keys or len({k[0] for k in keys}) < n:
        return None
    nb = (n + 3) // 4
    bucket = [[] for _ in range(nb)]
    for k, key in enumerate(keys):
        bucket[lt_bucket(key[0], nb)].append(k)
    order = sorted(range(nb), key=lambda b: -len(bucket[b]))  # stable: equal sizes stay in index order
    taken = np.zeros(n, bool)
    disp, slot_of = [0] * nb, {}
    for b in order:
        if not bucket[b]:
            break
        d = _first_displacement([keys[k][0] for k in bucket[b]], taken, n)
        if d is None:
            return None
        disp[b] = d
        for k in bucket[b]:
            sl = lt_slot(keys[k][0], d, n)
            taken[sl] = True
            slot_of[keys[k][1:3]] = sl
    words = np.zeros((3 * n + nb + 3) & ~3, np.uint32)
    for _, rip, ports, fid in keys:
        sl = slot_of[(rip, ports)]
        words[sl], words[n + sl], words[2 * n + sl] = rip, ports, fid
    words[3 * n: 3 * n + nb] = disp
    return SimpleNamespace(n=n, nb=nb, words=words, disp=disp, slot_of=slot_of)


def udp_local_words(flows, cfg_ip=CFG):
    """The port table's kPortUdpLocal words: the flow id bound to (cfg_ip, port), NONE elsewhere; the last bind wins."""
    local = np.full(65536, NONE, np.uint32)
    for i, (kind, lip, _, lp, _) in enumerate(rows(flows)):
        if kind == UDP and lip == cfg_ip:
            local[lp] = i
    return local


def udp_build(local, seeds=range(64)):
    """build_udp_table (lds_table.h) from the port table's local-bind words: None when the host refuses (no bind, more
    than 32,768, a flow id >= 0xFFFF, no seed), else mask, seed, the words and the seeds that failed before it."""
    keys = [int(p) | int(local[p]) << 16 for p in np.nonzero(np.asarray(local) != NONE)[0]]
    if not keys or len(keys) > 1 << 15 or any(e >> 16 >= 0xFFFF for e in keys):
        return None
    nb = max(16, _pow2(len(keys)))
    m = nb - 1
    failed = []
    for sd in seeds:
        out, ok = [UB_EMPTY] * (2 * nb), True
        for e in keys:
            frm, kick = None, 0
            while True:
                h = ub_hash(e & 0xFFFF, sd)
                b1, b2 = h & m, (h >> 16) & m
                at = next((2 * b + w for b in (b1, b2) for w in (0, 1) if out[2 * b + w] == UB_EMPTY), None)
                if at is not None:
                    out[at] = e
                    break
                if kick == 500:
                    ok = False
                    break
                b = b2 if frm == b1 else b1  # not back into the bucket it just left
                e, out[2 * b + (kick & 1)] = out[2 * b + (kick & 1)], e
                frm, kick = b, kick + 1
            if not ok:
                break
        if ok:
            return SimpleNamespace(mask=m, seed=sd, words=np.array(out, np.uint32), failed=failed)
        failed.append(sd)
    return None


def ub_buckets(port, seed, mask):
    h = ub_hash(port, seed)
    return h & mask, (h >> 16) & mask


# ---------------------------------------------------------------------------------------------------------------------
# the reference: plain dicts
# ---------------------------------------------------------------------------------------------------------------------
def model(flows, cfg_ip, proto, src_ip, sport, dport):
    """Expected (flow id, verdict) per frame. TCP: Active(cfg_ip, dport, src_ip, sport), else Passive(cfg_ip, dport),
    else no socket. UDP: (cfg_ip, dport), else (0.0.0.0, dport), else no socket. A repeated key's last row wins."""
    act, pas, udp = {}, {}, {}
    for i, (kind, lip, rip, lp, rp) in enumerate(rows(flows)):
        if kind == ACTIVE:
            act[(lip, lp, rip, rp)] = i
        elif kind == PASSIVE:
            pas[(lip, lp)] = i
        else:
            udp[(lip, lp)] = i
    fid = np.full(len(proto), NONE, np.uint32)
    v = np.zeros(len(proto), np.uint32)
    for k, (p, s, sp, dp) in enumerate(zip(proto.tolist(), src_ip.tolist(), sport.tolist(), dport.tolist())):
        if p == 6:
            f = act.get((cfg_ip, dp, s, sp), pas.get((cfg_ip, dp)))
            v[k] = N.V["TCP_NOSOCK"] if f is None else N.V["OK_TCP"]
        else:
            f = udp.get((cfg_ip, dp), udp.get((0, dp)))
            v[k] = N.V["UDP_NOSOCK"] if f is None else N.V["OK_UDP"]
        if f is not None:
            fid[k] = f
    return fid, v


def outcome(keys, cfg_ip, t):
    """What a target row ends as, by the model's rule: active / listener / tcp_nosock / bind / any / udp_nosock.
    keys: the table's rows as a set."""
    kind, lip, rip, lp, rp = t
    if kind == ACTIVE:
        return "active" if (ACTIVE, cfg_ip, rip, lp, rp) in keys else \
            "listener" if (PASSIVE, cfg_ip, 0, lp, 0) in keys else "tcp_nosock"
    return "bind" if (UDP, cfg_ip, 0, lp, 0) in keys else "any" if (UDP, 0, 0, lp, 0) in keys else "udp_nosock"


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------
def rip(a, b, c, first=10):
    """first.a.b.c in octet order: unicast for first in 1..223, so the IPv4 source checks pass."""
    return first | a << 8 | b << 16 | c << 24


def akey(r, ports):
    """An Active row on the configured address from a remote address and a ports word."""
    return (ACTIVE, CFG, r, ports & 0xFFFF, ports >> 16)


def akey_hash(r, target_hash):
    return akey(r, ports_for(ACTIVE, CFG, r, target_hash))


def key_hash(row):
    return flow_hash(ACTIVE, row[1], row[2], row[3] | row[4] << 16)


def _arr(rws):
    return np.array(rws, dtype=FLOW_DTYPE)


def _case(name, stored, absent, extra=(), targets_extra=(), front=(), **facts):
    """flows = front rows, the stored Active keys, a Passive listener on the local port of every second absent TCP
    key, then `extra`; targets = stored keys, absent keys and `targets_extra`."""
    listeners = [(PASSIVE, CFG, 0, t[3], 0) for t in [a for a in absent if a[0] == ACTIVE][::2]]
    flows = _arr(list(front) + list(stored) + listeners + list(extra))
    targets = _arr(list(stored) + list(absent) + list(targets_extra))
    flows.setflags(write=False)
    targets.setflags(write=False)
    return SimpleNamespace(name=name, flows=flows, targets=targets, first=len(front), nstored=len(stored),
                           facts=SimpleNamespace(**facts))


def _wrap():
    tail = 0x3FFFFFF  # the last slot of every power-of-two table of up to 2^26 slots
    stored = [akey_hash(rip(j, 7, 1), j << 26 | tail) for j in range(1, 13)]
    # misses through the whole chain, each with a stored key's remote address (only the ports differ)
    full = [akey_hash(stored[j - 13][2], j << 26 | tail) for j in range(13, 21)]
    after = [akey_hash(rip(j, 8, 1), j << 26 | 3) for j in range(1, 9)]  # enter the chain after the wrap
    more = [akey_hash(rip(j, 9, 1), j << 26 | s) for j, s in ((1, 0), (2, 10), (3, 11), (4, tail - 1), (5, 5), (6, 8))]
    walk = {**{t: 12 for t in full}, **{t: 8 for t in after},
            **dict(zip(more, (11, 1, 0, 0, 6, 3)))}
    return _case("wrap", stored, full + after + more, walk=walk)


def _one_hash():
    H = 0x5A5A5A3D  # slot 61 of the 64 this table gets: the chain of eight wraps as well
    stored = [akey_hash(rip(j, 21, 3), H) for j in range(1, 9)]
    same = [akey_hash(rip(j, 22, 3), H) for j in range(1, 9)]
    near = [akey_hash(rip(1, 23, 3), H + 3), akey_hash(rip(2, 23, 3), H - 1), akey_hash(rip(3, 23, 3), H + 11)]
    return _case("one_hash", stored, same + near, H=H, same=same)


def _random_keys(rng, k):
    return [akey(rip(*(int(x) for x in rng.integers(0, 256, 3)), first=int(rng.integers(1, 224))),
                 int(rng.integers(0, 1 << 32))) for _ in range(k)]


def _full_hash_miss():
    rng = np.random.default_rng(41)
    stored = _random_keys(rng, 16)
    absent = [akey_hash(rip(j, 31, 5, first=172), key_hash(s)) for j, s in enumerate(stored)]
    return _case("full_hash_miss", stored, absent, twin=dict(zip(absent, stored)))


def _same_slot_one_field():
    rng = np.random.default_rng(43)
    stored = _random_keys(rng, 16)
    slots = global_place(_arr(stored))
    lt = lds_build(slots)
    mask = len(slots) - 1

    def lds_slot(row):
        h = key_hash(row)
        return lt_slot(h, lt.disp[lt_bucket(h, lt.nb)], lt.n)

    def one_bit(K):
        return [K[:3] + (K[3] ^ 1 << b, K[4]) for b in range(16)] + [K[:4] + (K[4] ^ 1 << b,) for b in range(16)]

    # K: a key in its home slot with a one-bit neighbour that lands on its LDS slot
    K = next(K for K in stored if slots[key_hash(K) & mask][1:] == (CFG, K[2], K[3] | K[4] << 16)
             and any(lds_slot(t) == lds_slot(K) for t in one_bit(K)))
    ports = K[3] | K[4] << 16
    hK, other_ip = key_hash(K), []
    for t in range(1, 1 << 22):  # same ports, another remote address: K's global slot, LDS bucket and LDS slot
        r = rip(t & 255, t >> 8 & 255, t >> 16 & 255, first=172)
        h = flow_hash(ACTIVE, CFG, r, ports)
        if ((h ^ hK) & mask == 0 and lt_bucket(h, lt.nb) == lt_bucket(hK, lt.nb)
                and lds_slot(akey(r, ports)) == lds_slot(K)):
            other_ip.append(akey(r, ports))
            if len(other_ip) == 3:
                break
    swapped = K[:3] + (K[4], K[3])
    K2 = next(s for s in stored if s != K and s[3] != K[3])
    # K's 4-tuple as UDP (no bind on its port) and K2's (a bind on its port): UDP never reads the Active table
    as_udp = [(UDP, CFG, K[2], K[3], K[4]), (UDP, CFG, K2[2], K2[3], K2[4])]
    return _case("same_slot_one_field", stored, other_ip + one_bit(K) + [swapped], extra=[(UDP, CFG, 0, K2[3], 0)],
                 targets_extra=as_udp, K=K, other_ip=other_ip, one_bit=one_bit(K), swapped=swapped, as_udp=as_udp)


def _crowded_bucket(seed=0):
    """14 keys in LDS bucket 0 of 4: the builder needs a displacement that puts all 14 on 14 different slots of 14, a
    chance of 14! / 14^14 = 1 in 127,000 per try. Under seed 0 the first one is 148,868 (seeds 0..11 gave between
    15,780 and 331,482); tests/test_demux_keys.py asserts that it does not fit 16 bits."""
    rng = np.random.default_rng(seed)
    hashes = sorted(set(int(x) for x in rng.integers(0, 1 << 30, 14)))  # bucket 0 of 4: mulhi(h, 4) == 0
    assert len(hashes) == 14
    stored = [akey_hash(rip(j, 51, 7), h) for j, h in enumerate(hashes)]
    absent = [akey_hash(rip(j, 52, 7), int(rng.integers(0, 1 << 30))) for j in range(6)]
    absent += [akey_hash(rip(j, 53, 7), b << 30 | int(rng.integers(0, 1 << 30)))
               for j, b in enumerate((1, 1, 2, 2, 3, 3))]
    return _case("crowded_bucket", stored, absent)


def _tiny1():
    h = 0x13572469
    stored = [akey_hash(rip(1, 61, 9), h)]
    absent = [akey_hash(rip(2, 61, 9), h), akey_hash(rip(3, 61, 9), h ^ 0x40), akey_hash(rip(4, 61, 9), h + 1),
              akey_hash(rip(5, 61, 9), h ^ 0x80000000)]
    return _case("tiny1", stored, absent, walk=dict(zip(absent, (1, 1, 0, 1))))


def _tiny2():
    stored = [akey_hash(rip(1, 62, 9), 0x2468ACEF), akey_hash(rip(2, 62, 9), 0x9753135F)]  # both in slot 15 of 16
    absent = [akey_hash(rip(3, 62, 9), 0x2468ACEF), akey_hash(rip(4, 62, 9), 0x1111111F),
              akey_hash(rip(5, 62, 9), 0x22222220), akey_hash(rip(6, 62, 9), 0x33333331)]
    return _case("tiny2", stored, absent, walk=dict(zip(absent, (2, 2, 1, 0))))


def _tcp_side(tag):
    """A few Active keys and strays for the UDP cases, so their waves mix both protocols."""
    stored = [akey(rip(j, tag, 11), 0x1F900000 + 0x10001 * j) for j in range(1, 5)]
    absent = [akey(rip(j, tag, 12), 0x1F910000 + 0x10001 * j) for j in range(1, 5)]
    return stored, absent


def _ubind(port, lip=CFG):
    return (UDP, lip, 0, port, 0)


def _udp_seed():
    ports = []
    for seed in (0, 1, 2):  # five ports that share one pair of buckets under this seed: four words cannot hold them
        groups = {}
        for p in range(1024, 65535):
            if p not in ports:
                groups.setdefault(ub_buckets(p, seed, 15), []).append(p)
        pair = max((k for k in groups if k[0] != k[1]), key=lambda k: (len(groups[k]), k))
        ports += groups[pair][:5]
    ports.append(65535)
    binds = [_ubind(p) for p in ports]
    ub = udp_build(udp_local_words(_arr(binds)))
    bound_pairs = {ub_buckets(p, ub.seed, ub.mask) for p in ports}
    colliding = [q for q in range(65536) if q not in ports and ub_buckets(q, ub.seed, ub.mask) in bound_pairs]
    rng = np.random.default_rng(47)
    sample = sorted(int(q) for q in rng.choice(colliding, 48, replace=False))
    tcp_stored, tcp_absent = _tcp_side(71)
    # every third colliding port has a bind on 0.0.0.0; one bound port has one too (the configured address wins)
    anys = [_ubind(q, 0) for q in sample[::3]] + [_ubind(ports[2], 0)]
    return _case("udp_seed", tcp_stored, tcp_absent + [_ubind(q) for q in sample], extra=binds + anys,
                 targets_extra=binds, ports=ports, colliding=len(colliding), sample=sample)


def _udp_fid_edge(index):
    port = 40000
    front = [_ubind(1024 + k % 60000, ELSEWHERE) for k in range(index)]  # stored nowhere: the tables stay small
    ub = udp_build(udp_local_words(_arr([_ubind(port)])))
    pair = ub_buckets(port, ub.seed, ub.mask)
    share = [q for q in range(1024, 65535) if q != port and ub_buckets(q, ub.seed, ub.mask) == pair][:6]
    half = [q for q in range(1024, 65535) if q != port and ub_buckets(q, ub.seed, ub.mask)[1] == pair[0]][:2]
    tcp_stored, tcp_absent = _tcp_side(72)
    unbound = [_ubind(q) for q in share + half + [65535, 0, 1024]]  # 65535 unbound: it equals an empty word's low half
    anys = [_ubind(q, 0) for q in share[::2]]
    return _case(f"udp_fid_edge_{index:04x}", [_ubind(port)], unbound + tcp_absent, extra=tcp_stored + anys,
                 targets_extra=tcp_stored, front=front, port=port, index=index)


BUILDERS = {
    "wrap": _wrap, "one_hash": _one_hash, "same_slot_one_field": _same_slot_one_field,
    "full_hash_miss": _full_hash_miss, "crowded_bucket": _crowded_bucket, "tiny1": _tiny1, "tiny2": _tiny2,
    "udp_seed": _udp_seed, "udp_fid_edge_fffe": lambda: _udp_fid_edge(0xFFFE),
    "udp_fid_edge_ffff": lambda: _udp_fid_edge(0xFFFF),
}
CASES = list(BUILDERS)
TCP_CASES = CASES[:7]
UDP_CASES = CASES[7:]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def tables(name):
    """The three restated structures of a case's socket table (lds, ub: None where the host refuses)."""
    c = case(name)
    slots = global_place(c.flows)
    return SimpleNamespace(slots=slots, lds=lds_build(slots), ub=udp_build(udp_local_words(c.flows)))


@functools.lru_cache(maxsize=None)
def depths(name):
    """Per target: its outcome (see `outcome`) and, for TCP targets, the occupied slots the global probe visits before
    it answers (a hit's depth in its chain, a miss's walk to the empty slot)."""
    c, t = case(name), tables(name)
    out, keys = [], set(rows(c.flows))
    for row in rows(c.targets):
        steps = global_lookup(t.slots, row[1], row[2], row[3] | row[4] << 16)[1] if row[0] == ACTIVE else 0
        out.append((outcome(keys, CFG, row), steps))
    return out


def wave_groups(name):
    """Target indices for the three whole waves that follow the random draw: for the Active cases hits at depth 0, hits
    at the deepest chain entry and misses with the longest walk; for the UDP cases bind hits, unbound ports with a
    bind on 0.0.0.0 and unbound ports with none."""
    d = depths(name)
    if name in UDP_CASES:
        return [[k for k, (o, _) in enumerate(d) if o == want] for want in ("bind", "any", "udp_nosock")]
    hits = [(k, s) for k, (o, s) in enumerate(d) if o == "active"]
    miss = [(k, s) for k, (o, s) in enumerate(d) if o in ("listener", "tcp_nosock")]
    deep, far = max(s for _, s in hits), max(s for _, s in miss)
    return [[k for k, s in hits if s == 0], [k for k, s in hits if s == deep], [k for k, s in miss if s == far]]


@functools.lru_cache(maxsize=None)
def frames(name, small):
    """The case as N_FRAMES frames with valid checksums: targets drawn at random (the lanes of one wave need different
    walk depths), then three whole waves of one kind each (wave_groups). small: 64-byte frames for the small-frame
    kernel, else frame lengths drawn from 64..1514. A UDP target with a remote address is sent from that address and
    port. Returns the blob, its descriptors, the header fields the model needs and the target of each frame."""
    c = case(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    idx = [rng.integers(0, len(c.targets), N_FRAMES - 3 * WAVE)]
    idx += [rng.choice(np.asarray(g), WAVE) for g in wave_groups(name)]
    idx = np.concatenate(idx).astype(np.int64)
    ip_len = np.full(N_FRAMES, 50, np.uint16) if small else rng.integers(50, 1501, N_FRAMES).astype(np.uint16)
    tr = synth.traffic(N_FRAMES, ip_len, c.targets, seed=int(rng.integers(1 << 30)))
    t = c.targets[idx]
    tcp = t["kind"] == ACTIVE
    named = tcp | (t["remote_ip"] != 0)
    tr.proto = np.where(tcp, 6, 17).astype(np.uint8)
    tr.src_ip = np.where(named, t["remote_ip"], tr.src_ip).astype(np.uint32)
    tr.sport = np.where(named, t["remote_port"], tr.sport).astype(np.uint16)
    tr.dport = t["local_port"].astype(np.uint16)
    tr.flow = idx
    blob, off, lens = synth.build_numpy(tr)
    out = SimpleNamespace(blob=blob, off=off, lens=lens, proto=tr.proto, src_ip=tr.src_ip, sport=tr.sport,
                          dport=tr.dport, idx=idx, n=N_FRAMES)
    for v in vars(out).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(name, small):
    """model() on the case's frames: (flow id, verdict) per frame."""
    f = frames(name, small)
    return model(case(name).flows, CFG, f.proto, f.src_ip, f.sport, f.dport)


# ---------------------------------------------------------------------------------------------------------------------
# the demux over the restated structures (and its deliberately wrong variants)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _port_side(name):
    """The port table of a case: local binds, binds on 0.0.0.0 and listeners by port."""
    c = case(name)
    anyw, pas = {}, {}
    for i, (kind, lip, _, lp, _) in enumerate(rows(c.flows)):
        if kind == UDP and lip == 0:
            anyw[lp] = i
        if kind == PASSIVE and lip == CFG:
            pas[lp] = i
    return udp_local_words(c.flows), anyw, pas


def restated_demux(name, small, active="global", binds="port", **wrong):
    """(flow id, verdict) per frame of the case as the kernels compute it, over the restated tables: Active keys in the
    global table or the LDS copy, local binds in the port table or the compact table; listeners and binds on 0.0.0.0
    from the port table. `wrong` passes a mutation's switches to the lookup it belongs to: wrap, max_steps, cmp_rip,
    cmp_ports (global); compare, disp_bits, cmp_rip, cmp_ports (LDS); seed, first_only, accept_ffff (compact bind
    table)."""
    c, t, f = case(name), tables(name), frames(name, small)
    gl = {k: wrong[k] for k in ("wrap", "max_steps", "cmp_rip", "cmp_ports") if k in wrong}
    ld = {k: wrong[k] for k in ("compare", "disp_bits", "cmp_rip", "cmp_ports") if k in wrong}
    ub = {k: wrong[k] for k in ("first_only", "accept_ffff") if k in wrong}
    local, anyw, pas = _port_side(name)
    fid = np.full(f.n, NONE, np.uint32)
    v = np.zeros(f.n, np.uint32)
    for k, (p, s, sp, dp) in enumerate(zip(f.proto.tolist(), f.src_ip.tolist(), f.sport.tolist(), f.dport.tolist())):
        if p == 6:
            ports = dp | sp << 16
            if active == "lds":
                x = lt_lookup(t.lds.words, t.lds.n, t.lds.nb, CFG, s, ports, **ld)
            else:
                x = global_lookup(t.slots, CFG, s, ports, **gl)[0]
            x = pas.get(dp) if x is None else x
            v[k] = N.V["TCP_NOSOCK"] if x is None else N.V["OK_TCP"]
        else:
            if binds == "compact":
                x = ub_lookup(t.ub.words, t.ub.mask, wrong.get("seed", t.ub.seed), dp, **ub)
            else:
                x = None if local[dp] == NONE else int(local[dp])
            x = anyw.get(dp) if x is None else x
            v[k] = N.V["UDP_NOSOCK"] if x is None else N.V["OK_UDP"]
        if x is not None:
            fid[k] = x
    return fid, v
