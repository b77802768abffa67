"""Shared ARP scenarios for tests/test_arp_model.py (the model on the CPU) and tests/test_gpu_arp.py (the device against
the model). A Case is a peer (its cfg, its initial cache, its query rows and links) and a list of steps; the frames are
built with the arp() builder of tests/control_frames.py. Pure Python + numpy."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import arp_reference as R
import control_frames as CF
import frames as F
from demikernel_amd import _native as N
from demikernel_amd.rx import ipv4

ALICE, BOB, CARRIE = "192.168.1.1", "192.168.1.2", "192.168.1.3"
ALICE_MAC, BOB_MAC = F.ALICE_MAC, F.BOB_MAC
CARRIE_MAC = bytes([0xEF, 0xCD, 0xAB, 0x89, 0x67, 0x45])
MACS = {ALICE: ALICE_MAC, BOB: BOB_MAC, CARRIE: CARRIE_MAC}
SEC = 1_000_000_000
TTL = 10 * SEC


def mac_of(k: int) -> bytes:
    return bytes([0x02, 0xAA, (k >> 24) & 0xFF, (k >> 16) & 0xFF, (k >> 8) & 0xFF, k & 0xFF])


def host(k: int) -> str:
    """An address outside the three named ones."""
    return f"10.{(k >> 16) & 0xFF}.{(k >> 8) & 0xFF}.{k & 0xFF}"


def req(spa, tpa, sha=None, name="q") -> CF.Ctl:
    return CF.arp(name, op=1, sha=MACS.get(spa, mac_of(ipv4(spa))) if sha is None else sha, spa=spa, tha=(0xFF,) * 6, tpa=tpa)


def rep(spa, tpa, sha=None, tha=(0,) * 6, name="r") -> CF.Ctl:
    return CF.arp(name, op=2, sha=MACS.get(spa, mac_of(ipv4(spa))) if sha is None else sha, spa=spa, tha=tha, tpa=tpa)


def model_frames(frames) -> list:
    """What dk_arp_process reads of each frame (a Ctl, or raw bytes of a frame that is not ARP)."""
    out = []
    for c in frames:
        if isinstance(c, CF.Ctl) and c.verdict == "ARP":
            out.append(R.Frame(True, c.hi >> 8, c.frame[22:28], c.src_ip, c.dst_ip))
        else:
            out.append(R.Frame(False))
    return out


def raw(c) -> bytes:
    return c.frame if isinstance(c, CF.Ctl) else c


def links_of(k: int) -> np.ndarray:
    """k dk_tx_link rows with recognisable bytes everywhere, so an untouched field shows."""
    a = np.zeros(k, N.TX_LINK_DTYPE)
    for j in range(k):
        a[j]["dst_mac"] = np.arange(6) + 0x10 * (j + 1)
        a[j]["src_mac"] = np.arange(6) + 0x10 * (j + 1) + 8
        a[j]["reserved"] = 0xC0DE0000 + j
    return a


def waiting(ips, now=0, timeout=SEC, links=None, tags=None) -> np.ndarray:
    """Query rows as dk_arp_query_start leaves them after a miss."""
    t = np.zeros(len(ips), N.ARP_QUERY_DTYPE)
    t["ip"] = [ipv4(a) for a in ips]
    t["link"] = R.NO_LINK if links is None else links
    t["tag"] = 100 + np.arange(len(ips)) if tags is None else tags
    t["state"], t["sent"], t["deadline_ns"] = R.WAITING, 1, now + timeout
    return t


def idle(ips, links=None) -> np.ndarray:
    t = waiting(ips, links=links)
    t["state"], t["sent"], t["deadline_ns"] = R.IDLE, 0, 0
    return t


@dataclass
class Case:
    name: str
    local: str = ALICE
    cap: int = 64
    ttl: int = TTL
    timeout: int = SEC
    retries: int = 2
    disabled: bool = False
    initial: list = field(default_factory=list)  # (ip string, mac) pairs inserted at clock `initial_clock`
    initial_clock: int = 0
    rows: np.ndarray = None
    links: np.ndarray = None
    steps: list = field(default_factory=list)    # ("process", frames, clock, kw) | ("start", start, now, kw) |
                                                 # ("timers", now, kw) | ("lookup", ips, link) | ("insert", pairs, clock)

    def model(self) -> R.ArpModel:
        m = R.ArpModel(ipv4(self.local), MACS[self.local], cap=self.cap, cache_ttl_ns=self.ttl,
                       request_timeout_ns=self.timeout, retry_count=self.retries, disabled=self.disabled, rows=self.rows,
                       links=self.links, clock=self.initial_clock)
        m.insert_initial([(ipv4(a), mac) for a, mac in self.initial], self.initial_clock)
        return m


def run_model(case: Case):
    """The model through the case's steps: (model, [each step's result])."""
    m, outs = case.model(), []
    for st in case.steps:
        if st[0] == "process":
            outs.append(m.process(model_frames(st[1]), st[2], **st[3]))
        elif st[0] == "start":
            outs.append(m.start(st[1], st[2], **st[3]))
        elif st[0] == "timers":
            outs.append(m.timers(st[1], **st[2]))
        elif st[0] == "lookup":
            outs.append(m.lookup([ipv4(a) for a in st[1]], st[2]))
        elif st[0] == "insert":
            m.insert_initial([(ipv4(a), mac) for a, mac in st[1]], st[2])
            outs.append(None)
    return m, outs


# ---- the reference's own four scenarios (arp/tests.rs) ---------------------------------------------------------------
def immediate_reply():
    return Case("immediate_reply", local=ALICE, steps=[("process", [req(BOB, ALICE)], 1000, {})])


def no_reply():
    return Case("no_reply", local=ALICE, steps=[("process", [req(BOB, CARRIE)], 1000, {})])


def cache_update():
    return Case("cache_update", local=BOB, steps=[("process", [req(CARRIE, BOB)], 1000, {})])


def query_timeout():
    return Case("query_timeout", local=ALICE, retries=2, timeout=SEC, rows=idle([CARRIE]),
                steps=[("start", [0], 0, {})] + [("timers", k * SEC, {}) for k in (1, 2, 3, 4)])


# ---- the cache's clock -----------------------------------------------------------------------------------------------
def expired_still_answers():
    """An expired entry answers get until the next insert: a batch with no f0 cleans nothing up."""
    return Case("expired_still_answers", initial=[(BOB, BOB_MAC)], rows=idle([BOB, CARRIE], links=[0, 1]), links=links_of(2),
                steps=[("process", [req(host(1), host(2))], 2 * TTL, {}), ("lookup", [BOB, CARRIE], [1, 0]),
                       ("start", [0, 1], 5, {})])


def first_insert_cleans_others():
    """The first insert of a batch removes the expired entries of other keys, exactly at clock == expiration."""
    return Case("first_insert_cleans_others", initial=[(BOB, BOB_MAC), (CARRIE, CARRIE_MAC)],
                steps=[("process", [req(host(1), host(2)), rep(host(3), ALICE)], TTL, {}), ("lookup", [BOB, CARRIE, host(3)], None)])


def one_tick_early():
    """At clock == expiration - 1 nothing leaves."""
    return Case("one_tick_early", initial=[(BOB, BOB_MAC)],
                steps=[("process", [rep(host(3), ALICE)], TTL - 1, {})])


def f0_expired_hit():
    """f0's own hit test still sees an expired entry; a later frame of another expired key does not."""
    return Case("f0_expired_hit", initial=[(BOB, BOB_MAC), (CARRIE, CARRIE_MAC)],
                steps=[("process", [req(BOB, host(9), sha=mac_of(7)), req(CARRIE, host(9)), req(BOB, host(9), sha=mac_of(8))],
                        TTL + 5, {})])


def reply_to_us_unknown():
    return Case("reply_to_us_unknown", steps=[("process", [rep(BOB, ALICE, tha=ALICE_MAC)], 7, {})])


def reply_other_unknown():
    return Case("reply_other_unknown", steps=[("process", [rep(BOB, CARRIE, tha=CARRIE_MAC)], 7, {})])


def first_waking_mac():
    """A row keeps the first waking MAC while the cache ends with the second."""
    return Case("first_waking_mac", rows=waiting([BOB], links=[1]), links=links_of(2),
                steps=[("process", [rep(BOB, ALICE, sha=mac_of(1)), rep(BOB, ALICE, sha=mac_of(2))], 3, {})])


def disabled():
    return Case("disabled", disabled=True, rows=np.concatenate([idle([CARRIE], links=[0]), waiting([BOB])]), links=links_of(1),
                steps=[("start", [0], 0, {}), ("process", [req(BOB, ALICE), req(host(1), host(2)), rep(BOB, host(2))], 1, {}),
                       ("lookup", [BOB, host(5)], [0, R.NO_LINK])])


def timers_lookup_resolves():
    """The cache look after the re-send resolves the row although its frame still goes out."""
    return Case("timers_lookup_resolves", rows=waiting([BOB, CARRIE], links=[0, R.NO_LINK]), links=links_of(1),
                steps=[("insert", [(BOB, BOB_MAC)], 0), ("timers", SEC, {})])


MODEL_CASES = [immediate_reply, no_reply, cache_update, query_timeout, expired_still_answers, first_insert_cleans_others,
               one_tick_early, f0_expired_hit, reply_to_us_unknown, reply_other_unknown, first_waking_mac, disabled,
               timers_lookup_resolves]


# ---- shapes for the device -------------------------------------------------------------------------------------------
def empty_and_one():
    return Case("empty_and_one", steps=[("process", [], 1, {}), ("process", [req(BOB, ALICE)], 1, {}),
                                        ("start", [], 1, {}), ("timers", 1, {})])


def second_wave(f0_at_64: bool):
    """65 covered frames of 63 senders; two frames of one sender with different sha at positions 63 and 64. With
    f0_at_64 nothing before position 64 has an entry or is addressed to us."""
    tpa = host(900) if f0_at_64 else ALICE
    fr = [req(host(k + 1), tpa) for k in range(63)]
    fr += [req(host(500), tpa, sha=mac_of(63)), rep(host(500), ALICE, sha=mac_of(64))]
    return Case(f"second_wave_f0_{64 if f0_at_64 else 0}", cap=256, rows=waiting([host(500), host(3)], links=[0, 1]),
                links=links_of(2), steps=[("process", fr, 5, {}), ("lookup", [host(500), host(3)], None)])


def past_one_workgroup():
    """257 covered frames (one more than a workgroup of lanes) with repeated senders in both halves."""
    fr = []
    for k in range(257):
        s = host(1 + k % 100)
        fr.append(req(s, ALICE if k % 3 == 0 else host(2000 + k), sha=mac_of(k)) if k % 2 else
                  rep(s, ALICE if k % 5 == 0 else host(2000 + k), sha=mac_of(k)))
    return Case("past_one_workgroup", cap=512, initial=[(host(7), mac_of(7000)), (host(8), mac_of(8000))],
                rows=waiting([host(1 + k) for k in range(0, 120, 7)]), steps=[("process", fr, TTL, {})])


def interleaved():
    """ARP frames among TCP, UDP, ICMP, ARP_SHORT and ARP_UNSUP frames, which get SKIP and leave no trace."""
    other = [F.tcp_frame(b"abc"), F.udp_frame(b"xyz"), CF.icmp("echo", p=8),
             CF.arp("short", "ARP_SHORT", cut=14 + 27, spa=host(77), tpa=ALICE),
             CF.arp("unsup", "ARP_UNSUP", op=3, spa=host(78), tpa=ALICE)]
    fr = []
    for k in range(12):
        fr.append(other[k % len(other)])
        fr.append(req(host(1 + k % 4), ALICE if k % 2 else BOB, sha=mac_of(k)))
    return Case("interleaved", local=BOB, rows=waiting([host(77), host(78), host(2)]),
                steps=[("process", fr, 9, {}), ("lookup", [host(77), host(78), host(1), host(2)], None)])


def many_waiters():
    """Many WAITING rows on one address woken by one frame; rows on several addresses woken by different frames."""
    ips = [host(5)] * 70 + [host(6), host(7), host(5), host(6), host(99)]
    rows = waiting(ips, links=[k % 3 for k in range(len(ips))])
    rows["link"][:70] = 0
    rows["link"][70:] = [1, 2, 0, 1, R.NO_LINK]
    fr = [rep(host(7), ALICE), req(host(6), ALICE), rep(host(1), host(2)), rep(host(5), ALICE), rep(host(6), ALICE, sha=mac_of(1))]
    return Case("many_waiters", rows=rows, links=links_of(3), steps=[("process", fr, 2, {})])


def random_case(seed: int):
    """Two random batches of 300 frames over 60 senders, of which 10 have an expired entry at the first clock and 10 a
    live one; a third of the frames are addressed to us, and the batch opens with frames that neither hit nor are
    local. 30 WAITING rows, one link per address. The second clock expires everything the first call left."""
    rng = np.random.default_rng(seed)
    hosts = [host(1 + k) for k in range(60)]

    def batch(n, lead):
        fr = [req(hosts[40 + int(rng.integers(20))], host(9000 + k), sha=mac_of(70000 + k)) for k in range(lead)]
        for k in range(n - lead):
            s, local = hosts[int(rng.integers(60))], rng.random() < 0.33
            fr.append((req if rng.random() < 0.5 else rep)(s, ALICE if local else host(9000 + k), sha=mac_of(1000 * seed + k)))
        return fr

    who = rng.integers(60, size=30)
    rows = waiting([hosts[int(w)] for w in who], links=[int(w) if w % 3 else R.NO_LINK for w in who])
    return Case(f"random_{seed}", cap=256, rows=rows, links=links_of(60),
                steps=[("insert", [(hosts[k], mac_of(k)) for k in range(10)], 0),
                       ("insert", [(hosts[k], mac_of(k)) for k in range(10, 20)], TTL // 2),
                       ("process", batch(300, 5), TTL + 1, {}), ("lookup", hosts, None),
                       ("process", batch(300, 0), 3 * TTL, {}), ("lookup", hosts, None)])


DEVICE_CASES = [empty_and_one, lambda: second_wave(False), lambda: second_wave(True), past_one_workgroup, interleaved,
                many_waiters, lambda: random_case(1), lambda: random_case(2), lambda: random_case(3)]
