"""ICMPv4 and ARP frames for the receive kernels, each with the record it must produce, written down from the
builder's arguments and the packing rules of include/dk_rx.h (never read back from the oracle or a kernel):

  ICMP:  meta = 3 | 1 << 8 | type << 16 | code << 24, src_ip / dst_ip of the IPv4 header, ports = id | seq << 16,
         payload = (S + 8) | (E - S - 8) << 16 with S = 14 + IHL * 4 and E = 14 + total_length
         (icmpv4/header.rs:47-66: length, then the checksum over [S, E) folding to zero, then the type byte;
         protocols/mod.rs:47-71 for the sum)
  ARP:   meta = 2 | operation << 16, src_ip / dst_ip = sender / target protocol address,
         payload = 14 | (len - 14) << 16  (arp/header.rs:80-111)
  every other verdict: all fields zero; every control frame: flow_id = DK_FLOW_NONE.

`icmp_ladder` puts the ICMP message at every size-class boundary of rx_kernels.hip (the constants are parsed from
the source, kernel_constants), `arp_set` is the ARP side, `control_mix` splices both into synth TCP/UDP traffic so the
batch's mean size picks the kernel family. Pure Python + numpy: nothing here touches the GPU library.
"""
from __future__ import annotations

import functools
import os
import random
import re
from dataclasses import dataclass

import numpy as np

import frames as F
from demikernel_amd import synth
from demikernel_amd.rx import ipv4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DK_FLOW_NONE = 0xFFFFFFFF
# enum dk_verdict (include/dk_rx.h) of the seven control-plane verdicts
CODES = {"ARP": 2, "ICMP": 3, "ARP_SHORT": 34, "ARP_UNSUP": 35, "ICMP_SHORT": 36, "ICMP_CSUM": 37, "ICMP_TYPE": 38}
CONTROL_VERDICTS = tuple(CODES)
# Icmpv4Type2::parse (icmpv4/protocol.rs:35-58)
ICMP_ACCEPTED = (0, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14)
ICMP_REJECTED = (1, 2, 6, 7, 15, 16, 255)
CLASSES = ("window", "medium", "large", "multi")
FIELDS = ("meta", "src_ip", "dst_ip", "ports", "payload", "flow_id")


def kernel_constants() -> dict:
    """Size-class boundaries of demikernel_amd/csrc/rx_kernels.hip in bytes from the frame's granule base (sh + len):
    window: RegAcc::w, the 64-byte register window (frames of sh + len <= window are never streamed);
    med:    16 bytes * kMedGran = 16 * 16 * DK_COOP_MED_U, the medium step shape's span;
    span:   16 bytes * kCoopSpan = 16 * 16 * DK_COOP_U, one quarter-wave iteration (longer frames take several);
    resum:  seg_sum_fast re-sums the segment in-lane when E lies more than this many bytes before the end of the
            frame's last granule."""
    with open(os.path.join(ROOT, "demikernel_amd", "csrc", "rx_kernels.hip")) as fh:
        src = fh.read()

    def macro(name):
        return int(re.search(rf"^#define {name} (\d+)", src, re.M).group(1))

    words = int(re.search(r"struct RegAcc \{\s*uint32_t w\[(\d+)\];", src).group(1))
    assert re.search(r"kCoopSpan = 16 \* kCoopU;", src) and re.search(r"kCoopU = DK_COOP_U;", src)
    assert re.search(r"kMedGran = DK_COOP_MED_U > 0 \? 16 \* kMedU : 0;", src)
    resum = int(re.search(r"\(int\)\(16 \* C\.nblk - C\.sh\) - E <= (\d+)\)", src).group(1))
    return {"window": 4 * words, "med": 16 * 16 * macro("DK_COOP_MED_U"), "span": 16 * 16 * macro("DK_COOP_U"),
            "resum": resum}


K = kernel_constants()


@dataclass(frozen=True)
class Ctl:
    """One control-plane frame and what it must produce."""

    name: str
    frame: bytes
    verdict: str
    kind: str             # "icmp" or "arp"
    hi: int = 0           # meta bits 8..31
    src_ip: int = 0
    dst_ip: int = 0
    ports: int = 0
    payload: int = 0
    ihl: int = 5
    E: int = 0            # ICMP: 14 + total_length
    summed: bool = False  # ICMP: the message is >= 8 bytes, so its checksum is computed
    tags: tuple = ()

    @property
    def meta(self) -> int:
        return CODES[self.verdict] | self.hi << 8


def size_class(sh: int, ln: int) -> str:
    span = sh + ln
    return "window" if span <= K["window"] else "medium" if span <= K["med"] else "large" if span <= K["span"] \
        else "multi"


def path(c: Ctl, sh: int, aligned16: bool = False) -> int:
    """The dk_diag.h path counter a frame at offset sh mod 16 adds to: 0 in the register window, 1 streamed,
    2 streamed with the segment re-summed in-lane, 3 byte path (odd address, or any address but 0 mod 16 under the
    DK_RX_BATCH_ALIGNED16 hint; ARP; IHL != 5; shorter than the fixed headers)."""
    ln = len(c.frame)
    if sh % 2 or (aligned16 and sh) or c.kind == "arp" or ln < 34 or c.ihl != 5:
        return 3
    if sh + ln <= K["window"]:
        return 0
    last_granule_end = (sh + ln + 15) // 16 * 16 - sh  # frame-relative
    return 2 if c.summed and last_granule_end - c.E > K["resum"] else 1


def path_counts(ctls, sh: int, aligned16: bool = False) -> list:
    out = [0, 0, 0, 0]
    for c in ctls:
        out[path(c, sh, aligned16)] += 1
    return out


def census(ctls, shifts=(0,)) -> dict:
    """{(verdict, size class): frames} over the given offsets mod 16."""
    out = {}
    for sh in shifts:
        for c in ctls:
            k = (c.verdict, size_class(sh, len(c.frame)))
            out[k] = out.get(k, 0) + 1
    return out


def can_occur(verdict: str, cls: str) -> bool:
    """Ethernet padding carries any control frame into any size class, except an ARP PDU of < 28 bytes (the frame is
    then < 42 bytes)."""
    return cls == "window" if verdict == "ARP_SHORT" else True


def expected(ctls) -> dict:
    out = {k: np.array([getattr(c, k) for c in ctls], np.uint32) for k in FIELDS[:-1]}
    out["flow_id"] = np.full(len(ctls), DK_FLOW_NONE, np.uint32)
    return out


def assert_control(res: dict, idx, ctls, ctx: str = "") -> None:
    """Every field of every control frame of `res` (arrays over the whole batch; dst_ip may be absent) equals the
    construction's."""
    exp = expected(ctls)
    idx = np.asarray(idx, np.int64)
    assert len(idx) == len(ctls)
    for k in FIELDS:
        if k not in res:
            assert k == "dst_ip", k
            continue
        got = np.asarray(res[k])[idx]
        bad = np.nonzero(got != exp[k])[0]
        if bad.size:
            j = int(bad[0])
            raise AssertionError(f"{ctx}: '{k}' of control frame {ctls[j].name} (batch index {int(idx[j])}, built "
                                 f"{ctls[j].verdict}): got {int(got[j]):#x} want {int(exp[k][j]):#x}; "
                                 f"{bad.size} frames differ")


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
def icmp(name, p=0, type_=8, code=0, ident=0x1234, seq=1, payload=None, checksum=None, pad=0, ihl=5, corrupt=None,
         tags=(), rng=None) -> Ctl:
    """An ICMPv4 message of p payload bytes behind Ethernet + IPv4 (IHL words; options are NOPs) with `pad` bytes of
    Ethernet padding after total_length. corrupt: one bit flipped in the "last" / "first" payload byte or the
    checksum "field" (-> ICMP_CSUM), or in the "pad" (outside [S, E): the verdict stays)."""
    if payload is None:
        payload = (rng or random.Random(p)).randbytes(p)
    S = 14 + 4 * ihl
    E = S + 8 + len(payload)
    f = bytearray(F.icmp_frame(type_, code, ident, seq, payload, checksum, ip_options=bytes([1]) * (4 * (ihl - 5)),
                               pad=pad))
    assert len(f) == E + pad
    if corrupt is not None:
        pos = {"last": E - 1, "first": S + 8, "field": S + 3, "pad": E + pad // 2}[corrupt]
        assert (S + 8 <= pos < E) if corrupt in ("last", "first") else (E <= pos < len(f)) if corrupt == "pad" else True
        f[pos] ^= 0x10
    if corrupt in ("last", "first", "field"):
        verdict = "ICMP_CSUM"       # icmpv4/header.rs:55-57, before the type byte is looked at
    else:
        verdict = "ICMP" if type_ in ICMP_ACCEPTED else "ICMP_TYPE"
    rec = {}
    if verdict == "ICMP":
        rec = dict(hi=1 | type_ << 8 | code << 16, src_ip=ipv4(F.ALICE_IPV4), dst_ip=ipv4(F.BOB_IPV4),
                   ports=ident | seq << 16, payload=(S + 8) | (E - S - 8) << 16)
    return Ctl(name, bytes(f), verdict, "icmp", ihl=ihl, E=E, summed=True, tags=tuple(tags), **rec)


def icmp_short(name, seg, pad=0, tags=()) -> Ctl:
    """An ICMPv4 message of seg < 8 bytes (icmpv4/header.rs:48-50)."""
    assert seg < 8
    f = F.frame(F.icmp_message()[:seg], proto=1, pad=pad)
    return Ctl(name, f, "ICMP_SHORT", "icmp", E=34 + seg, tags=tuple(tags))


def arp(name, verdict="ARP", op=1, spa=F.ALICE_IPV4, tpa=F.BOB_IPV4, pad=0, cut=None, tags=(), **kw) -> Ctl:
    f = F.arp_frame(op=op, spa=spa, tpa=tpa, pad=pad, **kw)
    if cut is not None:
        f = f[:cut]
    rec = {}
    if verdict == "ARP":
        rec = dict(hi=op << 8, src_ip=ipv4(spa), dst_ip=ipv4(tpa), payload=14 | (len(f) - 14) << 16)
    return Ctl(name, f, verdict, "arp", tags=tuple(tags), **rec)


def icmp_ladder(seed: int = 1) -> list:
    """The ladder described at _icmp_ladder (built once per seed; a fresh list of the same frozen records)."""
    return list(_icmp_ladder(seed))


@functools.lru_cache(maxsize=None)
def _icmp_ladder(seed: int) -> tuple:
    """ICMP messages at every size-class boundary of the kernels (frame length 42 + p for IHL 5), each boundary B
    (window, med, span of kernel_constants) at sh + len = B - 1, B, B + 1 for sh = 0 and 2, E == 64 exactly (the
    wave-uniform sum form), two whole stream iterations, 9,000 bytes, p = 0 and 1, and per size class: odd p, Ethernet
    padding of 1 / 16 / 17 / 40 bytes, IHL 6 and 15, an all-0xFF payload, the all-zero echo reply with checksum field
    0 and 0xFFFF (both accepted: the word sum is 0 mod 0xFFFF), one flipped bit in the last / first payload byte and
    in the checksum field, one in the padding (still ICMP), every accepted and seven rejected type bytes, and
    ICMP_SHORT at segment lengths 0 and 7."""
    rng = random.Random(seed)
    L = []

    def add(name, **kw):
        L.append(icmp(name, rng=rng, **kw))

    for key in ("window", "med", "span"):
        B = K[key]
        for sh in (0, 2):
            for d in (-1, 0, 1):
                add(f"bound_{key}_sh{sh}_{d:+d}", p=B - sh + d - 42, tags=(("bound", key, sh, d),))
    for d in (-1, 0, 1):  # E == window exactly: no byte of the window's last dword is masked
        add(f"E_window_{d:+d}", p=K["window"] - 42 + d, tags=(("E", d),))
    for sh in (0, 2):
        add(f"two_iterations_sh{sh}", p=2 * K["span"] - sh - 42, tags=(("two_iter", sh),))
    add("jumbo_9000", p=9000 - 42, tags=("jumbo",))
    add("jumbo_9000_odd", p=9001 - 42)
    add("jumbo_9000_bad_last", p=9000 - 42, corrupt="last")
    add("jumbo_9000_pad17", p=9000 - 42 - 17, pad=17)
    add("jumbo_9000_pad40_odd", p=9001 - 42 - 40, pad=40)
    add("jumbo_9000_ihl15", p=9000 - 82, ihl=15)
    add("p0", p=0)
    add("p1", p=1)
    # frames whose message ends inside the window but whose padding carries them past it
    for p, pad in ((22, 1), (22, 2), (22, 16), (22, 17), (10, 13), (10, 20), (0, 23), (1, 40), (4, 14),
                   (10, K["span"] - 100), (11, 2 * K["span"])):
        add(f"E_in_window_p{p}_pad{pad}", p=p, pad=pad, tags=("pad_past_window",))
    add("E_in_window_bad_p10_pad20", p=10, pad=20, corrupt="last")
    add("E_in_window_padflip_p22_pad16", p=22, pad=16, corrupt="pad")
    # one representative even payload length per size class (the odd one is p + 1), clear of the boundaries
    reps = {"window": 8, "medium": (K["window"] + K["med"]) // 2 - 42 & ~1, "large": (K["med"] + K["span"]) // 2 - 42 & ~1,
            "multi": K["span"] + 1000 & ~1}
    for cls, p in reps.items():
        assert size_class(2, 42 + p + 1) == cls == size_class(0, 42 + p)
        add(f"{cls}_even", p=p)
        add(f"{cls}_odd", p=p + 1)
        for pad in (1, 16, 17, 40):
            # keep the padded window frames in the window where they fit: p shrinks by the pad
            q = max(p - pad, 0) if cls == "window" and 42 + p + pad + 3 > K["window"] else p
            add(f"{cls}_pad{pad}", p=q, pad=pad)
            add(f"{cls}_pad{pad}_odd", p=q + 1, pad=pad)
        add(f"{cls}_padflip", p=p + 1, pad=17, corrupt="pad")
        for ihl in (6, 15):
            add(f"{cls}_ihl{ihl}", p=p, ihl=ihl)
            add(f"{cls}_ihl{ihl}_odd", p=p + 1, ihl=ihl)
        add(f"{cls}_ihl6_bad_last", p=p + 1, ihl=6, corrupt="last")
        add(f"{cls}_ff", p=p, payload=b"\xff" * p)
        add(f"{cls}_ff_odd", p=p + 1, payload=b"\xff" * (p + 1))
        add(f"{cls}_zero_reply_field0", p=p, type_=0, ident=0, seq=0, payload=bytes(p), checksum=0)
        add(f"{cls}_zero_reply_fieldffff", p=p, type_=0, ident=0, seq=0, payload=bytes(p), checksum=0xFFFF)
        add(f"{cls}_bad_last", p=p, corrupt="last")
        add(f"{cls}_bad_last_odd", p=p + 1, corrupt="last")
        add(f"{cls}_bad_first", p=p, corrupt="first")
        add(f"{cls}_bad_field", p=p + 1, corrupt="field")
        add(f"{cls}_bad_last_pad17", p=p, pad=17, corrupt="last")
        for t in ICMP_ACCEPTED + ICMP_REJECTED:
            add(f"{cls}_type{t}", p=p + 1, type_=t, code=t & 7, ident=0x100 + t, seq=0xFF00 | t)
        for seg in (0, 7):
            L.append(icmp_short(f"{cls}_short{seg}", seg, pad=0 if cls == "window" else 42 + p - 34 - seg))
    L.append(icmp_short("short7_eth_min", 7, pad=60 - 41))
    names = [c.name for c in L]
    assert len(set(names)) == len(names)
    return tuple(L)


def arp_set() -> list:
    """Request, reply, padded to 60 and to 1,500 bytes (and into the medium and multi-iteration classes), 27-byte
    and empty PDUs, and each of HTYPE, PTYPE, HLEN, PLEN and the operation wrong on its own."""
    med, multi = (K["window"] + K["med"]) // 2, K["span"] + 1000
    L = [arp("arp_request"),
         arp("arp_reply", op=2, sha=F.BOB_MAC, spa=F.BOB_IPV4, tha=F.ALICE_MAC, tpa=F.ALICE_IPV4),
         arp("arp_request_other", spa="10.1.2.3", tpa="172.16.5.9"),
         arp("arp_pad60", pad=60 - 42),
         arp("arp_pad_medium", op=2, spa="10.9.8.7", pad=med - 42),
         arp("arp_pad1500", pad=1500 - 42),
         arp("arp_pad_multi", op=2, tpa="10.0.0.1", pad=multi - 42),
         arp("arp_pdu27", "ARP_SHORT", cut=14 + 27),
         arp("arp_pdu0", "ARP_SHORT", cut=14)]
    bad = dict(htype=dict(htype=6), ptype=dict(ptype=0x86DD), hlen=dict(hlen=8), plen=dict(plen=16), op3=dict(op=3),
               op0=dict(op=0))
    for k, kw in bad.items():
        L.append(arp(f"arp_bad_{k}", "ARP_UNSUP", **kw))
    # an HTYPE whose first byte reads as an IPv4 version / IHL byte with IHL 5 (frame byte 14): only the ethertype
    # keeps such a frame off the kernels' IPv4 fast parse
    for htype in (0x4500, 0x0500):
        for pad in (0, 18, 1500 - 42):
            L.append(arp(f"arp_bad_htype_{htype:#x}_pad{pad}", "ARP_UNSUP", htype=htype, pad=pad))
    for k, pad in (("pad60", 18), ("medium", med - 42), ("pad1500", 1500 - 42), ("multi", multi - 42)):
        L.append(arp(f"arp_bad_htype_{k}", "ARP_UNSUP", htype=6, pad=pad))
        L.append(arp(f"arp_bad_op_{k}", "ARP_UNSUP", op=0x0100, pad=pad))
    return L


def splice(carrier: list, pool: list, n_ctl: int, seed: int):
    """`n_ctl` frames of `pool` (every one of them once before any repeats, in shuffled order) at random positions
    among the carrier frames, whose order is kept. Returns (frames, control positions, their Ctl, carrier positions)."""
    rng = np.random.default_rng(seed)
    n = len(carrier) + n_ctl
    idx = np.sort(rng.choice(n, size=n_ctl, replace=False))
    picks = np.concatenate([rng.permutation(len(pool)) for _ in range(n_ctl // len(pool) + 1)])[:n_ctl]
    ctls = [pool[int(k)] for k in picks]
    is_ctl = np.zeros(n, bool)
    is_ctl[idx] = True
    cpos = np.nonzero(~is_ctl)[0]
    frames = [None] * n
    for j, c in zip(idx, ctls):
        frames[int(j)] = c.frame
    for j, f in zip(cpos, carrier):
        frames[int(j)] = f
    return frames, idx, ctls, cpos


def control_mix(n, carrier_ip_len, flows, seed, share=0.25, pool=None, misalign=None):
    """A synth TCP/UDP carrier batch (5 % corrupted, as the other tests build it) of IPv4 total length
    `carrier_ip_len` (a scalar, or an array whose first entries are used) with control frames spliced in at random
    positions: n frames in all, `share` of them control frames drawn from `pool` (default: the ladder and the ARP set,
    up to the carrier's largest frame, so that the carrier's size decides the mean blob bytes per frame and with it
    the kernel family). Returns blob, off, lens, the control frames' indices and their Ctl records."""
    n_ctl = int(round(n * share))
    n_car = n - n_ctl
    ip_len = np.asarray(carrier_ip_len)
    if ip_len.ndim:
        ip_len = ip_len[:n_car]
    tr = synth.traffic(n_car, ip_len, flows, seed=seed)
    blob0, off0, lens0 = synth.build_numpy(tr, seed=seed)
    synth.corrupt_numpy(blob0, off0, synth.corruption_plan(n_car, 0.05, tr, seed))
    carrier = [blob0[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(off0, lens0)]
    if pool is None:
        cap = max(int(lens0.max()), K["window"])
        pool = [c for c in icmp_ladder() + arp_set() if len(c.frame) <= cap]
    frames, idx, ctls, _ = splice(carrier, pool, n_ctl, seed + 1)
    blob, off, lens = F.pack(frames, misalign=misalign)
    return blob, off, lens, idx, ctls
