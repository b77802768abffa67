"""TCP and UDP frames whose checksums are steered to the values where the residue -> checksum map has a seam, at the
lengths where the summing kernels change path, each with the record it must produce, written down from the builder's
arguments and the packing rules of include/dk_rx.h (never read back from the oracle or a kernel), as
tests/control_frames.py does for ICMP and ARP.

  steer(rest, target): the 16-bit word w with ref_checksum(rest + w) == target. The reference's fold keeps its state in
      1..0xFFFF, so a word sum of residue m mod 0xFFFF is stored as 0xFFFF - m, and residue 0 as 0x0000 (never
      0xFFFF): m = 0 for target 0, else 0xFFFF - target, and w = (m - rest) mod 0xFFFF.
  OK_TCP:  meta = 0 | 6 << 8 | byte 13 << 16 | byte 12 << 24, ports = sport | dport << 16,
           payload = (S + 4 doff) | payload bytes << 16, tcp_win = window | urgent << 16, flow_id = 0
  OK_UDP:  meta = 1 | 17 << 8, payload = (S + 8) | payload bytes << 16, flow_id = 2       (frames.corpus_flows())
  TCP_CSUM / UDP_CSUM: meta = the verdict, every other field zero, flow_id = DK_FLOW_NONE.

The L4 checksum is steered through the last whole payload word (the fill "one_last" keeps its 0x01 in the last byte and
is steered through the first word), the IPv4 header checksum through the identification. Ethernet padding and the blob
between the frames are 0xFF bytes, so a granule summed past E, past len or in front of a misaligned frame adds
something visible. Pure Python + numpy: nothing here touches the oracle or the GPU library.
"""
from __future__ import annotations

import functools
import struct
from dataclasses import dataclass, replace

import numpy as np

import control_frames as CF
import frames as F
from demikernel_amd.rx import ipv4

K = CF.K
DK_FLOW_NONE = 0xFFFFFFFF
CODES = {"OK_TCP": 0, "OK_UDP": 1, "TCP_CSUM": 25, "UDP_CSUM": 31}  # enum dk_verdict (include/dk_rx.h)
FLOW_TCP, FLOW_UDP = 0, 2                                          # rows of frames.corpus_flows()
SPORT, TCP_DPORT, UDP_DPORT = 40000, 12345, 5000
FIELDS = ("meta", "src_ip", "dst_ip", "ports", "payload", "flow_id", "tcp_seq", "tcp_ack", "tcp_win")
FILLS = ("ff", "fffe", "ff00", "one_first", "one_last", "random")
TARGETS = (0x0000, 0x0001, 0x00FF, 0x0100, 0x7FFF, 0x8000, 0xFFFE)
IP_TARGETS = (0x0000, 0x0001, 0xFFFE)
PADS = (1, 17, 40)
SHIFTS = (0, 2, 1)
TWINS = ("stored_ffff", "udp_zero", "flip_first", "flip_last", "flip_span", "flip_pad")
# frame lengths: each boundary B at sh + len = B - 1, B, B + 1 for sh = 0, 1 and 2 (so len = B - 3 .. B + 1), two whole
# stream iterations, jumbo, and the powers of two up to the 16-bit descriptor's limit
LENGTHS = tuple(sorted({K[key] + d for key in ("window", "med", "span") for d in range(-3, 2)} |
                       {2 * K["span"], 9000, 9001, 16383, 16384, 16385, 32767, 32768, 32769, 65534, 65535}))
# the lengths that carry the full fills x targets cross: one per size class (at every offset in SHIFTS), and 65,535
CROSS = {"window": K["window"] - 2, "medium": K["med"] - 3, "large": K["span"] - 2, "multi": 9001, "max": 65535}


def steer(rest_sum_be: int, target: int) -> int:
    """The 16-bit word w such that the reference's fold of rest_sum_be + w is `target` (target != 0xFFFF, which the
    fold never gives)."""
    assert 0 <= target < 0xFFFF
    m = 0 if target == 0 else 0xFFFF - target
    w = (m - rest_sum_be) % 0xFFFF
    assert F.ref_checksum(rest_sum_be + w) == target
    return w


def be_sum(data: bytes) -> int:
    """Sum of big-endian 16-bit words, an odd last byte padded with zero: the true integer sum."""
    if len(data) % 2:
        data = bytes(data) + b"\0"
    return int(np.frombuffer(bytes(data), ">u2").sum(dtype=np.uint64)) if data else 0


def fill_bytes(fill: str, n: int, seed: int) -> bytes:
    if fill == "ff":          # every word = 0 mod 0xFFFF: accumulators at their maximum
        return b"\xff" * n
    if fill == "fffe":        # every word = -1: the residue counts the words summed
        return (b"\xff\xfe" * (n // 2 + 1))[:n]
    if fill == "ff00":        # 0xFF00, and 0x00FF on a grid one byte off: the x256 swap at full magnitude
        return (b"\xff\x00" * (n // 2 + 1))[:n]
    if fill == "one_first":
        return b"\x01" + bytes(n - 1)
    if fill == "one_last":
        return bytes(n - 1) + b"\x01"
    assert fill == "random"
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@dataclass(frozen=True)
class Vec:
    """One frame and what it must produce."""

    name: str
    frame: bytes
    proto: int
    verdict: str
    fill: str
    target: int            # the L4 checksum the frame was steered to (what `stored` holds unless a twin rewrote it)
    ip_target: int         # the IPv4 header checksum (steered, or whatever the identification gave)
    stored: int            # the L4 checksum field as the frame carries it
    ihl: int
    doff: int              # TCP data offset in words (UDP: 2)
    pad: int
    E: int                 # 14 + total_length
    P0: int                # frame offset of the payload
    spos: int              # frame offset of the steering word
    fill_word: bytes       # what the fill had there
    seq: int = 0
    ack: int = 0
    win: int = 0
    twin: str = ""
    tags: tuple = ()

    @property
    def ok(self) -> bool:
        return self.verdict in ("OK_TCP", "OK_UDP")

    @property
    def summed(self) -> bool:
        """The receive side computes the L4 sum: always for TCP, for UDP unless the field is 0 (udp/header.rs:78-82)."""
        return self.proto == 6 or self.stored != 0

    @property
    def cfield(self) -> int:
        """Frame offset of the L4 checksum field."""
        return 14 + 4 * self.ihl + (16 if self.proto == 6 else 6)

    @property
    def payload(self) -> bytes:
        return self.frame[self.P0:self.E]

    def record(self) -> dict:
        if not self.ok:
            return dict.fromkeys(FIELDS, 0) | {"meta": CODES[self.verdict], "flow_id": DK_FLOW_NONE}
        tcp = self.proto == 6
        hi = 6 | 0x18 << 8 | (self.doff << 4) << 16 if tcp else 17
        return {"meta": CODES[self.verdict] | hi << 8, "src_ip": ipv4(F.ALICE_IPV4), "dst_ip": ipv4(F.BOB_IPV4),
                "ports": SPORT | (TCP_DPORT if tcp else UDP_DPORT) << 16, "payload": self.P0 | (self.E - self.P0) << 16,
                "flow_id": FLOW_TCP if tcp else FLOW_UDP, "tcp_seq": self.seq if tcp else 0,
                "tcp_ack": self.ack if tcp else 0, "tcp_win": self.win if tcp else 0}


def l4_rest_sum(proto: int, header: bytes, payload: bytes) -> int:
    """Pseudo-header + L4 header + payload as big-endian words (the header's checksum field and whatever word is being
    steered hold zero)."""
    return F.pseudo(F.ALICE_IPV4, F.BOB_IPV4, proto, len(header) + len(payload)) + be_sum(header) + be_sum(payload)


def vector(name, proto, length, fill, target, *, ip_target=None, ihl=5, doff=5, pad=0, k=0, steered=True,
           tags=()) -> Vec:
    """A frame of `length` bytes (Ethernet padding included) accepted by the receive chain, L4 checksum == target."""
    tcp = proto == 6
    S = 14 + 4 * ihl
    hl = 4 * doff if tcp else 8
    E = length - pad
    plen = E - S - hl
    assert plen >= (3 if fill == "one_last" else 2), (name, plen)
    pay = bytearray(fill_bytes(fill, plen, k))
    sp = 0 if fill == "one_last" else (plen // 2 - 1) * 2  # the last whole word; an odd tail byte keeps the fill
    fill_word = bytes(pay[sp:sp + 2])
    pay[sp:sp + 2] = b"\0\0"
    seq, ack, win = (0x9E3779B1 * (k + 1)) & 0xFFFFFFFF, (0x85EBCA6B * (k + 3)) & 0xFFFFFFFF, (k * 7919 + 1) & 0xFFFF
    if tcp:
        hdr = struct.pack("!HHIIBBHHH", SPORT, TCP_DPORT, seq, ack, doff << 4, 0x18, win, 0, 0) + b"\x01" * (hl - 20)
    else:
        hdr = struct.pack("!HHHH", SPORT, UDP_DPORT, 8 + plen, 0)
    rest = l4_rest_sum(proto, hdr, bytes(pay))
    w = steer(rest, target) if steered else int.from_bytes(fill_word, "big")
    pay[sp:sp + 2] = struct.pack("!H", w)
    stored = F.ref_checksum(rest + w)
    assert not steered or stored == target
    hdr = hdr[:16 if tcp else 6] + struct.pack("!H", stored) + hdr[18 if tcp else 8:]
    opts = b"\x01" * (4 * (ihl - 5))
    ident = (k * 40503 + 7) & 0xFFFF
    if ip_target is not None:
        h0 = F.ipv4_header(ihl=ihl, total_length=E - 14, ident=0, proto=proto, options=opts, checksum=0)
        ident = steer(be_sum(h0[:20]), ip_target)
    ip = F.ipv4_header(ihl=ihl, total_length=E - 14, ident=ident, proto=proto, options=opts)
    ipc = int.from_bytes(ip[10:12], "big")
    assert ip_target is None or ipc == ip_target
    frame = F.eth_header() + ip + hdr + bytes(pay) + b"\xff" * pad
    assert len(frame) == length
    return Vec(name, frame, proto, "OK_TCP" if tcp else "OK_UDP", fill, target if steered else stored, ipc, stored, ihl,
               doff if tcp else 2, pad, E, S + hl, S + hl + sp, fill_word, seq, ack, win, tags=tuple(tags))


def twin(v: Vec, kind: str):
    """v with one change, and the verdict it must then produce; None where the kind does not apply to v."""
    f = bytearray(v.frame)
    bad = "TCP_CSUM" if v.proto == 6 else "UDP_CSUM"
    kw = {}
    if kind == "stored_ffff":       # RFC 1071's other zero on a zero-residue segment: the reference rejects it
        if v.stored != 0:
            return None
        f[v.cfield:v.cfield + 2] = b"\xff\xff"
        kw = dict(verdict=bad, stored=0xFFFF)
    elif kind == "udp_zero":        # "no checksum" over a payload whose true checksum is not 0: not verified
        if v.proto != 17 or v.stored == 0:
            return None
        f[v.cfield:v.cfield + 2] = b"\0\0"
        kw = dict(stored=0)
    elif kind in ("flip_first", "flip_last", "flip_span"):
        pos = {"flip_first": v.P0, "flip_last": v.E - 1, "flip_span": K["span"] - 1}[kind]
        if not v.summed or not v.P0 <= pos < v.E or (kind == "flip_span" and pos in (v.P0, v.E - 1)):
            return None
        f[pos] ^= 0x10
        kw = dict(verdict=bad)
    else:
        assert kind == "flip_pad"   # outside [S, E): the verdict stays
        if not v.pad:
            return None
        f[v.E + v.pad // 2] ^= 0x10
    return replace(v, name=f"{v.name}_{kind}", frame=bytes(f), twin=kind, **kw)


def size_class(v: Vec, sh: int = 0) -> str:
    return CF.size_class(sh, len(v.frame))


def path(v: Vec, sh: int, aligned16: bool = False) -> int:
    """control_frames.path's rule for a TCP or UDP frame: the dk_diag.h path counter it adds to at offset sh mod 16."""
    ln = len(v.frame)
    if sh % 2 or (aligned16 and sh) or v.ihl != 5:
        return 3
    if sh + ln <= K["window"]:
        return 0
    last_granule_end = (sh + ln + 15) // 16 * 16 - sh
    return 2 if v.summed and last_granule_end - v.E > K["resum"] else 1


def path_counts(vecs, sh: int, aligned16: bool = False) -> list:
    out = [0, 0, 0, 0]
    for v in vecs:
        out[path(v, sh, aligned16)] += 1
    return out


def expected(vecs) -> dict:
    recs = [v.record() for v in vecs]
    return {k: np.array([r[k] for r in recs], np.uint32) for k in FIELDS}


def assert_records(res: dict, vecs, ctx: str = "", idx=None) -> None:
    """Every field of `res` present equals the construction's, for the frames idx (default: all, in order)."""
    exp = expected(vecs)
    idx = np.arange(len(vecs)) if idx is None else np.asarray(idx, np.int64)
    for k in FIELDS:
        if k not in res:
            assert k in ("dst_ip", "tcp_seq", "tcp_ack", "tcp_win"), k
            continue
        got = np.asarray(res[k])[idx]
        bad = np.nonzero(got != exp[k])[0]
        if bad.size:
            j = int(bad[0])
            names = sorted({vecs[int(b)].name for b in bad})[:6]
            raise AssertionError(f"{ctx}: '{k}' of {vecs[j].name} (built {vecs[j].verdict}): got {int(got[j]):#x} "
                                 f"want {int(exp[k][j]):#x}; {bad.size} frames differ, e.g. {names}")


def pack(frames, sh: int = 0, align: int = 64):
    """frames.pack with every frame `sh` bytes past an `align`-byte slot boundary and 0xFF in every gap, in front of the
    first frame and for 64 bytes behind the last."""
    offs, pos = [], 0
    for f in frames:
        pos = (pos + align - 1) // align * align + sh
        offs.append(pos)
        pos += len(f)
    blob = np.full(pos + 64, 0xFF, np.uint8)
    for o, f in zip(offs, frames):
        blob[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return blob, np.array(offs, np.uint32), np.array([len(f) for f in frames], np.uint16)


def scramble_fields(blob: np.ndarray, off, vecs, seed: int = 3) -> np.ndarray:
    """A copy of the blob with the IPv4 and L4 checksum fields of every frame overwritten with random bytes."""
    out = blob.copy()
    rng = np.random.default_rng(seed)
    for o, v in zip(off, vecs):
        for p in (24, 25, v.cfield, v.cfield + 1):
            out[int(o) + p] = rng.integers(0, 256)
    return out


def catalogue() -> list:
    return list(_catalogue())


def base_vectors() -> list:
    """The as-built frames (no twin): every one is accepted and carries its two targets."""
    return [v for v in _catalogue() if not v.twin]


@functools.lru_cache(maxsize=None)
def _catalogue() -> tuple:
    L = []
    count = [0]

    def add(proto, length, fill, target, twins=TWINS, **kw):
        k = count[0]
        count[0] += 1
        ipt = (None,) + IP_TARGETS
        kw.setdefault("ip_target", ipt[k % 4])
        extra = "".join(f"_{a}{kw[a]}" for a in ("ihl", "doff", "pad") if a in kw)
        v = vector(f"{'tcp' if proto == 6 else 'udp'}_{length}_{fill}_{target:04x}{extra}", proto, length, fill, target,
                   k=k, **kw)
        L.append(v)
        if fill in ("ff", "fffe"):
            for kind in twins:
                t = twin(v, kind)
                if t is not None:
                    L.append(t)

    cross = set(CROSS.values())
    for length in sorted(cross | set(LENGTHS)):
        for proto in (6, 17):
            if length in cross:
                for fill in FILLS:
                    for target in TARGETS:
                        add(proto, length, fill, target, tags=("cross",))
            else:
                for fill in ("fffe", "ff"):
                    for target in (0x0000, 0xFFFE):
                        add(proto, length, fill, target)
    for length in cross:
        for fill in ("fffe", "ff"):
            for target in (0x0000, 0xFFFE):
                for proto in (6, 17):
                    for pad in PADS:  # the frame keeps its length: the payload shrinks by the padding
                        if length - pad - (54 if proto == 6 else 42) >= 2:
                            add(proto, length, fill, target, twins=("flip_pad", "flip_last"), pad=pad, tags=("pad",))
                if length > 14 + 60 + 60 + 2:  # IPv4 options and TCP options to their limits (byte path / option walk)
                    for proto, ihl, doff in ((6, 15, 5), (6, 5, 15), (6, 15, 15), (17, 15, 5)):
                        kw = dict(ihl=ihl) if proto == 17 else dict(ihl=ihl, doff=doff)
                        add(proto, length, fill, target, twins=("flip_last",), tags=("opts",), **kw)
    # the largest sum[E, end) the re-sum rule ever meets: 65,535 bytes of which total_length covers 100 payload bytes
    for proto in (6, 17):
        add(proto, 65535, "fffe", 0xFFFE, twins=("flip_pad", "flip_last"), pad=65535 - (54 if proto == 6 else 42) - 100,
            tags=("pad_max",))
    guard(L)
    return tuple(L)


def guard(L) -> None:
    """The coverage the tests built on the catalogue rely on."""
    names = [v.name for v in L]
    assert len(set(names)) == len(names)
    base = [v for v in L if not v.twin]
    assert all(v.ok and v.stored == v.target for v in base)
    classes = CF.CLASSES
    seen = {(v.fill, v.proto, size_class(v)) for v in base}
    assert seen >= {(f, p, c) for f in FILLS for p in (6, 17) for c in classes}
    seen = {(v.target, v.proto, size_class(v)) for v in base}
    assert seen >= {(t, p, c) for t in TARGETS for p in (6, 17) for c in classes}
    seen = {(v.ip_target, v.proto, size_class(v)) for v in base}
    assert seen >= {(t, p, c) for t in IP_TARGETS for p in (6, 17) for c in classes}
    lens = {len(v.frame) for v in base}
    assert lens >= set(LENGTHS) and max(lens) == 65535
    for key in ("window", "med", "span"):  # every boundary at -1 / 0 / +1 for every offset the tests pack at
        for sh in SHIFTS:
            assert {K[key] + d - sh for d in (-1, 0, 1)} <= lens
    # a saturating fill never stands alone for a length: "ff" is blind to a dropped granule
    for n in lens:
        assert {"ff", "fffe"} <= {v.fill for v in base if len(v.frame) == n}, n
    reach = {"stored_ffff": classes, "udp_zero": classes, "flip_first": classes, "flip_last": classes,
             "flip_span": ("multi",), "flip_pad": classes}
    seen = {(v.twin, size_class(v)) for v in L if v.twin}
    assert seen >= {(t, c) for t in TWINS for c in reach[t]}
    assert all(v.verdict.endswith("CSUM") for v in L if v.twin in ("stored_ffff", "flip_first", "flip_last", "flip_span"))
    assert all(v.ok for v in L if v.twin in ("udp_zero", "flip_pad"))
    assert {(v.ihl, v.doff) for v in base if v.proto == 6} >= {(5, 5), (15, 5), (5, 15), (15, 15)}
    assert {p for v in base for p in [v.pad] if p} >= set(PADS)
    for sh in (0, 2):  # every path is reached at the even offsets; an odd one is the byte path throughout
        assert all(x > 0 for x in path_counts(L, sh)), sh
    assert path_counts(L, 1) == [0, 0, 0, len(L)]


def census(L) -> dict:
    """{(fill, size class): vectors}, with twins and totals under their own keys."""
    out = {}
    for v in L:
        for key in ((v.fill, size_class(v)), ("twin:" + v.twin if v.twin else "as built", "all"), ("total", "all")):
            out[key] = out.get(key, 0) + 1
    out["bytes", "all"] = sum(len(v.frame) for v in L)
    return out
