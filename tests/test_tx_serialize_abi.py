"""dk_tx_serialize on the CPU: the ABI additions (struct layouts, constants, dk_tx_header_bytes) and the pinning of
tests/tx_reference.py, the plain-Python restatement of the send chain the GPU tests compare against: its frames equal
tests/frames.py's independent builders byte for byte, the oracle's checksum pair of each frame is the pair it stored,
and the receive oracle delivers every frame with the fields and option records that went in. No GPU work."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np

import frames as F
import tx_reference as R
from demikernel_amd import _native as N
from demikernel_amd import ipv4, synth, tx_header_bytes
from oracle import oracle as O
from oracle.oracle import OraclePeer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_rx.h")
ALICE, BOB = ipv4(synth.ALICE_IPV4), ipv4(synth.BOB_IPV4)


def test_tx_struct_layout_matches_ctypes(tmp_path):
    """sizeof / offsetof from the C compiler == the ctypes mirror (dk_tx_link, dk_tx_segs) and the numpy link record."""
    structs = {"dk_tx_link": N.DkTxLink, "dk_tx_segs": N.DkTxSegs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert ctypes.sizeof(N.DkTxLink) == N.TX_LINK_DTYPE.itemsize == 16
    for fname, _ in N.DkTxLink._fields_:
        assert N.TX_LINK_DTYPE.fields[fname][1] == getattr(N.DkTxLink, fname).offset, fname
    assert [f for f, _ in N.DkTxSegs._fields_] == N.TX_SEG_FIELDS + ["n", "flags"]


def test_tx_constants_match_header():
    hdr = open(HEADER).read()
    for i, name in enumerate(N.TX_STATUSES):
        assert re.search(rf"DK_TX_{name} = {i}[,\s]", hdr), name
        assert getattr(N, f"DK_TX_{name}") == i == getattr(R, name)
    assert f"#define DK_TX_OFFLOAD_TCP {N.DK_TX_OFFLOAD_TCP}u" in hdr and N.DK_TX_OFFLOAD_TCP == R.OFFLOAD_TCP
    assert f"#define DK_TX_OFFLOAD_UDP {N.DK_TX_OFFLOAD_UDP}u" in hdr and N.DK_TX_OFFLOAD_UDP == R.OFFLOAD_UDP
    assert "#define DK_RX_ABI_VERSION 4u" in hdr  # additive entry points: the version does not move
    lib = N.load_library()
    assert lib.dk_tx_serialize and lib.dk_tx_header_bytes


def test_tx_header_bytes():
    assert tx_header_bytes(17) == 42
    assert tx_header_bytes(6) == 54
    assert tx_header_bytes(6, R.opts_record([])) == 54
    assert tx_header_bytes(6, R.opts_record([("mss", 1460), ("ws", 7)])) == 62  # 4 + 3 + 1 EOL = 8
    assert tx_header_bytes(1) == 0 and tx_header_bytes(0) == 0
    want = dict(mss=62, ws=58, sack_ok=58, ts=66, nop=58, eol=58, sack1=66, sack4=90, fill40=94)
    for name, entries, _ in R.option_cases():
        rec = R.opts_record(entries)
        got = tx_header_bytes(6, rec)
        assert got == R.header_bytes(6, rec[0]) and got % 4 == 2, name
        if name in want:
            assert got == want[name], name
        assert tx_header_bytes(17, rec) == 42  # the list does not matter for UDP
    for name, rec in R.bad_option_cases():
        assert tx_header_bytes(6, rec) == 0 == R.header_bytes(6, rec[0]), name


# ---------------------------------------------------------------------------------------------------------------------
# tests/tx_reference.py pinned against independent code
# ---------------------------------------------------------------------------------------------------------------------
def _segments():
    """(proto, payload, fields dict, option entries, hand-encoded option bytes) for the pinning tests."""
    rng = np.random.default_rng(20)
    pl = rng.integers(0, 256, 1500, dtype=np.uint8).tobytes()
    segs = []
    for k, ln in enumerate([0, 1, 2, 33, 100, 1460]):
        f = dict(sport=40000, dport=12345, seq=0x01020304 + k, ack=0xF0E0D0C0 - k, b13=0x18, window=4096 + k, urg=k)
        segs.append((6, pl[:ln], f, [], b""))
        segs.append((17, pl[k:k + ln], dict(sport=40000 + k, dport=5000), [], b""))
    for k, (name, entries, raw) in enumerate(R.option_cases()):
        f = dict(sport=40000, dport=12345, seq=k, ack=0, b13=0x02 if k % 2 else 0x12, window=65535, urg=0)
        segs.append((6, pl[:3 * k], f, entries, raw))
    return segs


def _zero_residue_segment():
    """A TCP segment whose words (pseudo-header included) sum to 0 mod 0xFFFF: its last payload word is the checksum
    the same segment has with that word zero."""
    f = dict(sport=40000, dport=12345, seq=7, ack=9, b13=0x18, window=1000, urg=0)
    pl = bytearray(np.random.default_rng(21).integers(0, 256, 64, dtype=np.uint8).tobytes())
    pl[62:64] = b"\0\0"
    h = _headers(6, bytes(pl), f, [])
    pl[62:64] = h[50:52]
    return 6, bytes(pl), f, [], b""


def _headers(proto, payload, f, entries, flags=0):
    rec = R.opts_record(entries)[0] if entries else None
    options = R.tcp_option_bytes(rec)
    meta = proto << 8 | f.get("b13", 0) << 16 | ((20 + len(options)) // 4) << 28
    return R.headers(payload, proto, ALICE, BOB, f["sport"] | f["dport"] << 16, meta=meta, seq=f.get("seq", 0),
                     ack=f.get("ack", 0), winurg=f.get("window", 0) | f.get("urg", 0) << 16, options=options,
                     dst_mac=synth.BOB_MAC, src_mac=synth.ALICE_MAC, flags=flags)


def _independent(proto, payload, f, raw, nonempty):
    """The same frame from tests/frames.py (RFC 1071 checksums, option bytes encoded by hand; a list that is not empty
    ends with the EndOfOptionsList byte, and frames.py pads with zeros to a multiple of 4)."""
    if proto == 17:
        return F.udp_frame(payload, sport=f["sport"], dport=f["dport"], ttl=255, ident=0, flags=0x2)
    options = raw + b"\0" if nonempty else b""
    return F.tcp_frame(payload, options=options, sport=f["sport"], dport=f["dport"], ttl=255, ident=0, flags=0x2,
                       tcp_kw=dict(seq=f["seq"], ack=f["ack"], flags=f["b13"], window=f["window"], urg=f["urg"]))


def test_reference_equals_independent_builders():
    checked = 0
    for proto, payload, f, entries, raw in _segments() + [_zero_residue_segment()]:
        h = _headers(proto, payload, f, entries)
        mine = h + payload
        theirs = _independent(proto, payload, f, raw, bool(entries))
        l4 = theirs[34:]
        rfc = struct.unpack("!H", l4[16:18] if proto == 6 else l4[6:8])[0]
        if rfc == 0xFFFF:  # RFC 1071's all-ones form of zero: the reference's fold never produces it
            continue
        assert mine == theirs, (proto, len(payload), entries)
        checked += 1
    assert checked == len(_segments()) + 1


def test_zero_residue_stores_zero_not_ffff():
    proto, payload, f, entries, _ = _zero_residue_segment()
    h = _headers(proto, payload, f, entries)
    seg = h[34:] + payload
    assert (R.pseudo_sum(ALICE, BOB, 6, len(seg)) + R.be_words(seg)) % 0xFFFF == 0
    assert h[50:52] == b"\0\0"
    assert O.tx_checksum_fields(h + payload) >> 16 == 0


def test_reference_checksums_are_the_oracles():
    for proto, payload, f, entries, _ in _segments() + [_zero_residue_segment()]:
        h = _headers(proto, payload, f, entries)
        cs = 34 + (16 if proto == 6 else 6)
        stored = struct.unpack("!H", h[24:26])[0] | struct.unpack("!H", h[cs:cs + 2])[0] << 16
        assert O.tx_checksum_fields(h + payload) == stored, (proto, len(payload), entries)
        # offload: the two checksum bytes are zero, every other byte is unchanged
        ho = _headers(proto, payload, f, entries, flags=R.OFFLOAD_TCP | R.OFFLOAD_UDP)
        assert ho[cs:cs + 2] == b"\0\0" and ho[:cs] == h[:cs] and ho[cs + 2:] == h[cs + 2:]


def test_oracle_peer_delivers_reference_frames():
    cases = _segments() + [_zero_residue_segment()]
    frames = [_headers(p, pl, f, e) + pl for p, pl, f, e, _ in cases]
    blob, off, lens = F.pack(frames)
    peer = OraclePeer(BOB)
    peer.set_flows(F.corpus_flows())
    r = peer.process(blob, off, lens)
    for i, (proto, payload, f, entries, _) in enumerate(cases):
        H = len(frames[i]) - len(payload)
        assert r["meta"][i] & 0xFF == (N.V["OK_TCP"] if proto == 6 else N.V["OK_UDP"]), i
        assert (r["meta"][i] >> 8) & 0xFF == proto
        assert r["src_ip"][i] == ALICE and r["dst_ip"][i] == BOB
        assert r["ports"][i] == f["sport"] | f["dport"] << 16
        assert r["payload"][i] == H | len(payload) << 16
        if proto != 6:
            continue
        assert r["meta"][i] >> 16 == f["b13"] | ((H - 34) // 4) << 12
        assert (r["tcp_seq"][i], r["tcp_ack"][i]) == (f["seq"], f["ack"])
        assert r["tcp_win"][i] == f["window"] | f["urg"] << 16
        if entries:
            kept = [e for e in entries if e[0] not in ("nop", "eol")]  # not entries on the receive side
            want = R.opts_record(kept)[0]
            assert r["tcp_opts"][i].tobytes() == want.tobytes(), (i, entries)


def test_serialize_batch_statuses_and_layout():
    """The batch form: headers land in front of the payload, failures write nothing, the first failing check wins."""
    blob = np.full(4096, 0xEE, np.uint8)
    links = np.zeros(1, N.TX_LINK_DTYPE)
    mk = lambda **kw: {k: np.array([v]) for k, v in kw.items()}  # noqa: E731
    base = dict(payload_off=100, payload_len=10, meta=17 << 8, src_ip=ALICE, dst_ip=BOB, ports=1 | 2 << 16)
    out, off, ln, st = R.serialize_batch(blob, mk(**base), links)
    assert (st[0], off[0], ln[0]) == (R.OK, 58, 52) and (out[:58] == 0xEE).all() and (out[100:] == 0xEE).all()
    for kw, want in ((dict(meta=1 << 8), R.E_PROTO), (dict(meta=6 << 8 | 6 << 28), R.E_OPTS),
                     (dict(link=1), R.E_LINK), (dict(payload_len=65535 - 41), R.E_LEN),
                     (dict(payload_off=41), R.E_RANGE), (dict(payload_off=4090), R.E_RANGE),
                     (dict(meta=1 << 8, link=1), R.E_PROTO), (dict(link=1, payload_off=41), R.E_LINK)):
        out, off, ln, st = R.serialize_batch(blob, mk(**dict(base, **kw)), links)
        assert (st[0], off[0], ln[0]) == (want, 0, 0) and (out == 0xEE).all(), kw
