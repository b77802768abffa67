"""The steered TCP / UDP checksum vectors (tests/checksum_vectors.py) against the CPU oracle: OraclePeer.process must
give the by-construction record on every field of every vector at offsets 0, 2 and 1 mod 16, every as-built frame must
carry its two targets, oracle.tx_fill_checksums must restore scrambled fields byte for byte, and the builder's guards
hold, so the GPU tests built on the catalogue cannot quietly lose a case."""
import numpy as np
import pytest

import checksum_vectors as CV
import frames as F
from demikernel_amd import synth
from demikernel_amd._native import DK_FLOW_NONE, V
from demikernel_amd.rx import ipv4
from oracle import oracle as O
from oracle.oracle import OraclePeer


def run_oracle(blob, off, lens):
    p = OraclePeer(ipv4(synth.BOB_IPV4))
    p.set_flows(F.corpus_flows())
    return p.process(blob, off, lens)


def test_codes_and_flows_match_the_abi():
    assert {k: V[k] for k in CV.CODES} == CV.CODES and CV.DK_FLOW_NONE == DK_FLOW_NONE
    flows = F.corpus_flows()
    assert int(flows["local_port"][CV.FLOW_TCP]) == CV.TCP_DPORT and int(flows["remote_port"][CV.FLOW_TCP]) == CV.SPORT
    assert int(flows["local_port"][CV.FLOW_UDP]) == CV.UDP_DPORT


def test_steer_meets_every_target_from_every_residue_class():
    rng = np.random.default_rng(5)
    rests = [0, 1, 0xFFFE, 0xFFFF, 0x10000, 0x1FFFE, 65535 * 32768] + rng.integers(0, 1 << 31, 200).tolist()
    for rest in rests:
        for target in CV.TARGETS:
            w = CV.steer(rest, target)
            assert 0 <= w < 0xFFFF and F.ref_checksum(rest + w) == target
            assert F.ref_checksum(rest + w) == F.rfc1071(b"", rest + w) or target == 0  # RFC 1071 differs at residue 0
    assert F.rfc1071(b"", 0xFFFF) == 0 and F.rfc1071(b"", 0) == 0xFFFF and F.ref_checksum(0) == 0


@pytest.mark.parametrize("sh", CV.SHIFTS)
def test_oracle_matches_the_construction(sh):
    vecs = CV.catalogue()
    blob, off, lens = CV.pack([v.frame for v in vecs], sh)
    assert (off % 16 == sh).all() and int(lens.max()) == 65535
    res = run_oracle(blob, off, lens)
    CV.assert_records(res, vecs, f"offset {sh}")
    want = np.bincount([CV.CODES[v.verdict] for v in vecs], minlength=len(res["verdict_counts"]))
    assert np.array_equal(res["verdict_counts"], want.astype(np.uint64))


def test_as_built_frames_store_their_targets():
    for v in CV.base_vectors():
        f = v.frame
        assert int.from_bytes(f[24:26], "big") == v.ip_target, v.name
        assert int.from_bytes(f[v.cfield:v.cfield + 2], "big") == v.target == v.stored, v.name
        # the same two values by an independent sum over the finished frame
        assert F.ref_checksum(CV.be_sum(f[14:24] + f[26:34])) == v.ip_target, v.name
        seg = f[14 + 4 * v.ihl:v.cfield] + b"\0\0" + f[v.cfield + 2:v.E]
        assert F.ref_checksum(F.pseudo(F.ALICE_IPV4, F.BOB_IPV4, v.proto, len(seg)) + CV.be_sum(seg)) == v.target, v.name
        if v.pad:
            assert set(f[v.E:]) == {0xFF}, v.name
    steered = [v for v in CV.base_vectors() if v.ip_target in CV.IP_TARGETS]
    assert len(steered) > len(CV.base_vectors()) // 2


def test_oracle_tx_fill_restores_scrambled_fields():
    vecs = CV.base_vectors()
    blob, off, lens = CV.pack([v.frame for v in vecs], 2)
    scr = CV.scramble_fields(blob, off, vecs)
    assert (scr != blob).sum() > len(vecs)
    for v, o, ln in zip(vecs, off, lens):
        fr = bytearray(scr[int(o):int(o) + int(ln)].tobytes())
        O.tx_fill_checksums(fr)
        assert bytes(fr) == v.frame, v.name
        assert O.tx_checksum_fields(bytes(scr[int(o):int(o) + int(ln)])) == v.ip_target | v.target << 16, v.name


def test_guards_and_census(capsys):
    L = CV.catalogue()
    CV.guard(L)
    cen = CV.census(L)
    with capsys.disabled():
        print("\nchecksum vectors: fill x size class")
        for fill in CV.FILLS:
            print(f"  {fill:10s} " + " ".join(f"{c}={cen.get((fill, c), 0)}" for c in ("window", "medium", "large", "multi")))
        print("  " + ", ".join(f"{k[0]}={n}" for k, n in sorted(cen.items()) if k[1] == "all"))
    assert cen["total", "all"] == len(L) and cen["as built", "all"] == len(CV.base_vectors())


def test_steering_bites():
    """With the steering word left as the fill, a vector meets its target only by accident: the targets are reached by
    the steering and not by the fills themselves."""
    met = total = 0
    for v in CV.base_vectors():
        if "cross" not in v.tags:
            continue
        f = bytearray(v.frame)
        f[v.spos:v.spos + 2] = v.fill_word
        seg = bytes(f[14 + 4 * v.ihl:v.cfield]) + b"\0\0" + bytes(f[v.cfield + 2:v.E])
        natural = F.ref_checksum(F.pseudo(F.ALICE_IPV4, F.BOB_IPV4, v.proto, len(seg)) + CV.be_sum(seg))
        total += 1
        met += natural == v.target
    assert total >= 5 * len(CV.FILLS) * len(CV.TARGETS) * 2
    # a natural checksum is one value in 65,535: a handful of coincidences at the most among a few hundred vectors
    assert met <= 2, (met, total)
