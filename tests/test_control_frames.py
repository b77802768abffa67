"""The control-plane frame builder (tests/control_frames.py) against the CPU oracle: OraclePeer.process must give the
by-construction record on every field of every ICMPv4 / ARP frame of the ladder, the ARP set and a 4,000-frame mix;
plus a guard on the builder itself (every control verdict in every size class it can occur in, every ladder boundary
at offsets 0 and 2 mod 16), so the GPU tests built on it cannot quietly lose a case."""
import numpy as np
import pytest

import control_frames as CF
import frames as F
from demikernel_amd import synth
from demikernel_amd._native import DK_FLOW_NONE, V, VERDICTS
from demikernel_amd.rx import ipv4
from oracle.oracle import OraclePeer


def oracle(blob, off, lens, flows=None):
    p = OraclePeer(ipv4(synth.BOB_IPV4))
    if flows is not None:
        p.set_flows(flows)
    return p.process(blob, off, lens)


def test_codes_match_the_abi():
    assert {k: V[k] for k in CF.CODES} == CF.CODES and CF.DK_FLOW_NONE == DK_FLOW_NONE
    assert CF.K["window"] == 64  # RegAcc::w; the other three are free to move with the kernels' tuning
    assert CF.K["window"] < CF.K["med"] < CF.K["span"]


@pytest.mark.parametrize("misalign", [None, [2], [1], list(range(16))])
def test_ladder_and_arp_set_match_oracle(misalign):
    ctls = CF.icmp_ladder() + CF.arp_set()
    blob, off, lens = F.pack([c.frame for c in ctls], misalign=misalign)
    res = oracle(blob, off, lens)
    CF.assert_control(res, np.arange(len(ctls)), ctls, f"misalign={misalign}")
    for k in ("tcp_seq", "tcp_ack", "tcp_win"):
        assert not res[k].any(), k
    assert not res["flow_counts"].any()
    want = np.bincount([CF.CODES[c.verdict] for c in ctls], minlength=len(VERDICTS))
    assert np.array_equal(res["verdict_counts"], want.astype(np.uint64))


def test_mix_matches_oracle():
    n = 4000
    flows = np.concatenate([synth.make_flows(300), synth.make_flows(20, kind="udp")])
    blob, off, lens, idx, ctls = CF.control_mix(n, synth.imix_ip_lengths(n, seed=4), flows, seed=6)
    assert len(off) == n and len(idx) == len(ctls) == 1000  # every control frame is checked: none left out
    res = oracle(blob, off, lens, flows)
    CF.assert_control(res, idx, ctls, "imix mix")
    car = np.ones(n, bool)
    car[idx] = False
    v = res["meta"] & 0xFF
    assert not np.isin(v[car], list(CF.CODES.values())).any()  # the carrier holds no control frame of its own
    assert (v[car] <= 1).mean() > 0.9
    deliv = v <= 1
    assert np.array_equal(res["flow_counts"], np.bincount(res["flow_id"][deliv], minlength=len(flows)).astype(np.uint64))
    assert 128 <= blob.size // n < CF.K["med"]  # the staged kernel's band under launch_batch's rule


def remap_refs(views, cpos, count=None):
    """Frame indices of the unspliced batch -> their positions in the spliced one (the EOF buffer has none)."""
    from demikernel_amd._native import DK_TCP_REF_EOF

    v = views.copy()
    sel = v["ref"] != DK_TCP_REF_EOF
    if count is not None:
        sel &= np.arange(v.shape[-1])[None, :] < count[:, None]
    v["ref"][sel] = cpos[v["ref"][sel]].astype(np.uint32)
    return v


def build_tcp_mix():
    """synth.tcp_streams(3000, 7) with 1,000 ICMP and ARP frames spliced between the segments, the oracle chain
    (OraclePeer -> oracle.tcp_process) over it, and the oracle chain over the same streams without the splice."""
    from types import SimpleNamespace

    from oracle import oracle as O

    flows, tr, table = synth.tcp_streams(3000, 7, buffer_size=1 << 22, seed=77)
    blob0, off0, lens0 = synth.build_numpy(tr)
    synth.corrupt_numpy(blob0, off0, synth.corruption_plan(len(off0), 0.002, tr))
    carrier = [blob0[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(off0, lens0)]
    pool = [c for c in CF.icmp_ladder() + CF.arp_set() if len(c.frame) <= 1514]
    frames, idx, ctls, cpos = CF.splice(carrier, pool, 1000, seed=78)
    # ICMP types 1, 2 and 4: bits 16..23 of an ICMP meta word are where a TCP record keeps FIN, SYN and RST
    assert {1, 2, 4} <= {c.frame[34] for c in ctls if c.kind == "icmp" and c.ihl == 5 and c.summed}
    blob, off, lens = F.pack(frames)
    m = SimpleNamespace(blob=blob, off=off, lens=lens, idx=idx, ctls=ctls, flows=flows, n=len(off),
                        exp=oracle(blob, off, lens, flows))
    exp_t = table.copy()
    exp = O.tcp_process(exp_t, m.exp)
    plain_t = table.copy()
    plain = O.tcp_process(plain_t, oracle(blob0, off0, lens0, flows))
    return SimpleNamespace(m=m, table=table, exp_t=exp_t, exp=exp, plain_t=plain_t, plain=plain, cpos=cpos)


def test_splice_leaves_the_oracle_streams_alone():
    """The reference side of the GPU test through the TCP stage: in the oracle chain the spliced control frames match
    the construction and are DK_TCP_SKIP, and the connection table and deliveries are those of the streams alone
    (frame references moved to the frames' new positions)."""
    from demikernel_amd._native import A

    x = build_tcp_mix()
    CF.assert_control(x.m.exp, x.m.idx, x.m.ctls, "tcp streams with control frames")
    assert A["SKIP"] == 0 and not x.exp["action"][x.m.idx].any()
    assert np.array_equal(x.exp["action"][x.cpos], x.plain["action"])
    assert np.array_equal(x.exp["deliv_start"], x.plain["deliv_start"])
    assert np.array_equal(x.exp["deliv_count"], x.plain["deliv_count"])
    assert int(x.exp["deliv_count"].sum()) > 1000  # not vacuous: a third of the 3,000 segments reach a receive queue
    for c in range(len(x.table)):
        s, k = int(x.exp["deliv_start"][c]), int(x.exp["deliv_count"][c])
        assert np.array_equal(x.exp["deliv"][s:s + k], remap_refs(x.plain["deliv"][s:s + k], x.cpos)), c
    want_t = x.plain_t.copy()
    want_t["ooo"] = remap_refs(x.plain_t["ooo"], x.cpos, x.plain_t["ooo_count"])
    assert np.array_equal(x.exp_t.view(np.uint8), want_t.view(np.uint8))


def test_builder_guard():
    """Every control verdict in every size class where it can occur, at offsets 0 and 2 mod 16; every boundary at
    -1 / 0 / +1 for both offsets; E == 64; the accepted and rejected types; the paths the ladder must reach."""
    ladder, arps = CF.icmp_ladder(), CF.arp_set()
    ctls = ladder + arps
    for sh in (0, 2):
        cen = CF.census(ctls, (sh,))
        for v in CF.CONTROL_VERDICTS:
            for cls in CF.CLASSES:
                assert (cen.get((v, cls), 0) > 0) == CF.can_occur(v, cls), (v, cls, sh)
    tags = {t for c in ladder for t in c.tags}
    for key in ("window", "med", "span"):
        for sh in (0, 2):
            for d in (-1, 0, 1):
                assert ("bound", key, sh, d) in tags
                hit = [c for c in ladder if ("bound", key, sh, d) in c.tags]
                assert all(sh + len(c.frame) == CF.K[key] + d and c.verdict == "ICMP" and c.ihl == 5 for c in hit)
    assert any(c.E == 64 == len(c.frame) and c.verdict == "ICMP" for c in ladder)
    assert any(c.E <= 64 < len(c.frame) and c.verdict == "ICMP" for c in ladder)
    assert any(2 * CF.K["span"] == len(c.frame) for c in ladder) and any(len(c.frame) == 9000 for c in ladder)
    for cls in CF.CLASSES:
        here = [c for c in ladder if CF.size_class(0, len(c.frame)) == cls]
        types = {(c.hi >> 8) & 0xFF for c in here if c.verdict == "ICMP"}
        assert set(CF.ICMP_ACCEPTED) <= types, cls
        assert sum(c.verdict == "ICMP_TYPE" for c in here) >= len(CF.ICMP_REJECTED), cls
        # an IHL-15 header ends at byte 74: past the 64-byte window
        assert {c.ihl for c in here} >= ({5, 6} if cls == "window" else {5, 6, 15}), cls
        assert any(c.summed and (c.E - 34) % 2 for c in here), cls  # an odd message length
    assert {len(c.frame) for c in arps} >= {14, 41, 42, 60, 1500}
    for sh in (0, 2):
        st = CF.path_counts(ctls, sh)
        assert all(x > 0 for x in st) and sum(st) == len(ctls), st
    assert CF.path_counts(ctls, 1) == [0, 0, 0, len(ctls)] == CF.path_counts(ctls, 2, aligned16=True)
    # the mixes the GPU tests run keep that coverage: every verdict, every class up to the carrier's size
    flows = synth.make_flows(8)
    _, _, _, _, mix = CF.control_mix(6000, synth.imix_ip_lengths(6000, seed=4), flows, seed=6)
    cen = CF.census(mix)
    for v in CF.CONTROL_VERDICTS:
        for cls in ("window", "medium", "large"):
            assert (cen.get((v, cls), 0) > 0) == CF.can_occur(v, cls), (v, cls)
