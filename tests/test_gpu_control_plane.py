"""ICMPv4 and ARP frames through every receive kernel family (unstaged, staged, split, small-frame), where so far
only the unstaged kernel had ever seen one. Every case has two checks: all result arrays and both counter arrays
bit-exact against the CPU oracle (as test_gpu_parity.check), and every field of every control frame equal to the
record tests/control_frames.py wrote down by construction. Mixes and their oracle results are built once per module."""
from types import SimpleNamespace

import numpy as np
import pytest

import control_frames as CF
import frames as F
import test_control_frames as TC
import test_gpu_parity as P
from demikernel_amd import Config, FrameBatch, RxEngine, RxResults, synth
from demikernel_amd import _native as N

pytestmark = pytest.mark.gpu

LOCAL = synth.BOB_IPV4
FAMILIES = ["unstaged", "staged", "split", "small"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def flows_tcp_udp():
    return np.concatenate([synth.make_flows(300), synth.make_flows(20, kind="udp")])


def frozen(**kw):
    """A batch with its oracle result, shared by the cases of this module and never written."""
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return SimpleNamespace(**kw)


def make_batch(frames, idx, ctls, flows, misalign=None):
    blob, off, lens = F.pack(frames, misalign=misalign)
    return frozen(blob=blob, off=off, lens=lens, idx=np.asarray(idx, np.int64), ctls=ctls, flows=flows,
                  exp=P.run_oracle(blob, off, lens, flows), n=len(off))


def device_batch(m):
    """The shared (read-only) host arrays of m, copied to the device."""
    return FrameBatch.from_numpy(m.blob.copy(), m.off.copy(), m.lens.copy(), device=0)


def run(m, tuning=None, aligned16=None, tcp_fields=True, dst_ip=True, stats=False):
    """One launch of batch m on a fresh engine: (results as numpy, path counters or None)."""
    import torch

    eng = RxEngine(Config(LOCAL), device=0, tuning=tuning)
    eng.set_sockets(m.flows)
    if stats:
        eng.path_stats(True)
    b = device_batch(m)
    if aligned16 is not None:
        b.aligned16 = aligned16
    r = eng.results(m.n, tcp_fields=tcp_fields, dst_ip=dst_ip)
    eng.receive_batch(b, r)
    torch.cuda.synchronize()
    out = r.to_numpy()
    st = eng.path_stats().tolist() if stats else None
    eng.close()
    return out, st


def both_checks(got, m, ctx):
    P.assert_same(got, m.exp, ctx)
    CF.assert_control(got, m.idx, m.ctls, ctx)


@pytest.fixture(scope="module")
def imix():
    """6,000 frames, IMIX carrier with 25 % control frames, descriptors permuted."""
    n = 6000
    flows = flows_tcp_udp()
    blob, off, lens, idx, ctls = CF.control_mix(n, synth.imix_ip_lengths(n, seed=4), flows, seed=6)
    perm = np.random.default_rng(8).permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    off, lens, idx = off[perm].copy(), lens[perm].copy(), inv[idx]
    assert 128 <= blob.size // n < CF.K["med"]
    return frozen(blob=blob, off=off, lens=lens, idx=idx, ctls=ctls, flows=flows, n=n,
                  exp=P.run_oracle(blob, off, lens, flows))


# ---------------------------------------------------------------------------------------------------------------------
# Case 1: every family, schedule and record
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("record", ["libos", "headline"])
@pytest.mark.parametrize("grid", [None, "7"])
@pytest.mark.parametrize("sched", ["0", "1"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_mix_every_variant(torch_cuda, imix, fam, sched, grid, record):
    """The test_kernel_variants matrix on the mix: each family under both wave schedules, the default grid and one of 7
    workgroups, with and without the TCP fields (an ICMP or ARP record in a staged 9-word slot must carry zeros
    there). sched 1 writes no dst_ip."""
    tune = {**P.family(fam), "sched": int(sched), "grid": int(grid) if grid else -1}
    got, _ = run(imix, tune, tcp_fields=record == "libos", dst_ip=sched != "1")
    assert ("dst_ip" in got) == (sched != "1") and ("tcp_seq" in got) == (record == "libos")
    both_checks(got, imix, f"{fam} sched={sched} grid={grid} {record}")
    if record == "libos":
        for k in ("tcp_seq", "tcp_ack", "tcp_win"):
            assert not got[k][imix.idx].any(), k


# ---------------------------------------------------------------------------------------------------------------------
# Case 2: the ladder at every shift, with the path counters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladders():
    ctls = CF.icmp_ladder() + CF.arp_set()
    fr = [c.frame for c in ctls]
    return [make_batch(fr, np.arange(len(ctls)), ctls, F.corpus_flows(), misalign=[s]) for s in range(16)]


@pytest.mark.parametrize("shift", list(range(16)))
@pytest.mark.parametrize("fam", FAMILIES)
def test_ladder_every_shift(torch_cuda, ladders, fam, shift):
    """The whole ladder and ARP set at one offset mod 16 under one forced family, with the realigning instantiation
    (aligned16 None: the hint follows the offsets) and without (aligned16 True: a frame off the 16-byte grid takes
    the byte path). The four path counters must equal the counts the construction gives, so no frame can pass by
    quietly taking another path."""
    m = ladders[shift]
    for hint in (None, True):
        ctx = f"{fam} shift={shift} aligned16={hint}"
        got, st = run(m, P.family(fam), aligned16=hint, stats=True)
        both_checks(got, m, ctx)
        assert st == CF.path_counts(m.ctls, shift, aligned16=bool(hint)), ctx


# ---------------------------------------------------------------------------------------------------------------------
# Case 3: the engine's own rule
# ---------------------------------------------------------------------------------------------------------------------
def launch_lines(err):
    out = []
    for line in err.splitlines():
        if line.startswith("dk_rx: "):
            kv = dict(w.split("=") for w in line.split()[1:])
            out.append({k: int(kv[k]) for k in ("stage", "split", "small", "n")})
    return out


@pytest.fixture(scope="module")
def rule_mixes(imix):
    """One mix per band of launch_batch's rule: 64-byte carrier frames (control frames up to 64 bytes), the IMIX mix,
    and 9,000-byte carrier frames (the whole ladder)."""
    out = {"staged": imix}
    for band, n, ip_len in (("small", 3000, 50), ("split", 1200, 8986)):
        flows = flows_tcp_udp()
        blob, off, lens, idx, ctls = CF.control_mix(n, ip_len, flows, seed=21)
        out[band] = frozen(blob=blob, off=off, lens=lens, idx=idx, ctls=ctls, flows=flows, n=n,
                           exp=P.run_oracle(blob, off, lens, flows))
    return out


@pytest.mark.parametrize("band", ["small", "staged", "split"])
def test_rule_picks_the_family(torch_cuda, capfd, rule_mixes, band):
    """No forced tuning: the mean blob bytes per frame (<= 96, [128, 1280), >= 1280) must put the mix on the
    small-frame, staged and split kernel, as the debug line shows."""
    m = rule_mixes[band]
    per = m.blob.size // m.n
    assert {"small": per <= 96, "staged": 128 <= per < 1280, "split": per >= 1280}[band], per
    capfd.readouterr()
    got, _ = run(m, {"debug": 1})
    lines = launch_lines(capfd.readouterr().err)
    want = {"small": dict(stage=0, split=0, small=1), "staged": dict(stage=1, split=0, small=0),
            "split": dict(stage=1, split=1, small=0)}[band]
    assert lines == [{**want, "n": m.n}], lines
    both_checks(got, m, f"rule, {band} band")
    assert {c.verdict for c in m.ctls} == set(CF.CONTROL_VERDICTS)


# ---------------------------------------------------------------------------------------------------------------------
# Case 4: whole-wave shapes
# ---------------------------------------------------------------------------------------------------------------------
WAVE_SIZES = (1, 63, 64, 65, 256)
WAVE_KINDS = ("icmp_e64", "arp", "icmp_streamed", "alternating")


def wave_frames(kind, n):
    if kind == "icmp_e64":  # E == 64 in every lane: the wave-uniform sum form (a flipped bit keeps E)
        return [CF.icmp(f"e64_{k}", p=CF.K["window"] - 42, type_=CF.ICMP_ACCEPTED[k % 11], code=k & 3, ident=k,
                        seq=0xFFFF - k, corrupt="last" if k % 7 == 3 else None) for k in range(n)]
    ladder, arps = CF.icmp_ladder(), CF.arp_set()
    if kind == "arp":  # every lane of every chunk deferred to the small-frame kernel's second pass
        return [arps[k % len(arps)] for k in range(n)]
    big = [c for c in ladder if CF.K["window"] < len(c.frame) <= 2 * CF.K["span"] and c.ihl == 5]
    if kind == "icmp_streamed":
        return [big[(5 * k) % len(big)] for k in range(n)]
    return [arps[(k // 2) % len(arps)] if k % 2 else ladder[(7 * k) % len(ladder)] for k in range(n)]


@pytest.fixture(scope="module")
def waves():
    out = {}
    for kind in WAVE_KINDS:
        for n in WAVE_SIZES:
            ctls = wave_frames(kind, n)
            out[kind, n] = make_batch([c.frame for c in ctls], np.arange(n), ctls, F.corpus_flows())
    return out


@pytest.mark.parametrize("kind", WAVE_KINDS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_whole_wave_shapes(torch_cuda, waves, fam, kind):
    """Batches of 1, 63, 64, 65 and 256 frames that are only E == 64 ICMP, only ARP, only streamed ICMP, or ICMP and
    ARP alternating: whole waves (and a lone lane, a wave short of one lane, a wave and one lane) of one shape."""
    for n in WAVE_SIZES:
        m = waves[kind, n]
        got, st = run(m, P.family(fam), stats=True)
        both_checks(got, m, f"{fam} {kind} n={n}")
        assert st == CF.path_counts(m.ctls, 0), (fam, kind, n, st)
        if kind == "icmp_e64":
            assert st[0] == n and all(c.E == 64 == len(c.frame) for c in m.ctls)


# ---------------------------------------------------------------------------------------------------------------------
# Case 5: counters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_counters_across_launches(torch_cuda, imix, fam):
    """Three launches back to back on one engine and stream, the middle one with deferred counters (completed inside
    the third launch's kernel), then a deferred one completed by a flush: each launch's verdict_counts and
    flow_counts equal the oracle's, and the control frames add nothing to flow_counts."""
    import torch

    m = imix
    eng = RxEngine(Config(LOCAL), device=0, tuning=P.family(fam))
    eng.set_sockets(m.flows)
    b = device_batch(m)
    rs = [eng.results(m.n, tcp_fields=True) for _ in range(4)]
    for k, r in enumerate(rs[:3]):
        eng.receive_batch(b, r, defer_counts=k == 1)
    eng.receive_batch(b, rs[3], defer_counts=True)
    eng.flush_counts()
    torch.cuda.synchronize()
    car = np.ones(m.n, bool)
    car[m.idx] = False
    for k, r in enumerate(rs):
        got = r.to_numpy()
        both_checks(got, m, f"{fam} launch {k}")
        v = got["meta"] & 0xFF
        assert np.array_equal(got["verdict_counts"], np.bincount(v, minlength=N.DK_V_COUNT).astype(np.uint64))
        deliv = car & (v <= 1)
        assert np.array_equal(got["flow_counts"],
                              np.bincount(got["flow_id"][deliv], minlength=len(m.flows)).astype(np.uint64)), k
        assert int(got["flow_counts"].sum()) == int(deliv.sum()) > 0
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# Case 6: host pipeline
# ---------------------------------------------------------------------------------------------------------------------
CHUNK = 37


@pytest.fixture(scope="module")
def host_batch(imix):
    """Descriptor order for chunk_frames = 37: three chunks of 60-byte ARP, two of 1,500-byte ICMP, twenty mixed
    (the IMIX mix plus option-bearing TCP segments), one more of ARP, one of ICMP and a short mixed tail."""
    arps = [c for c in CF.arp_set() if len(c.frame) == 60]
    big = [CF.icmp(f"icmp1500_{k}", p=1500 - 42, type_=CF.ICMP_ACCEPTED[k % 11], ident=k, seq=k * 257 & 0xFFFF,
                   corrupt=("last", "first", "field")[k % 3] if k % 5 == 4 else None) for k in range(3 * CHUNK)]
    opts = [o for o, _ in F.tcp_opt_cases()]
    frames, idx, ctls = [], [], []

    def put(c):
        idx.append(len(frames))
        ctls.append(c)
        frames.append(c.frame)

    for k in range(3 * CHUNK):
        put(arps[k % len(arps)])
    for k in range(2 * CHUNK):
        put(big[k])
    is_ctl = np.zeros(imix.n, bool)
    is_ctl[imix.idx] = True
    by_pos = dict(zip(imix.idx.tolist(), imix.ctls))
    for k in range(20 * CHUNK):
        if k % 19 == 7:
            frames.append(F.tcp_frame(bytes(range(k % 90)), options=opts[k // 19 % len(opts)], sport=40000 + k,
                                      dport=synth.LOCAL_PORT))
        elif is_ctl[k]:
            put(by_pos[k])
        else:
            o, ln = int(imix.off[k]), int(imix.lens[k])
            frames.append(imix.blob[o:o + ln].tobytes())
    for k in range(CHUNK):
        put(arps[(k + 1) % len(arps)])
    for k in range(CHUNK):
        put(big[2 * CHUNK + k])
    for k in range(11):
        if k % 2:
            put(CF.icmp_ladder()[k])
        else:
            frames.append(F.udp_frame(b"tail", dport=5000 + k))
    return make_batch(frames, idx, ctls, imix.flows)


def test_host_pipeline_changes_family_per_chunk(torch_cuda, capfd, host_batch):
    """receive_batch_host from pageable memory in chunks of 37 frames whose kind changes along the call: the
    per-chunk rule runs the small-frame, split and staged kernels inside one call. tcp_opts is requested too: the
    oracle's records for the option-bearing segments, zeros for every control frame."""
    m = host_batch
    eng = RxEngine(Config(LOCAL), tuning={"debug": 1})
    eng.set_sockets(m.flows)
    r = RxResults(m.n, len(m.flows), tcp_fields=True, host=True, tcp_opts=True)
    capfd.readouterr()
    eng.receive_batch_host(np.array(m.blob), np.array(m.off), np.array(m.lens), r, chunk_frames=CHUNK)
    lines = launch_lines(capfd.readouterr().err)
    eng.close()
    fams = ["small" if ln["small"] else "split" if ln["split"] else "staged" if ln["stage"] else "unstaged"
            for ln in lines]
    want = []  # launch_batch's rule on each chunk's covering byte range (64-byte slots: it starts at the first frame)
    for a in range(0, m.n, CHUNK):
        e = min(a + CHUNK, m.n)
        per = (int(m.off[e - 1]) + int(m.lens[e - 1]) - int(m.off[a])) // (e - a)
        want.append("small" if per <= 96 else "split" if per >= 1280 else "staged" if per >= 128 else "unstaged")
    assert want[:5] == ["small"] * 3 + ["split"] * 2 and want[25:27] == ["small", "split"], want
    assert set(want[5:25]) == {"staged"}, want
    assert fams == want and [ln["n"] for ln in lines] == [min(CHUNK, m.n - a) for a in range(0, m.n, CHUNK)], lines
    got = r.to_numpy()
    opts = got.pop("tcp_opts")
    both_checks(got, m, "host pipeline")
    assert opts.tobytes() == m.exp["tcp_opts"].tobytes()
    assert (m.exp["tcp_opts"]["num"] > 0).sum() >= 10  # tcp_opt_cases' well-formed lists, each at least once
    assert not opts[m.idx].view(np.uint8).any()


# ---------------------------------------------------------------------------------------------------------------------
# Case 7: through the TCP stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tcp_mix():
    return TC.build_tcp_mix()


@pytest.mark.parametrize("walk", ["lane", "wave", "relay", "scan"])
def test_tcp_stage_skips_control_frames(torch_cuda, tcp_mix, walk):
    """dk_rx_process -> dk_tcp_rx_process on the spliced batch under each walk, bit-exact against OraclePeer ->
    oracle.tcp_process: every control frame DK_TCP_SKIP, table and deliveries those of the streams alone."""
    import test_gpu_tcp as T
    import torch
    from demikernel_amd.tcp import TcpOut, TcpReceiver

    x, m = tcp_mix, tcp_mix.m
    tcp = TcpReceiver(0, walk=walk)
    eng = RxEngine(Config(LOCAL), device=0)
    eng.set_sockets(m.flows)
    r = eng.results(m.n, tcp_fields=True)
    b = device_batch(m)
    eng.receive_batch(b, r)
    conns = tcp.conns_to_device(x.table)
    out = TcpOut(m.n, len(x.table))
    tcp.process(r, conns, out)
    torch.cuda.synchronize()
    got_rx, got, got_t = r.to_numpy(), out.to_numpy(), tcp.conns_to_host(conns)
    tcp.close()
    eng.close()
    both_checks(got_rx, m, f"rx before tcp ({walk})")
    T.assert_same(got_t, got, x.exp_t, x.exp, f"{walk} walk")
    assert not got["action"][m.idx].any()
    assert np.array_equal(got["action"][x.cpos], x.plain["action"])
