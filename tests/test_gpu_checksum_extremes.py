"""Checksums at extreme values and lengths in every summing kernel: the steered TCP / UDP vectors of
tests/checksum_vectors.py (targets at the seams of the residue -> checksum map, saturating fills, frames up to the
65,535 bytes a descriptor can hold) through the four receive families, dk_tx_checksum / dk_tx_checksum_fields,
dk_tx_serialize and dk_tcp_tx_segment. Everything is bit-exact: the receive results against the construction and the
CPU oracle, the TX outputs against the as-built frames and the plain-Python models, the stored checksums against their
targets, and whatever a TX kernel writes goes back through the forced receive families."""
from types import SimpleNamespace

import numpy as np
import pytest

import checksum_vectors as CV
import frames as F
import test_gpu_control_plane as G
import test_gpu_parity as P
import test_gpu_tcp_tx_segment as T
import tx_reference as R
import tx_segment_reference as M
from demikernel_amd import Config, FrameBatch, RxEngine, TxSegments, ipv4, synth, tx_serialize, tx_tuning
from demikernel_amd import _native as N
from demikernel_amd.tx import ip_word
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LOCAL = synth.BOB_IPV4
FAMILIES = G.FAMILIES
OK = {6: N.V["OK_TCP"], 17: N.V["OK_UDP"]}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available()
    return torch


def batch_of(vecs, sh):
    """The vectors packed at offset sh mod 16 over a 0xFF background, with the oracle's results; never written."""
    blob, off, lens = CV.pack([v.frame for v in vecs], sh)
    flows = F.corpus_flows()
    return G.frozen(blob=blob, off=off, lens=lens, vecs=vecs, flows=flows, n=len(off),
                    exp=P.run_oracle(blob, off, lens, flows))


def receive_checks(m, fam, sh, ctx):
    """Batch m under one forced family, with and without the realigning instantiation, both records: results against
    the construction and the oracle, path counters against the rule. Returns the counters of one run."""
    want = CV.path_counts(m.vecs, sh)
    for hint in (None, False):
        for record in ("libos", "headline"):
            c = f"{ctx} {fam} offset={sh} aligned16={hint} {record}"
            # the counters ride on the kernels' optional-output instantiation: the headline record runs without them
            got, st = G.run(m, P.family(fam), aligned16=hint, tcp_fields=record == "libos", stats=record == "libos")
            assert ("tcp_seq" in got) == (record == "libos")
            CV.assert_records(got, m.vecs, c)
            P.assert_same(got, m.exp, c)
            if st is not None:
                assert st == want, (c, st, want)
    return want


# ---------------------------------------------------------------------------------------------------------------------
# 1. receive: the catalogue and two whole-wave shapes in every family
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packs():
    return {sh: batch_of(CV.catalogue(), sh) for sh in CV.SHIFTS}


@pytest.mark.parametrize("sh", CV.SHIFTS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_receive_catalogue(torch_cuda, packs, fam, sh):
    m = packs[sh]
    st = receive_checks(m, fam, sh, "catalogue")
    assert sum(st) == m.n and (all(st) if sh % 2 == 0 else st[:3] == [0, 0, 0])
    print(f"\n{fam} offset {sh}: {m.n} frames, {m.blob.size} bytes, path counters {st}")


def small_frames(n):
    """n steered 64-byte frames (the register window exactly), TCP and UDP alternating."""
    return [CV.vector(f"w64_{k}", (6, 17)[k % 2], 64, CV.FILLS[k % 3], CV.TARGETS[k % 7], k=5000 + k) for k in range(n)]


@pytest.fixture(scope="module")
def wave_shapes():
    big = [v for v in CV.catalogue() if len(v.frame) == 65535]
    assert len(big) >= 64 and {v.twin for v in big} >= {"", "stored_ffff", "flip_span", "flip_last", "flip_pad"}
    small = small_frames(63)
    out = {}
    for sh in (0, 2):
        # one 65,535-byte frame among 63 of 64 bytes: owned by a lane of each quarter-wave in turn
        for q, pos in enumerate((3, 19, 40, 63)):
            one = big[(11 * q + 5) % len(big)]
            out["lone", q, sh] = batch_of(small[:pos] + [one] + small[pos:], sh)
        out["full", 0, sh] = batch_of(big[::len(big) // 64][:64], sh)
    return out


@pytest.mark.parametrize("fam", FAMILIES)
def test_receive_whole_wave_shapes(torch_cuda, wave_shapes, fam):
    for (kind, q, sh), m in wave_shapes.items():
        assert m.n == 64
        receive_checks(m, fam, sh, f"{kind} {q}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. dk_tx_checksum and dk_tx_checksum_fields
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tx_packs():
    """The as-built frames with their three checksum fields scrambled. What the in-place fill must give back is the
    as-built blob, known without any oracle; the oracle's own answers ride along."""
    out = {}
    vecs = CV.base_vectors()
    for sh in CV.SHIFTS:
        blob, off, lens = CV.pack([v.frame for v in vecs], sh)
        scr = CV.scramble_fields(blob, off, vecs, seed=sh)
        ofill = scr.copy()
        for o, ln in zip(off, lens):
            fr = bytearray(scr[int(o):int(o) + int(ln)].tobytes())
            O.tx_fill_checksums(fr)
            ofill[int(o):int(o) + int(ln)] = np.frombuffer(bytes(fr), np.uint8)
        ofields = np.array([O.tx_checksum_fields(scr[int(o):int(o) + int(ln)].tobytes()) for o, ln in zip(off, lens)],
                           np.uint32)
        out[sh] = G.frozen(blob=blob, off=off, lens=lens, scr=scr, vecs=vecs, ofill=ofill, ofields=ofields,
                           fields=np.array([v.ip_target | v.target << 16 for v in vecs], np.uint32))
    return out


@pytest.fixture
def tx_split(request):
    tx_tuning(split=int(request.param))
    yield request.param
    tx_tuning()


@pytest.mark.parametrize("sh", CV.SHIFTS)
@pytest.mark.parametrize("tx_split", ["0", "1"], indirect=True)
def test_tx_checksum_restores_the_as_built_frames(torch_cuda, tx_packs, tx_split, sh):
    import torch

    m = tx_packs[sh]
    eng = RxEngine(Config(LOCAL))
    b = FrameBatch.from_numpy(m.scr.copy(), m.off.copy(), m.lens.copy())
    eng.tx_checksum(b)
    torch.cuda.synchronize()
    got = b.blob.cpu().numpy()
    bad = np.nonzero(got != m.blob)[0]
    if bad.size:
        j = int(np.searchsorted(m.off, bad[0], side="right")) - 1
        raise AssertionError(f"split={tx_split} offset {sh}: {bad.size} bytes differ from the as-built blob, first at "
                             f"byte {int(bad[0]) - int(m.off[j])} of {m.vecs[j].name}")
    assert np.array_equal(got, m.ofill)
    b2 = FrameBatch.from_numpy(m.scr.copy(), m.off.copy(), m.lens.copy())
    fields = eng.tx_checksum_fields(b2)
    torch.cuda.synchronize()
    assert np.array_equal(b2.blob.cpu().numpy(), m.scr), "dk_tx_checksum_fields wrote to the frames"
    gf = fields.cpu().numpy().view(np.uint32)[:len(m.off)]
    bad = np.nonzero(gf != m.fields)[0]
    assert bad.size == 0, (tx_split, sh, [(m.vecs[int(j)].name, hex(int(gf[j])), hex(int(m.fields[j]))) for j in bad[:6]])
    assert np.array_equal(gf, m.ofields)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. dk_tx_serialize
# ---------------------------------------------------------------------------------------------------------------------
LINKS = T.LINKS


def resteer(c0: int, target: int) -> int:
    """The steering word for `target`, given the checksum c0 a model stored with that word zero: the fold's state is
    0xFFFF - c0, congruent to the rest of the sum."""
    return CV.steer(0xFFFF - c0, target)


@pytest.fixture(scope="module")
def ser_batch():
    """The payloads of the plain as-built vectors (IHL 5, no TCP options, no padding) behind headroom, at payload
    residues 0, 1, 2 and 15 mod 16, steered again against the headers tests/tx_reference.py builds for them:
    H + payload_len reaches 65,535 for both protocols."""
    vecs = [v for v in CV.base_vectors() if v.ihl == 5 and v.doff in (5, 2) and not v.pad]
    n = len(vecs)
    res = [(0, 1, 2, 15)[(k + k // 4) % 4] for k in range(n)]
    H = np.array([54 if v.proto == 6 else 42 for v in vecs])
    poff, pos = np.zeros(n, np.int64), 0
    for k, v in enumerate(vecs):
        p = pos + int(H[k])
        p += (res[k] - p) % 16
        poff[k] = p
        pos = p + len(v.payload)
    blob = np.full(pos + 64, 0xFF, np.uint8)
    protos = np.array([v.proto for v in vecs], np.int64)
    segs = dict(payload_off=poff.astype(np.uint32), payload_len=np.array([len(v.payload) for v in vecs], np.uint16),
                meta=(protos << 8 | np.where(protos == 6, 0x18 << 16 | 5 << 28, 0)).astype(np.uint32),
                src_ip=np.full(n, ipv4(F.ALICE_IPV4), np.uint32), dst_ip=np.full(n, ipv4(F.BOB_IPV4), np.uint32),
                ports=np.array([CV.SPORT | (CV.TCP_DPORT if v.proto == 6 else CV.UDP_DPORT) << 16 for v in vecs], np.uint32),
                tcp_seq=np.array([v.seq for v in vecs], np.uint32), tcp_ack=np.array([v.ack for v in vecs], np.uint32),
                tcp_win=np.array([v.win for v in vecs], np.uint32), tcp_opts=np.zeros(n, N.TCP_OPTS_DTYPE),
                ip_word=np.zeros(n, np.uint32), link=(np.arange(n) % len(LINKS)).astype(np.uint32))
    ip_t = [CV.IP_TARGETS[k % 3] for k in range(n)]
    for k, v in enumerate(vecs):
        pay = bytearray(v.payload)
        sp = v.spos - v.P0
        pay[sp:sp + 2] = b"\0\0"
        kw = dict(meta=int(segs["meta"][k]), seq=v.seq, ack=v.ack, winurg=v.win)
        ttl = 1 + k % 255
        h = R.headers(bytes(pay), v.proto, int(segs["src_ip"][k]), int(segs["dst_ip"][k]), int(segs["ports"][k]),
                      ipw=ttl << 16, **kw)
        at = 50 if v.proto == 6 else 40
        pay[sp:sp + 2] = resteer(int.from_bytes(h[at:at + 2], "big"), v.target).to_bytes(2, "big")
        ident = resteer(int.from_bytes(h[24:26], "big"), ip_t[k])
        segs["ip_word"][k] = ip_word(ident, ttl, 0)
        blob[poff[k]:poff[k] + len(pay)] = np.frombuffer(bytes(pay), np.uint8)
    assert {int(p) % 16 for p, v in zip(poff, vecs) if len(v.frame) == 65535 and v.proto == 6} == {0, 1, 2, 15}
    assert {int(p) % 16 for p, v in zip(poff, vecs) if len(v.frame) == 65535 and v.proto == 17} == {0, 1, 2, 15}
    exp = R.serialize_batch(blob, segs, LINKS)
    return G.frozen(blob=blob, segs=segs, vecs=vecs, ip_t=np.array(ip_t, np.uint32), exp=exp, H=H)


def test_tx_serialize_extremes(torch_cuda, ser_batch):
    import torch

    m = ser_batch
    eb, eoff, elen, est = m.exp
    assert (est == R.OK).all() and int(elen.max()) == 65535
    blob = torch.from_numpy(m.blob.copy()).to("cuda:0")
    b = tx_serialize(blob, TxSegments.from_numpy(**m.segs), LINKS)
    torch.cuda.synchronize()
    gb = blob.cpu().numpy()
    assert np.array_equal(b.status.cpu().numpy().view(np.uint32), est)
    assert np.array_equal(b.off.cpu().numpy().view(np.uint32), eoff)
    assert np.array_equal(b.len.cpu().numpy().view(np.uint16), elen)
    for name, arr in (("model", eb), ("device", gb)):
        o = eoff.astype(np.int64)
        at = o + np.where(m.H == 54, 50, 40)
        l4 = arr[at].astype(np.uint32) << 8 | arr[at + 1]
        ipc = arr[o + 24].astype(np.uint32) << 8 | arr[o + 25]
        want = np.array([v.target for v in m.vecs], np.uint32)
        bad = np.nonzero((l4 != want) | (ipc != m.ip_t))[0]
        assert bad.size == 0, (name, [(m.vecs[int(j)].name, hex(int(l4[j])), hex(int(ipc[j]))) for j in bad[:6]])
    bad = np.nonzero(gb != eb)[0]
    assert bad.size == 0, f"{bad.size} blob bytes differ from the model, first at {bad[:8]}"
    # back through every receive family: both sides agree on every stored value, 0x0000 included
    want_meta = np.array([OK[v.proto] for v in m.vecs], np.uint32)
    for fam in FAMILIES:
        eng = RxEngine(Config(LOCAL), device=0, tuning=P.family(fam))
        eng.set_sockets(F.corpus_flows())
        r = eng.results(b.n, tcp_fields=True)
        eng.receive_batch(b, r)
        torch.cuda.synchronize()
        got = r.to_numpy()
        eng.close()
        assert np.array_equal(got["meta"] & 0xFF, want_meta), fam
        assert np.array_equal(got["payload"], m.H.astype(np.uint32) | m.segs["payload_len"].astype(np.uint32) << 16), fam
    assert (want_meta == OK[6]).any() and (want_meta == OK[17]).any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. dk_tcp_tx_segment
# ---------------------------------------------------------------------------------------------------------------------
STRIDE = 65600  # 0 mod 16: a payload at frame_lead + 54 sits at 6, 7 or 8 mod 16 for frame_lead 0, 1, 2
SEG_BUFS = (("ff", (0x0000,)), ("fffe", (0xFFFE,)), ("ff00", (0x0001,)), ("fffe", (0x8000, 0x00FF, None)))


@pytest.fixture(scope="module")
def sender():
    from demikernel_amd.tcp_tx import TcpSender

    s = TcpSender(0)
    yield s
    s.close()


def segment_case(mss, lead):
    """Four connections, their buffers at source residues 0, 1, 2 and 15: three buffers of exactly one mss and one of
    2 mss + 1 (pieces of mss, mss and 1 byte), each piece filled and steered against the model's header for it."""
    residues = (0, 1, 2, 15)
    conn, lens, res = [], [], []
    for c, r in enumerate(residues):
        for fill, targets in SEG_BUFS:
            conn.append(c)
            lens.append(mss if len(targets) == 1 else 2 * mss + 1)
            res.append(r)
    src, conn, off, ln = M.pack_push(conn, lens, residues=res)
    assert [int(o) % 16 for o in off] == res
    pieces = []  # (source offset of the steering word, target) in frame order
    for b, (fill, targets) in enumerate(SEG_BUFS * len(residues)):
        o = int(off[b])
        src[o:o + int(ln[b])] = np.frombuffer(CV.fill_bytes(fill, int(ln[b]), b), np.uint8)
        for j, t in enumerate(targets):
            plen = min(mss, int(ln[b]) - j * mss)
            pieces.append((o + j * mss + (plen // 2 - 1) * 2 if t is not None else None, t))
    for sp, _ in pieces:
        if sp is not None:
            src[sp:sp + 2] = 0
    flows = T.flows_for(len(residues))
    tx = M.conns_toward(flows, mss=mss)
    nfr = len(pieces)
    kw = dict(slot_stride=STRIDE, frame_lead=lead, max_frames=nfr + 2)
    out0 = np.full((nfr + 2) * STRIDE + 64, T.CANARY, np.uint8)
    exp0 = M.segment(src, conn, off, ln, tx, T.LINKS, out0, **kw)
    assert exp0["n_frames"] == nfr
    for f, (sp, t) in enumerate(pieces):
        if sp is not None:
            a = int(exp0["off_out"][f]) + 50
            c0 = int.from_bytes(exp0["out"][a:a + 2].tobytes(), "big")
            src[sp:sp + 2] = np.frombuffer(resteer(c0, t).to_bytes(2, "big"), np.uint8)
    return SimpleNamespace(src=src, conn=conn, off=off, ln=ln, tx=tx, flows=flows, pieces=pieces, kw=kw,
                           out_size=out0.size)


@pytest.mark.parametrize("lead", [0, 1, 2])
@pytest.mark.parametrize("mss", [1460, 32768, 65481])
def test_tcp_tx_segment_extremes(torch_cuda, sender, mss, lead):
    import torch

    s = segment_case(mss, lead)
    got, exp = T.check(sender, s.src, s.conn, s.off, s.ln, s.tx, out_size=s.out_size, **s.kw)
    assert (exp["status"] == M.SENT).all() and exp["n_frames"] == len(s.pieces)
    assert int(exp["len_out"].max()) == 54 + mss
    parity = set()
    for f, (sp, t) in enumerate(s.pieces):
        a = int(exp["off_out"][f])
        for name, arr in (("model", exp["out"]), ("device", got["out"])):
            stored = int.from_bytes(arr[a + 50:a + 52].tobytes(), "big")
            assert t is None or stored == t, (name, f, hex(stored), hex(t))
        so = int(s.off[exp["frame_buf"][f]]) + (f - int(exp["first_frame"][exp["frame_buf"][f]])) * mss
        parity.add((so % 2, (a + 54) % 2))
    # both source parities on this destination grid (the three values of frame_lead give both grids)
    assert parity == {(0, lead % 2), (1, lead % 2)}, parity
    # the frames back through every receive family: every one OK_TCP, every payload view the source bytes
    batch = FrameBatch.from_numpy(got["out"], got["off_out"], got["len_out"])
    frames = got["out"]
    for fam in FAMILIES:
        eng = RxEngine(Config(LOCAL), device=0, tuning=P.family(fam))
        eng.set_sockets(s.flows)
        r = eng.results(batch.n, tcp_fields=True)
        eng.receive_batch(batch, r)
        torch.cuda.synchronize()
        rx = r.to_numpy()
        eng.close()
        assert ((rx["meta"] & 0xFF) == OK[6]).all(), (fam, rx["meta"] & 0xFF)
        for f in range(batch.n):
            b = int(exp["frame_buf"][f])
            so = int(s.off[b]) + (f - int(exp["first_frame"][b])) * mss
            po, pl = int(rx["payload"][f]) & 0xFFFF, int(rx["payload"][f]) >> 16
            assert po == 54 and pl == int(got["len_out"][f]) - 54, (fam, f)
            a = int(got["off_out"][f]) + po
            assert np.array_equal(frames[a:a + pl], s.src[so:so + pl]), (fam, f)


def test_mss_65481_is_one_full_frame_the_receive_path_accepts(torch_cuda, sender):
    import torch

    flows = T.flows_for(1)
    tx = M.conns_toward(flows, mss=65481)
    src, conn, off, ln = M.pack_push([0], [65481], residues=[3])
    got, exp = T.check(sender, src, conn, off, ln, tx, slot_stride=65535, frame_lead=0, max_frames=1, out_size=65535)
    assert list(exp["status"]) == [M.SENT] and list(got["len_out"]) == [65535] and list(got["off_out"]) == [0]
    batch = FrameBatch.from_numpy(got["out"], got["off_out"], got["len_out"])
    eng = RxEngine(Config(LOCAL), device=0)
    eng.set_sockets(flows)
    r = eng.results(1, tcp_fields=True)
    eng.receive_batch(batch, r)
    torch.cuda.synchronize()
    rx = r.to_numpy()
    eng.close()
    assert int(rx["meta"][0]) & 0xFF == OK[6] and int(rx["payload"][0]) == 54 | 65481 << 16
    assert int(rx["tcp_seq"][0]) == int(tx["snd_nxt"][0])


def test_mss_65482_fails_only_that_connection(sender):
    """54 + mss must fit the 16-bit len_out: one byte more is the connection error mss > 65,495 was, between two
    healthy connections; neither the stride nor anything else stands in its way."""
    tx = M.conns_toward(T.flows_for(3), mss=[1460, 65482, 65481])
    src, conn, off, ln = M.pack_push([0, 1, 1, 2], [3000, 70000, 0, 65481])
    got, exp = T.check(sender, src, conn, off, ln, tx, slot_stride=STRIDE, frame_lead=0, max_frames=8)
    assert list(exp["status"]) == [M.SENT, M.E_CONN, M.E_CONN, M.SENT] and exp["n_frames"] == 4
    assert list(got["len_out"]) == [1514, 1514, 134, 65535]
    assert got["tx_conns"][1].tobytes() == tx[1].tobytes()
