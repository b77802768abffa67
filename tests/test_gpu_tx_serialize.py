"""dk_tx_serialize on the MI355X: headers and outputs bit-exact against tests/tx_reference.py (pinned on the CPU by
tests/test_tx_serialize_abi.py). Every comparison is over the whole blob, so a stray write anywhere fails."""
import ctypes

import numpy as np
import pytest

import frames as F
import tx_reference as R
from demikernel_amd import Config, RxEngine, TxSegments, ipv4, synth, tx_links, tx_serialize
from demikernel_amd import _native as N
from demikernel_amd.tx import ip_word
from oracle.oracle import OraclePeer

pytestmark = pytest.mark.gpu

BOB = ipv4(synth.BOB_IPV4)
LINKS = tx_links([(synth.BOB_MAC, synth.ALICE_MAC), (bytes([2, 0, 0, 0xAA, 0xBB, 0xCC]), bytes([0xFE, 1, 2, 3, 4, 5]))])
PLENS = [0, 1, 2, 15, 16, 17, 49, 50, 63, 64, 65, 1446, 1460, 8960]
EINVAL = 22


def build(protos, plens, residues=None, entries=None, *, packed=False, seed=1, clean=False, fill=None):
    """A blob and the dk_tx_segs arrays of len(protos) segments. residues: each payload's address mod 16 (the blob is
    16-byte aligned on the device); packed: zero slack instead, segment i + 1's header room begins at the byte after
    segment i's payload. Header fields are random; unless `clean`, meta carries junk in the bits the call ignores
    (low byte, bits 25-27) and no-option TCP segments use the data-offset nibbles 0 and 5 alike. fill: the byte the
    blob outside the payloads holds before the call (None: random)."""
    rng = np.random.default_rng(seed)
    n = len(protos)
    protos, plens = np.asarray(protos, np.int64), np.asarray(plens, np.int64)
    recs = np.zeros(n, N.TCP_OPTS_DTYPE)
    H = np.where(protos == 17, 42, 54)
    if entries is not None:
        for i, e in enumerate(entries):
            if e:
                recs[i] = R.opts_record(e)[0]
                H[i] = R.header_bytes(6, recs[i])
    poff = np.zeros(n, np.int64)
    pos = 0
    for i in range(n):
        p = pos + int(H[i])
        if not packed:
            p += (int(residues[i]) - p) % 16
        poff[i] = p
        pos = p + int(plens[i])
    blob = rng.integers(0, 256, max(pos, 1), dtype=np.uint8)
    if fill is not None:
        keep = np.zeros(blob.size, bool)
        for i in range(n):
            keep[poff[i]:poff[i] + plens[i]] = True
        blob[~keep] = fill
    nib = (H - 34) // 4
    if not clean:
        nib = np.where((nib == 5) & (rng.random(n) < 0.5), 0, nib)
    meta = protos << 8 | rng.integers(0, 256, n) << 16 | rng.integers(0, 2, n) << 24 | nib << 28
    if clean:
        meta = np.where(protos == 6, meta, protos << 8)
    else:
        meta |= rng.integers(0, 256, n) | rng.integers(0, 8, n) << 25
    segs = dict(
        payload_off=poff.astype(np.uint32), payload_len=plens.astype(np.uint16), meta=meta.astype(np.uint32),
        src_ip=(10 | rng.integers(0, 1 << 16, n) << 8 | rng.integers(1, 255, n) << 24).astype(np.uint32),
        dst_ip=np.full(n, BOB, np.uint32),
        ports=(rng.integers(1024, 65536, n) | np.where(protos == 6, 12345, 5000) << 16).astype(np.uint32),
        tcp_seq=rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
        tcp_ack=rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
        tcp_win=rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
        tcp_opts=recs,
        ip_word=ip_word(rng.integers(0, 65536, n), rng.integers(1, 256, n), rng.integers(0, 256, n)).astype(np.uint32),
        link=rng.integers(0, len(LINKS), n).astype(np.uint32))
    return blob, segs


def run_gpu(blob_np, segs, links=LINKS, flags=0, status=True):
    import torch

    blob = torch.from_numpy(np.array(blob_np, np.uint8, copy=True)).to("cuda:0")
    assert blob.data_ptr() % 16 == 0
    ts = TxSegments.from_numpy(**segs)
    b = tx_serialize(blob, ts, links, offload_tcp=bool(flags & R.OFFLOAD_TCP), offload_udp=bool(flags & R.OFFLOAD_UDP),
                     status=status)
    torch.cuda.synchronize()
    st = b.status.cpu().numpy().view(np.uint32) if status else None
    return blob.cpu().numpy(), b.off.cpu().numpy().view(np.uint32), b.len.cpu().numpy().view(np.uint16), st, b


def assert_same(got, exp, segs):
    gb, goff, glen, gst = got[:4]
    eb, eoff, elen, est = exp
    if gst is not None:
        assert np.array_equal(gst, est), (np.nonzero(gst != est)[0][:8], gst[gst != est][:8], est[gst != est][:8])
    assert np.array_equal(goff, eoff), np.nonzero(goff != eoff)[0][:8]
    assert np.array_equal(glen, elen), np.nonzero(glen != elen)[0][:8]
    if not np.array_equal(gb, eb):
        bad = np.nonzero(gb != eb)[0]
        i = int(np.searchsorted(np.sort(segs["payload_off"].astype(np.int64)), bad[0], side="right"))
        raise AssertionError(f"{len(bad)} blob bytes differ, first at {bad[:8]} (near the {i}-th payload by offset): "
                             f"got {gb[bad[:8]]} expected {eb[bad[:8]]}")


def check(blob, segs, links=LINKS, flags=0):
    exp = R.serialize_batch(blob, segs, links, flags)
    got = run_gpu(blob, segs, links, flags)
    assert_same(got, exp, segs)
    return got, exp


# ---------------------------------------------------------------------------------------------------------------------
# 1. shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_every_length_at_every_residue():
    """Both protocols x the payload lengths that cross the register-window / streamed boundary x every payload address
    residue mod 16 (even: vector path at every shift; odd: byte path)."""
    combos = [(p, ln, r) for p in (6, 17) for ln in PLENS for r in range(16)]
    blob, segs = build([c[0] for c in combos], [c[1] for c in combos], [c[2] for c in combos], seed=11)
    (_, off, ln, st, _), _ = check(blob, segs)
    assert (st == R.OK).all()
    assert np.array_equal(segs["payload_off"] % 16, [c[2] for c in combos])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_a_chunk(n):
    rng = np.random.default_rng(100 + n)
    blob, segs = build(rng.choice([6, 17], n), rng.choice(PLENS[:-1], n), rng.integers(0, 16, n), seed=n)
    (_, _, _, st, _), _ = check(blob, segs)
    assert (st == R.OK).all()


def _mixed(n, seed, packed=False, fill=None, clean=False, with_options=True):
    rng = np.random.default_rng(seed)
    protos = rng.choice([6, 17], n, p=[0.7, 0.3])
    plens = rng.choice(PLENS, n, p=[.08, .08, .08, .08, .08, .08, .08, .08, .08, .08, .08, .05, .06, .01])
    cases = R.option_cases()
    if clean:
        cases = [c for c in cases if not any(e[0] in ("nop", "eol") for e in c[1])]
    entries = [cases[rng.integers(len(cases))][1] if with_options and p == 6 and rng.random() < 0.1 else None
               for p in protos]
    # mostly the common layouts (16-byte aligned payloads, NIC buffers at 2 mod 16), the rest anywhere
    res = np.where(rng.random(n) < 0.5, 0, np.where(rng.random(n) < 0.5, 2, rng.integers(0, 16, n)))
    return build(protos, plens, res, entries, packed=packed, seed=seed + 1, fill=fill, clean=clean)


_LARGE = {}


def _large():
    """About 20,000 mixed segments and their reference, computed once for the cases below."""
    if not _LARGE:
        blob, segs = _mixed(20011, 5)
        _LARGE.update(blob=blob, segs=segs, exp=R.serialize_batch(blob, segs, LINKS))
    return _LARGE["blob"], _LARGE["segs"], _LARGE["exp"]


@pytest.mark.parametrize("grid,sched", [(-1, -1), (3, 0), (5, 1)])
def test_large_mixed_batch(grid, sched):
    """A ragged last chunk under the engine's own grid, and several chunks per wave under a grid capped at a few
    workgroups (26 and 15 chunks per wave), in both schedules: round-robin tiles and one contiguous share per wave."""
    from demikernel_amd import tx_tuning
    from demikernel_amd.tx import tx_serialize_grid

    blob, segs, exp = _large()
    tx_serialize_grid(grid)
    tx_tuning(sched=sched)
    try:
        got = run_gpu(blob, segs)
    finally:
        tx_serialize_grid()
        tx_tuning()
    assert_same(got, exp, segs)
    assert (got[3] == R.OK).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. packed layout: a payload's first and last granules hold header room that another wave may be writing
# ---------------------------------------------------------------------------------------------------------------------
def test_packed_layout_is_independent_of_the_headroom():
    n = 3000
    blob_ff, segs = _mixed(n, 7, packed=True, fill=0xFF)
    blob_rnd, segs2 = _mixed(n, 7, packed=True)
    assert all(np.array_equal(segs[k], segs2[k]) for k in segs)
    ends = (segs["payload_off"].astype(np.int64) + segs["payload_len"]) % 16
    assert set(ends.tolist()) == set(range(16))  # payload ends at every residue mod 16
    (a, off, *_), (ea, *_) = check(blob_ff, segs)
    # zero slack: the first header room starts the blob, every other one begins at the byte after the previous payload
    assert off[0] == 0 and np.array_equal(off[1:], segs["payload_off"][:-1] + segs["payload_len"][:-1])
    (b, *_), (eb, *_) = check(blob_rnd, segs)
    assert np.array_equal(a, b) and np.array_equal(ea, eb)  # no slack: every byte is payload or a rebuilt header


# ---------------------------------------------------------------------------------------------------------------------
# 3. options
# ---------------------------------------------------------------------------------------------------------------------
def test_option_lists_and_unread_records():
    cases = R.option_cases()
    protos, plens, res, entries = [], [], [], []
    for k, (name, e, _) in enumerate(cases * 4):
        protos += [6, 6, 17]
        plens += [PLENS[k % 11], 1460, 33]
        res += [(2 * k) % 16, 0, k % 16]  # option-bearing segments at every even residue, then odd ones below
        entries += [e, None, None]
    for k, (name, e, _) in enumerate(cases):
        protos.append(6), plens.append(100 + k), res.append((2 * k + 1) % 16), entries.append(e)
    blob, segs = build(protos, plens, res, entries, seed=3)
    # data segments (nibble 0 / 5) and UDP carry a poisoned record: it must not be read
    plain = np.array([e is None for e in entries])
    poison = np.frombuffer(b"\xFF" * 96, N.TCP_OPTS_DTYPE)[0]
    segs["tcp_opts"][plain] = poison
    assert ((segs["meta"][plain] >> 28 <= 5) | (segs["meta"][plain] >> 8 & 0xFF == 17)).all()
    (_, _, ln, st, _), _ = check(blob, segs)
    assert (st == R.OK).all()
    want = [R.header_bytes(p, R.opts_record(e)[0] if e else None) + ln_ for p, e, ln_ in zip(protos, entries, plens)]
    assert np.array_equal(ln, want)


# ---------------------------------------------------------------------------------------------------------------------
# 4. offload flags
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_offload_flags(flags):
    blob, segs = _mixed(500, 9)
    (gb, off, _, st, _), _ = check(blob, segs, flags=flags)
    assert (st == R.OK).all()
    tcp = (segs["meta"] >> 8 & 0xFF) == 6
    at = off.astype(np.int64) + np.where(tcp, 50, 40)
    stored = gb[at].astype(np.uint32) << 8 | gb[at + 1]
    flagged = np.where(tcp, bool(flags & R.OFFLOAD_TCP), bool(flags & R.OFFLOAD_UDP))
    assert (stored[flagged] == 0).all()  # the other frames' checksums are pinned by the whole-blob comparison above


# ---------------------------------------------------------------------------------------------------------------------
# 5. statuses and the call contract
# ---------------------------------------------------------------------------------------------------------------------
def _status_batch():
    fb = 140000
    blob = np.random.default_rng(13).integers(0, 256, fb, dtype=np.uint8)
    bad_kind = R.opts_record([("raw", 9)])[0]
    mss = R.opts_record([("mss", 1460)])[0]  # 8 option bytes: nibble 7
    rows, want = [], []

    def add(status, proto, poff, plen, nib=0, rec=None, link=0):
        rows.append((poff, plen, proto << 8 | 0x18 << 16 | nib << 28, link, rec))
        want.append(status)

    add(R.OK, 17, 128, 30)
    add(R.E_PROTO, 1, 256, 10)
    add(R.OK, 6, 384, 100, nib=5)
    add(R.E_OPTS, 6, 640, 10, nib=6, rec=bad_kind)
    add(R.E_OPTS, 6, 768, 10, nib=6, rec=mss)               # the list needs nibble 7
    add(R.OK, 6, 896, 10, nib=7, rec=mss)
    add(R.E_LINK, 17, 1024, 10, link=len(LINKS))
    add(R.OK, 17, 1152, 7, link=len(LINKS) - 1)
    add(R.E_LEN, 17, 2048, 65535 - 41)                      # H + payload_len = 65536
    add(R.OK, 17, 70000, 65535 - 42)                        # H + payload_len = 65535
    add(R.E_RANGE, 17, 41, 4)                               # payload_off = H - 1
    add(R.E_RANGE, 6, fb - 10, 11, nib=5)                   # payload_off + payload_len = frames_bytes + 1
    add(R.OK, 6, fb, 0, nib=5)                              # a zero-length payload ending exactly at frames_bytes
    add(R.E_PROTO, 0, 1280, 10, link=99)                    # two kinds: the earlier one is reported
    add(R.E_OPTS, 6, 20, 10, nib=6, rec=bad_kind)           # options and range
    add(R.E_LINK, 17, 30, 65535, link=7)                    # link, length and range
    add(R.E_OPTS, 6, 1408, 10, nib=3)                       # a data offset below 5 words
    add(R.OK, 17, 1536, 64)
    n = len(rows)
    recs = np.zeros(n, N.TCP_OPTS_DTYPE)
    for i, r in enumerate(rows):
        if r[4] is not None:
            recs[i] = r[4]
    rng = np.random.default_rng(14)
    segs = dict(payload_off=np.array([r[0] for r in rows], np.uint32), payload_len=np.array([r[1] for r in rows], np.uint16),
                meta=np.array([r[2] for r in rows], np.uint32), src_ip=np.full(n, ipv4("10.0.0.1"), np.uint32),
                dst_ip=np.full(n, BOB, np.uint32), ports=rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
                tcp_seq=np.arange(n, dtype=np.uint32), tcp_ack=np.arange(n, dtype=np.uint32) * 7,
                tcp_win=np.full(n, 0x00010400, np.uint32), tcp_opts=recs, link=np.array([r[3] for r in rows], np.uint32))
    return blob, segs, np.array(want, np.uint32)


def test_statuses_interleaved_with_good_frames():
    blob, segs, want = _status_batch()
    (gb, off, ln, st, _), _ = check(blob, segs)
    assert np.array_equal(st, want)
    bad = st != R.OK
    assert (off[bad] == 0).all() and (ln[bad] == 0).all() and (ln[~bad] > 0).all()
    assert set(want.tolist()) == {R.OK, R.E_PROTO, R.E_OPTS, R.E_LINK, R.E_LEN, R.E_RANGE}
    # only the good frames' header rooms changed
    changed = np.nonzero(gb != blob)[0]
    room = np.zeros(blob.size, bool)
    for o, p in zip(off[~bad], segs["payload_off"][~bad]):
        room[o:p] = True
    assert room[changed].all()


def test_status_null_and_no_option_records():
    """status = NULL works; a nibble above 5 with tcp_opts == NULL is DK_TX_E_OPTS."""
    blob, segs, want = _status_batch()
    exp = R.serialize_batch(blob, segs, LINKS)
    got = run_gpu(blob, segs, status=False)
    assert got[3] is None
    assert_same(got, exp, segs)
    segs = dict(segs, tcp_opts=None, ip_word=None, link=None, tcp_seq=None, tcp_ack=None, tcp_win=None)
    exp = R.serialize_batch(blob, segs, LINKS)
    assert (exp[3][(segs["meta"] >> 28) > 5] == R.E_OPTS).all()
    assert_same(run_gpu(blob, segs), exp, segs)


def test_call_contract():
    import torch

    lib = N.load_library()
    blob, segs = build([6, 17], [10, 10], [0, 0], seed=2)
    dev = torch.device("cuda", 0)
    t_blob = torch.from_numpy(blob).to(dev)
    before = t_blob.clone()
    ts = TxSegments.from_numpy(**segs)
    links = torch.from_numpy(LINKS.view(np.uint8).copy()).to(dev)
    off = torch.full((2,), -1, dtype=torch.int32, device=dev)
    ln = torch.full((2,), -1, dtype=torch.int16, device=dev)

    def call(cs, frames_bytes=t_blob.numel(), nlinks=len(LINKS), links_ptr=links.data_ptr(), off_ptr=off.data_ptr()):
        return lib.dk_tx_serialize(t_blob.data_ptr(), frames_bytes, ctypes.byref(cs), links_ptr, nlinks, off_ptr,
                                   ln.data_ptr(), None, None)

    empty = ts.c_struct()
    empty.n = 0
    assert call(empty) == 0                                    # n = 0: no launch
    nul = ts.c_struct()
    nul.payload_off = None
    assert call(nul) == EINVAL
    assert call(ts.c_struct(), nlinks=0) == EINVAL
    assert call(ts.c_struct(), links_ptr=None) == EINVAL
    assert call(ts.c_struct(), off_ptr=None) == EINVAL
    assert call(ts.c_struct(), frames_bytes=0xFFFFFF01) == EINVAL  # > DK_RX_MAX_BLOB
    assert lib.dk_tx_serialize(None, 0, None, None, 0, None, None, None, None) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(t_blob, before) and (off == -1).all() and (ln == -1).all()  # nothing ran
    assert call(ts.c_struct()) == 0
    torch.cuda.synchronize()
    exp = R.serialize_batch(blob, segs, LINKS)
    assert np.array_equal(t_blob.cpu().numpy(), exp[0])
    assert np.array_equal(off.cpu().numpy().view(np.uint32), exp[1])


def test_stream_that_is_not_the_current_one():
    """The call on a side stream while torch's current stream is still busy: the wrapper queues nothing on the current
    stream that could land on the outputs after the kernel (a zero fill there gave off = len = status = 0 for every
    segment). Fresh outputs and caller-provided ones."""
    import torch

    blob, segs = _mixed(3000, 61)
    exp = R.serialize_batch(blob, segs, LINKS)
    dev = torch.device("cuda", 0)
    ts = TxSegments.from_numpy(**segs)
    links = torch.from_numpy(LINKS.view(np.uint8).copy()).to(dev)
    side = torch.cuda.Stream(device=dev)
    busy = torch.ones(1 << 26, dtype=torch.float32, device=dev)
    for pre in (False, True):
        t_blob = torch.from_numpy(blob.copy()).to(dev)
        out = None
        if pre:
            out = (torch.full((ts.n,), -1, dtype=torch.int32, device=dev),
                   torch.full((ts.n,), -1, dtype=torch.int16, device=dev),
                   torch.full((ts.n,), -1, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        for _ in range(20):  # a few ms of work queued on the current stream, ahead of anything the wrapper might add to it
            busy.mul_(1.0001)
        b = tx_serialize(t_blob, ts, links, stream=side, out=out)
        side.synchronize()  # the kernel is done while the current stream is still working
        got = (t_blob.cpu().numpy(), b.off.cpu().numpy().view(np.uint32), b.len.cpu().numpy().view(np.uint16),
               b.status.cpu().numpy().view(np.uint32))
        torch.cuda.synchronize()
        again = (b.off.cpu().numpy().view(np.uint32), b.len.cpu().numpy().view(np.uint16))
        assert_same(got, exp, segs)
        assert np.array_equal(again[0], exp[1]) and np.array_equal(again[1], exp[2])  # still there afterwards
        if pre:
            assert b.off is out[0] and b.len is out[1] and b.status is out[2]


# ---------------------------------------------------------------------------------------------------------------------
# 6. loopback: dk_tx_serialize -> dk_rx_process over the returned descriptors, on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offload", [False, True])
def test_loopback_through_the_receive_path(offload):
    import torch

    n = 4000
    blob, segs = _mixed(n, 21, clean=True)
    flags = (R.OFFLOAD_TCP | R.OFFLOAD_UDP) if offload else 0
    *_, batch = run_gpu(blob, segs, flags=flags)
    assert (batch.status == 0).all()
    eng = RxEngine(Config(synth.BOB_IPV4, tcp_checksum_offload=offload, udp_checksum_offload=offload), device=0)
    eng.set_sockets(F.corpus_flows())  # a listener on BOB:12345 and a UDP bind on BOB:5000
    res = eng.results(n, tcp_fields=True, tcp_opts=True)
    eng.receive_batch(batch, res)
    torch.cuda.synchronize()
    got = res.to_numpy()
    tcp = (segs["meta"] >> 8 & 0xFF) == 6
    assert np.array_equal(got["meta"] & 0xFF, np.where(tcp, N.V["OK_TCP"], N.V["OK_UDP"]))
    assert np.array_equal(got["meta"] >> 8, segs["meta"] >> 8)
    for k in ("src_ip", "dst_ip", "ports"):
        assert np.array_equal(got[k], segs[k]), k
    for k in ("tcp_seq", "tcp_ack", "tcp_win"):
        assert np.array_equal(got[k][tcp], segs[k][tcp]), k
    H = batch.len.cpu().numpy().view(np.uint16).astype(np.uint32) - segs["payload_len"]
    assert np.array_equal(got["payload"], H | segs["payload_len"].astype(np.uint32) << 16)
    assert got["tcp_opts"].tobytes() == segs["tcp_opts"].tobytes()
    assert ((segs["meta"] >> 28) > 5).sum() > 100
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. identity: parse, wipe the headers, serialize from the parse results -> the original bytes
# ---------------------------------------------------------------------------------------------------------------------
def test_parse_then_serialize_is_the_identity():
    import torch

    n = 4096
    flows = np.concatenate([synth.make_flows(256), synth.make_flows(64, kind="udp")])
    tr = synth.traffic(n, synth.imix_ip_lengths(n, seed=31), flows, seed=31)
    blob, off, lens = synth.build_numpy(tr, seed=31)
    o64 = off.astype(np.int64)
    tcp = tr.proto == 6
    # precondition: no stored checksum is RFC 1071's 0xFFFF (the reference's fold stores 0 there); counted, not assumed
    ip_c = blob[o64 + 24].astype(np.uint32) << 8 | blob[o64 + 25]
    at = o64 + np.where(tcp, 50, 40)
    l4_c = blob[at].astype(np.uint32) << 8 | blob[at + 1]
    assert int((ip_c == 0xFFFF).sum()) + int((l4_c == 0xFFFF).sum()) == 0
    peer = OraclePeer(BOB)
    peer.set_flows(flows)
    r = peer.process(blob, off, lens)
    assert np.array_equal(r["meta"] & 0xFF, np.where(tcp, N.V["OK_TCP"], N.V["OK_UDP"]))
    hdr = (r["payload"] & 0xFFFF).astype(np.int64)
    wiped = blob.copy()
    for h in (42, 54):
        idx = np.nonzero(hdr == h)[0]
        wiped[o64[idx][:, None] + np.arange(h)] = 0xA5
    assert int((hdr == 42).sum() + (hdr == 54).sum()) == n and (wiped != blob).any()
    t_blob = torch.from_numpy(wiped).to("cuda:0")
    segs = TxSegments.from_rx_results(r, (o64 + hdr).astype(np.uint32), (r["payload"] >> 16).astype(np.uint16),
                                      ip_word=ip_word(tr.ip_id, tr.ttl))
    batch = tx_serialize(t_blob, segs, tx_links([(synth.BOB_MAC, synth.ALICE_MAC)]))
    torch.cuda.synchronize()
    assert (batch.status == 0).all()
    assert np.array_equal(batch.off.cpu().numpy().view(np.uint32), off)
    # the frame without its Ethernet padding (a frame below 60 bytes is padded on the wire, not by the stack)
    assert np.array_equal(batch.len.cpu().numpy().view(np.uint16), 14 + tr.ip_len)
    assert np.array_equal(t_blob.cpu().numpy(), blob)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the product checksum kernel agrees with what serialize stored
# ---------------------------------------------------------------------------------------------------------------------
def test_checksum_fields_of_a_serialized_batch():
    import torch

    n = 3000
    blob, segs = _mixed(n, 41)
    gb, off, ln, st, batch = run_gpu(blob, segs)
    assert (st == R.OK).all()
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    fields = eng.tx_checksum_fields(batch)
    torch.cuda.synchronize()
    got = fields.cpu().numpy().view(np.uint32)[:n]
    o64 = off.astype(np.int64)
    tcp = (segs["meta"] >> 8 & 0xFF) == 6
    at = o64 + np.where(tcp, 50, 40)
    stored = (gb[o64 + 24].astype(np.uint32) << 8 | gb[o64 + 25]) | (gb[at].astype(np.uint32) << 8 | gb[at + 1]) << 16
    assert np.array_equal(got, stored)
    assert np.array_equal(batch.blob.cpu().numpy(), gb)  # the fields form only reads
    eng.close()
