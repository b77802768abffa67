"""dk_tcp_retransmit on the MI355X against tests/tcp_rtx_reference.py (pinned on the CPU by tests/test_tcp_rtx_model.py
against the recordings of tests/ack_net.py). Every call is compared whole: the output blob (a canary fill proves that
nothing outside the frames is written), every result array, the ACK table as bytes, the whole pool, and the TX table
and the source unchanged."""
import errno

import numpy as np
import pytest

import tcp_rtx_reference as X
import tx_segment_reference as M
from demikernel_amd import Config, Fail, RxEngine, synth
from demikernel_amd import _native as N
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_ack import TcpAcker, UnackedQueue, ack_conn_table
from demikernel_amd.tcp_rtx import RtxResults, fire_to_device, retransmit, retransmit_batch
from demikernel_amd.tcp_tx import TcpSender

pytestmark = pytest.mark.gpu

CANARY = 0xA5
LINKS = M.links_table()
MAX_BLOB = 0xFFFFFF00  # DK_RX_MAX_BLOB
CAP = 3  # pool entries per connection: the live ones are the second and the third
LENS = [0, 1, 15, 16, 17, 96, 1460]
SIZES = [1, 63, 64, 65, 1024, 1025, 2049]  # the scan tile is 1,024 items: the last two cross it, 2,049 takes a third
MASKS = ["none", "all", "second", "last", "kinds"]


@pytest.fixture(scope="module")
def sender():
    s = TcpSender(0)
    yield s
    s.close()


def mask(kind: str, n: int) -> np.ndarray:
    c = np.arange(n)
    if kind == "none":
        return np.zeros(n, np.uint8)
    if kind == "all":
        return np.full(n, X.FIRE_TIMEOUT, np.uint8)
    if kind == "second":
        return np.where(c % 2, X.FIRE_FAST, 0).astype(np.uint8)
    if kind == "last":
        return np.where(c == n - 1, X.FIRE_TIMEOUT, 0).astype(np.uint8)
    return np.where(c % 2, X.FIRE_FAST, X.FIRE_TIMEOUT).astype(np.uint8)


def table(lens, residues=None, seed=3, mss=1460):
    """n connections, connection c with two live entries at pool[c * CAP + 1 ..]: the front has lens[c] bytes at a
    source offset of residue residues[c] mod 16, behind it 5 more bytes; the first entry of each region is dead. Every
    fifth connection's SND.UNA is 0xFFFFFFF0, so the sequence number wraps inside its frame."""
    n = len(lens)
    rng = np.random.default_rng(seed)
    flows = synth.make_flows(n, passive=False)
    una = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    una[::5] = 0xFFFFFFF0
    tx = M.conns_toward(flows, seed=seed, snd_una=una, snd_nxt=una + np.asarray(lens, np.uint64) + 6, mss=mss)
    ak = ack_conn_table(n, q_first=np.arange(n) * CAP + 1, q_count=2)
    ak["rtx_armed"] = 1
    ak["rto"] = rng.choice([0.1, 0.25, 1.0, 3.5, 45.0], n)
    ak["srtt"], ak["rttvar"] = rng.random(n), rng.random(n)
    ak["rtx_base_ns"] = rng.integers(1, 1 << 40, n, dtype=np.uint64)
    pool = {"off": rng.integers(0, 1 << 32, n * CAP, dtype=np.uint64).astype(np.uint32),
            "len": rng.integers(0, 1 << 32, n * CAP, dtype=np.uint64).astype(np.uint32),
            "tx_time": rng.integers(1, 1 << 50, n * CAP, dtype=np.uint64)}
    pos = 0
    for c, l in enumerate(lens):
        if residues is not None:
            pos += (int(residues[c]) - pos) % 16
        e = c * CAP + 1
        pool["off"][e], pool["len"][e] = pos, l
        pool["off"][e + 1], pool["len"][e + 1] = pos + l, 5
        pos += int(l) + 5
    src = rng.integers(0, 256, pos + 3, dtype=np.uint8)
    return flows, src, tx, ak, pool


def run_gpu(sender, src, fire, tx, ak, pool, now, *, slot_stride, frame_lead=0, max_frames, out_size, rx_conns=None,
            flags=0, out_bytes=None, src_bytes=None, links=LINKS, frame_conn=True):
    import torch

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    d_src, d_out = up(src), torch.full((out_size,), CANARY, dtype=torch.uint8, device=dev)
    d_tx, d_ak, d_links = sender.conns_to_device(tx), TcpAcker.conns_to_device(ak), up(links)
    d_rx = None if rx_conns is None else up(rx_conns)
    queue = UnackedQueue.from_numpy(pool["off"], pool["len"], pool["tx_time"])
    res = RtxResults(max_frames, len(fire), frame_conn=frame_conn)
    res.status.fill_(-1), res.frame.fill_(7), res.n_frames.fill_(-1)
    retransmit(sender, d_src, fire_to_device(fire), d_tx, d_ak, queue, now, d_links, d_out, res, rx_conns=d_rx,
               slot_stride=slot_stride, frame_lead=frame_lead, flags=flags, out_bytes=out_bytes, src_bytes=src_bytes,
               max_frames=max_frames)
    torch.cuda.synchronize()
    got = res.to_numpy()
    w = got["frames_written"]  # entries of the per-frame arrays past the frames written are untouched
    assert not res.off_out.cpu().numpy()[w:].any() and not res.len_out.cpu().numpy()[w:].any()
    got.update(out=d_out.cpu().numpy(), ack_conns=TcpAcker.conns_to_host(d_ak), pool=queue.to_numpy(),
               tx_conns=sender.conns_to_host(d_tx), src=d_src.cpu().numpy(),
               rx_conns=None if d_rx is None else d_rx.cpu().numpy())
    return got


def check(sender, src, fire, tx, ak, pool, now=123456789012, *, slot_stride=1536, frame_lead=0, max_frames=None,
          out_size=None, **kw):
    n = len(fire)
    if max_frames is None:
        max_frames = n + 2
    if out_size is None:
        out_size = max_frames * slot_stride + 64
    exp = X.retransmit(src, fire, tx, ak, pool, now, kw.get("links", LINKS), np.full(out_size, CANARY, np.uint8),
                       slot_stride=slot_stride, frame_lead=frame_lead, max_frames=max_frames,
                       rx_conns=kw.get("rx_conns"), flags=kw.get("flags", 0), src_bytes=kw.get("src_bytes"),
                       out_bytes=kw.get("out_bytes"))
    got = run_gpu(sender, src, fire, tx, ak, pool, now, slot_stride=slot_stride, frame_lead=frame_lead,
                  max_frames=max_frames, out_size=out_size, **kw)
    assert got["n_frames"] == exp["n_frames"]
    for k in ("status", "frame", "off_out", "len_out", "frame_conn"):
        if k not in got:
            continue
        g, e = got[k], exp[k]
        assert len(g) == len(e), (k, len(g), len(e))
        assert np.array_equal(g, e), (k, np.nonzero(g != e)[0][:8], g[g != e][:8], e[g != e][:8])
    ga, ea = got["ack_conns"], exp["ack_conns"]
    assert ga.tobytes() == ea.tobytes(), [(c, k) for c in range(n) for k in ga.dtype.names
                                           if ga[k][c].tobytes() != ea[k][c].tobytes()][:8]
    for k in ("off", "len", "tx_time"):
        assert np.array_equal(got["pool"][k], exp["pool"][k]), (k, np.nonzero(got["pool"][k] != exp["pool"][k])[0][:8])
    if not np.array_equal(got["out"], exp["out"]):
        bad = np.nonzero(got["out"] != exp["out"])[0]
        raise AssertionError(f"{len(bad)} output bytes differ, first at {bad[:8]} (slot {bad[0] // slot_stride}): got "
                             f"{got['out'][bad[:8]]} expected {exp['out'][bad[:8]]}")
    assert got["tx_conns"].tobytes() == np.ascontiguousarray(tx).tobytes(), "the TX table was written"
    assert np.array_equal(got["src"], src), "the source blob was written"
    if kw.get("rx_conns") is not None:
        assert got["rx_conns"].tobytes() == np.ascontiguousarray(kw["rx_conns"]).tobytes(), "the RX table was written"
    return got, exp


# ---------------------------------------------------------------------------------------------------------------------
# 1. table sizes x masks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_masks(sender, n, kind):
    """Front lengths cycle through FIN, 1, 15, 16, 17 and 96 bytes, every 32nd is a 1,460-byte one; the source offsets
    fall where they fall."""
    lens = [1460 if c % 32 == 31 else LENS[c % 6] for c in range(n)]
    flows, src, tx, ak, pool = table(lens, seed=n)
    fire = mask(kind, n)
    got, exp = check(sender, src, fire, tx, ak, pool)
    want = int((fire != 0).sum())
    assert got["n_frames"] == want and (got["status"] == np.where(fire != 0, X.SENT, X.NOT_FIRED)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. front lengths and alignment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", range(16))
def test_lengths_at_every_alignment(sender, lead):
    """Every front length (one longer than the row's mss among them) at each of the 16 source residues, against this
    frame_lead: the copy's head and tail bytes, and the odd-address byte swap of the sum."""
    lens, res = [], []
    for r in range(16):
        for l in LENS + [33, 1461]:
            lens.append(l), res.append(r)
    flows, src, tx, ak, pool = table(lens, residues=res, seed=40 + lead)
    tx["mss"][np.asarray(lens) == 33] = 8       # sent whole: no repacketization
    tx["mss"][np.asarray(lens) == 1461] = 1460
    fire = mask("kinds", len(lens))
    got, _ = check(sender, src, fire, tx, ak, pool, slot_stride=1531 + lead, frame_lead=lead)
    assert (got["status"] == X.SENT).all()


def test_largest_entry_in_a_slot_that_just_fits(sender):
    """65,481 bytes: 54 + len is the largest a 16-bit frame length holds; the slot is frame_lead + 54 + len."""
    lens = [65481, 7, 65481]
    flows, src, tx, ak, pool = table(lens, residues=[5, 0, 9])
    fire = np.array([X.FIRE_TIMEOUT, X.FIRE_FAST, X.FIRE_FAST], np.uint8)
    got, _ = check(sender, src, fire, tx, ak, pool, slot_stride=3 + 54 + 65481, frame_lead=3, max_frames=3)
    assert (got["status"] == X.SENT).all() and got["len_out"].tolist() == [65535, 61, 65535]
    got, _ = check(sender, src, fire, tx, ak, pool, slot_stride=3 + 54 + 65480, frame_lead=3, max_frames=3)
    assert got["status"].tolist() == [X.E_SLOT, X.SENT, X.E_SLOT] and got["frame"].tolist() == [X.NO_FRAME, 0, X.NO_FRAME]
    pool["len"][0 * CAP + 1] = 65482  # beyond a frame length, whatever the slot
    src = np.concatenate([src, np.zeros(8, np.uint8)])
    got, _ = check(sender, src, fire, tx, ak, pool, slot_stride=70000, max_frames=3)
    assert got["status"].tolist() == [X.E_SLOT, X.SENT, X.SENT]


# ---------------------------------------------------------------------------------------------------------------------
# 3. sequence wrap, header sources
# ---------------------------------------------------------------------------------------------------------------------
def test_sequence_wrap(sender):
    lens = [1, 16, 17, 96, 0]
    flows, src, tx, ak, pool = table(lens)
    tx["snd_una"] = 0xFFFFFFF0
    got, _ = check(sender, src, mask("kinds", 5), tx, ak, pool)
    for f in range(5):
        a = int(got["off_out"][f])
        assert got["out"][a + 38:a + 42].tobytes() == bytes([0xFF, 0xFF, 0xFF, 0xF0])


@pytest.mark.parametrize("offload", [False, True])
@pytest.mark.parametrize("with_rx", [False, True])
def test_header_sources(sender, with_rx, offload):
    n = 65
    lens = [LENS[c % 7] for c in range(n)]
    flows, src, tx, ak, pool = table(lens, seed=9)
    rng = np.random.default_rng(10)
    rx = None
    if with_rx:
        rx = conn_table(n, receive_next=rng.integers(0, 1 << 32, n, dtype=np.uint64), buffer_size=60000)
        rx["reader_next"] = rx["receive_next"] - rng.integers(0, 50000, n).astype(np.uint32)
        tx["rcv_wscale"] = rng.integers(0, 4, n)
    got, _ = check(sender, src, mask("all", n), tx, ak, pool, rx_conns=rx, flags=N.DK_TX_OFFLOAD_TCP if offload else 0)
    assert (got["status"] == X.SENT).all()
    a = got["off_out"].astype(np.int64)
    csum = got["out"][a + 50].astype(int) << 8 | got["out"][a + 51]
    assert not csum.any() if offload else csum.any()
    if with_rx:
        ack = np.stack([got["out"][a + 42 + k] for k in range(4)], 1).astype(np.uint32)
        assert np.array_equal(ack[:, 0] << 24 | ack[:, 1] << 16 | ack[:, 2] << 8 | ack[:, 3], rx["receive_next"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. every status once
# ---------------------------------------------------------------------------------------------------------------------
def test_every_status_leaves_its_connection_alone(sender):
    n = 12
    lens = [10] * n
    flows, src, tx, ak, pool = table(lens)
    rx = conn_table(n, receive_next=77, buffer_size=1000)
    fire = np.full(n, X.FIRE_TIMEOUT, np.uint8)
    fire[0], fire[1], fire[11] = 0, 3, X.FIRE_FAST
    tx["state"][2] = N.DK_TCP_CLOSED
    ak["q_first"][3] = n * CAP - 1               # q_first + q_count beyond the pool
    pool["off"][4 * CAP + 1] = len(src) - 9      # the front ends one byte beyond src
    pool["len"][5 * CAP + 1] = 11                # 54 + 11 > 64
    tx["link"][6] = len(LINKS)
    rx["buffer_size"][7] = 1 << 20               # a window of 20 bits
    ak["q_count"][8] = 0
    ak["rtx_armed"][9] = 0                       # a None deadline cannot time out
    ak["rtx_armed"][11] = 0                      # FAST does not ask the timer
    want = [X.NOT_FIRED, X.E_FIRE, X.E_STATE, X.E_QUEUE, X.E_RANGE, X.E_SLOT, X.E_LINK, X.E_WINDOW, X.IDLE, X.IDLE,
            X.SENT, X.SENT]
    got, _ = check(sender, src, fire, tx, ak, pool, slot_stride=64, rx_conns=rx)
    assert got["status"].tolist() == want and got["n_frames"] == 2
    assert got["frame"].tolist() == [X.NO_FRAME] * 10 + [0, 1]
    for c in range(10):  # its rows and its pool entries as they were; `out` holds the two frames and the canary
        assert got["ack_conns"][c].tobytes() == ak[c].tobytes(), c
        for k in pool:
            assert np.array_equal(got["pool"][k][c * CAP:(c + 1) * CAP], pool[k][c * CAP:(c + 1) * CAP]), (c, k)
    assert (got["out"][2 * 64:] == CANARY).all()
    assert got["ack_conns"]["rtx_armed"].tolist() == [1] * 9 + [0, 1, 0]
    # one kind of failure for the whole table: nothing at all is written
    tx["state"] = N.DK_TCP_NONE
    got, _ = check(sender, src, mask("kinds", n), tx, ak, pool, slot_stride=64, rx_conns=rx)
    assert (got["status"] == X.E_STATE).all() and got["n_frames"] == 0 and (got["out"] == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the back-off, as bits
# ---------------------------------------------------------------------------------------------------------------------
def test_rto_doubling_bits(sender):
    rtos = [0.1, 1.0, 29.999999999999996, 30.0, 45.0, 60.0]
    n = 2 * len(rtos)
    flows, src, tx, ak, pool = table([4] * n)
    ak["rto"] = rtos + rtos
    fire = np.array([X.FIRE_TIMEOUT] * len(rtos) + [X.FIRE_FAST] * len(rtos), np.uint8)
    now = (1 << 62) + 12345
    got, _ = check(sender, src, fire, tx, ak, pool, now)
    want = np.array([0.2, 2.0, 2 * 29.999999999999996, 60.0, 60.0, 60.0] + rtos)
    assert got["ack_conns"]["rto"].tobytes() == want.tobytes()
    assert (got["ack_conns"]["rtx_base_ns"][:len(rtos)] == now).all()
    assert np.array_equal(got["ack_conns"]["rtx_base_ns"][len(rtos):], ak["rtx_base_ns"][len(rtos):])


# ---------------------------------------------------------------------------------------------------------------------
# 6. capacity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["max_frames", "out_bytes"])
def test_no_room_does_nothing(sender, short):
    n = 1025
    lens = [LENS[c % 6] for c in range(n)]
    flows, src, tx, ak, pool = table(lens, seed=77)
    fire = mask("kinds", n)
    fire[[3, 500]] = 0
    ak["q_count"][7] = 0  # IDLE stays IDLE
    need = n - 3
    kw = dict(max_frames=need - 1) if short == "max_frames" else dict(max_frames=need, out_bytes=need * 160 - 1)
    got, _ = check(sender, src, fire, tx, ak, pool, slot_stride=160, out_size=need * 160 + 64, **kw)
    assert got["n_frames"] == need and got["frames_written"] == 0 and (got["frame"] == X.NO_FRAME).all()
    assert (got["out"] == CANARY).all() and got["ack_conns"].tobytes() == ak.tobytes()
    assert all(np.array_equal(got["pool"][k], pool[k]) for k in pool)
    st = np.full(n, X.NO_ROOM)
    st[[3, 500]], st[7] = X.NOT_FIRED, X.IDLE
    assert np.array_equal(got["status"], st)
    # with the room it asks for, the same call goes through
    got, _ = check(sender, src, fire, tx, ak, pool, slot_stride=160, max_frames=need, out_size=need * 160 + 64,
                   out_bytes=need * 160)
    assert got["frames_written"] == need


def test_empty_calls_and_argument_errors(sender):
    import torch

    flows, src, tx, ak, pool = table([5, 6])
    got, _ = check(sender, src, np.zeros(2, np.uint8), tx, ak, pool, frame_conn=False)
    assert got["n_frames"] == 0 and (got["out"] == CANARY).all()
    got, _ = check(sender, src, np.zeros(0, np.uint8), tx[:0], ak[:0], pool, max_frames=0, out_size=64)
    assert got["n_frames"] == 0
    dev = torch.device("cuda", 0)
    d_tx, d_ak = sender.conns_to_device(tx), TcpAcker.conns_to_device(ak)
    d_links = torch.from_numpy(np.ascontiguousarray(LINKS).view(np.uint8).copy()).to(dev)
    d_src, d_out = torch.from_numpy(src).to(dev), torch.zeros(4096, dtype=torch.uint8, device=dev)
    queue = UnackedQueue.from_numpy(pool["off"], pool["len"], pool["tx_time"])
    res, fire = RtxResults(2, 2), fire_to_device(np.ones(2, np.uint8))
    odd = torch.zeros(d_ak.numel() + 16, dtype=torch.uint8, device=dev)[8:8 + d_ak.numel()]
    for kw, args in ((dict(), (d_tx, odd)), (dict(src_bytes=MAX_BLOB + 1), (d_tx, d_ak)),
                     (dict(out_bytes=MAX_BLOB + 1), (d_tx, d_ak))):
        with pytest.raises(Fail) as e:
            retransmit(sender, d_src, fire, *args, queue, 1, d_links, d_out, res, slot_stride=1536, **kw)
        assert e.value.errno == errno.EINVAL
    with pytest.raises(Fail) as e:
        retransmit(sender, d_src, fire, d_tx, d_ak, queue, 1, d_links[:0], d_out, res, slot_stride=1536)
    assert e.value.errno == errno.EINVAL
    torch.cuda.synchronize()
    assert TcpAcker.conns_to_host(d_ak).tobytes() == ak.tobytes() and not d_out.any()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the frames through the receive path
# ---------------------------------------------------------------------------------------------------------------------
def test_loopback_through_receive(sender):
    """The emitted batch through dk_rx_process with every checksum verified: each frame is accepted as TCP and demuxed
    to the flow of the connection it belongs to, with the sequence number and payload of the queue's front."""
    import torch

    n = 300
    lens = [LENS[c % 7] for c in range(n)]
    flows, src, tx, ak, pool = table(lens, seed=5)
    fire = mask("kinds", n)
    fire[::7] = 0
    dev = torch.device("cuda", 0)
    d_links = torch.from_numpy(np.ascontiguousarray(LINKS).view(np.uint8).copy()).to(dev)
    d_out = torch.zeros(n * 1536, dtype=torch.uint8, device=dev)
    d_tx, d_ak = sender.conns_to_device(tx), TcpAcker.conns_to_device(ak)
    queue = UnackedQueue.from_numpy(pool["off"], pool["len"], pool["tx_time"])
    res = RtxResults(n, n)
    batch = retransmit_batch(sender, torch.from_numpy(src).to(dev), fire_to_device(fire), d_tx, d_ak, queue, 99,
                             d_links, d_out, res, slot_stride=1536)
    conns = np.nonzero(fire)[0]
    assert batch.n == len(conns)
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    try:
        eng.set_sockets(flows)
        r = eng.results(batch.n, tcp_fields=True)
        eng.receive_batch(batch, r)
        torch.cuda.synchronize()
        h = r.to_numpy()
    finally:
        eng.close()
    assert ((h["meta"] & 0xFF) == N.V["OK_TCP"]).all()
    assert np.array_equal(h["flow_id"], conns) and np.array_equal(res.to_numpy()["frame_conn"], conns)
    assert np.array_equal(h["tcp_seq"], tx["snd_una"][conns])
    want_len = np.asarray(lens)[conns]
    assert np.array_equal(h["payload"], 54 | want_len.astype(np.uint32) << 16)
    fin = (h["meta"] >> 16) & 0x01
    assert np.array_equal(fin != 0, want_len == 0)
