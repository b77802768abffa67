"""dk_tcp_ack_timer on the MI355X against tests/tcp_ackemit_reference.py (pinned on the CPU by
tests/test_tcp_ackemit_model.py). Every call is compared whole: the output blob over a canary fill, every result array
over a canary fill, the dack table as bytes, and the receive and TX tables unchanged."""
import errno

import numpy as np
import pytest

import tcp_ackemit_reference as E
import tx_segment_reference as M
from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd.rx import Fail
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_ackemit import AckEmitResults, ack_timer, ack_timer_batch, dack_conn_table, dack_to_device, dack_to_host
from demikernel_amd.tcp_rtx import fire_to_device
from demikernel_amd.tcp_tx import TcpSender

pytestmark = pytest.mark.gpu

CANARY, FILL = 0xA5, 0x5A5A5A5A
LINKS = M.links_table()
SIZES = [1, 63, 64, 65, 1024, 1025, 2049]  # the scan tile is 1,024 items: the last two cross it, 2,049 takes a third
MASKS = ["none", "all", "second", "last"]


@pytest.fixture(scope="module")
def sender():
    s = TcpSender(0)
    yield s
    s.close()


def table(n: int, seed: int = 3):
    """n connections: every third disarmed, unread bytes and window scales of 0 to 14 at random, every fifth RCV.NXT at
    0xFFFFFFFE."""
    rng = np.random.default_rng(seed)
    flows = synth.make_flows(n, passive=False)
    snd = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    tx = M.conns_toward(flows, seed=seed, snd_nxt=snd)  # the far ends of a receiving peer's flows: the ACKs go to it
    tx["rcv_wscale"] = rng.integers(0, 15, n)
    rn = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    rn[::5] = 0xFFFFFFFE
    rx = conn_table(n, receive_next=rn, send_next=snd)
    rx["buffer_size"] = (rng.integers(1, 0x10000, n) << tx["rcv_wscale"]).astype(np.uint32)
    rx["reader_next"] = rx["receive_next"] - (rng.random(n) * rx["buffer_size"]).astype(np.uint32)
    dack = dack_conn_table(n, delay_ns=rng.integers(1, 1 << 40, n, dtype=np.uint64), armed=(np.arange(n) % 3 != 1),
                           deadline_ns=rng.integers(1, 1 << 50, n, dtype=np.uint64))
    return tx, rx, dack, flows


def mask(kind: str, n: int) -> np.ndarray:
    c = np.arange(n)
    return {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "second": (c % 2 * 7).astype(np.uint8),
            "last": (c == n - 1).astype(np.uint8)}[kind]


def check(sender, fire, tx, rx, dack, *, slot_stride=64, frame_lead=0, max_frames=None, out_size=None, flags=0,
          out_bytes=None, links=LINKS):
    import torch

    n = len(fire)
    max_frames = n + 2 if max_frames is None else max_frames
    out_size = max(max_frames, 1) * slot_stride + 64 if out_size is None else out_size
    exp = E.ack_timer(fire, tx, rx, dack, links, np.full(out_size, CANARY, np.uint8), slot_stride=slot_stride,
                      frame_lead=frame_lead, max_frames=max_frames, flags=flags, out_bytes=out_bytes)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    d_tx, d_rx, d_dack, d_links = up(tx), up(rx), dack_to_device(dack), up(links)
    d_out = torch.full((out_size,), CANARY, dtype=torch.uint8, device=dev)
    res = AckEmitResults(max_frames, n, fill=FILL)
    ack_timer(sender, fire_to_device(fire), d_tx, d_rx, d_dack, d_links, d_out, res, slot_stride=slot_stride,
              frame_lead=frame_lead, max_frames=max_frames, flags=flags, out_bytes=out_bytes)
    torch.cuda.synchronize()
    got = res.to_numpy()
    w = got["frames_written"]
    assert (res.off_out.cpu().numpy().view(np.uint32)[w:] == FILL).all()
    assert (res.frame_conn.cpu().numpy().view(np.uint32)[w:] == FILL).all()
    assert (res.frame_seg.cpu().numpy().view(np.uint32) == FILL).all(), "frame_seg is not this call's"
    assert got["n_frames"] == exp["n_frames"]
    for k in ("status", "n_acks", "ack_frame", "off_out", "len_out", "frame_conn"):
        g, e = got[k], exp[k]
        assert len(g) == len(e), (k, len(g), len(e))
        assert np.array_equal(g, e), (k, np.nonzero(g != e)[0][:8], g[g != e][:8], e[g != e][:8])
    assert dack_to_host(d_dack).tobytes() == exp["dack"].tobytes()
    out = d_out.cpu().numpy()
    if not np.array_equal(out, exp["out"]):
        bad = np.nonzero(out != exp["out"])[0]
        raise AssertionError(f"{len(bad)} output bytes differ, first at {bad[:8]}: got {out[bad[:8]]} expected "
                             f"{exp['out'][bad[:8]]}")
    assert d_tx.cpu().numpy().tobytes() == tx.tobytes() and d_rx.cpu().numpy().tobytes() == rx.tobytes()
    got.update(out=out, dack=exp["dack"])
    return got, exp


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_masks(sender, n, kind):
    tx, rx, dack, _ = table(n, seed=n)
    fire = mask(kind, n)
    got, exp = check(sender, fire, tx, rx, dack)
    armed = dack["armed"] != 0
    assert got["n_frames"] == int(((fire != 0) & armed).sum())
    assert np.array_equal(got["status"], np.where(fire == 0, E.NOT_FIRED, np.where(armed, E.OK, E.IDLE)))
    assert np.array_equal(got["dack"]["armed"], np.where(fire != 0, 0, dack["armed"]))
    assert np.array_equal(got["dack"]["deadline_ns"], dack["deadline_ns"])
    # ack number and sequence number of every frame, from the tables as they stand
    a, c = got["off_out"].astype(np.int64), got["frame_conn"]
    be32 = lambda o: sum(got["out"][a + o + k].astype(np.uint32) << (24 - 8 * k) for k in range(4))  # noqa: E731
    assert np.array_equal(be32(42), rx["receive_next"][c]) and np.array_equal(be32(38), tx["snd_nxt"][c])


def test_every_status(sender):
    n = 12
    tx, rx, dack, _ = table(n)
    dack["armed"] = 1
    fire = np.ones(n, np.uint8)
    fire[0] = 0
    tx["state"][1] = N.DK_TCP_CLOSED
    rx["send_next"][2] += 1
    tx["link"][3] = len(LINKS)
    tx["rcv_wscale"][4] = 15
    tx["rcv_wscale"][5], rx["buffer_size"][5] = 3, 0x10000 << 3
    dack["armed"][6] = 0
    tx["state"][7], dack["armed"][7] = N.DK_TCP_NONE, 0      # the connection's checks before IDLE
    rx["send_next"][8], tx["link"][8] = rx["send_next"][8] + 5, 9  # E_SND_NXT before E_LINK
    want = [E.NOT_FIRED, E.E_STATE, E.E_SND_NXT, E.E_LINK, E.E_WSCALE, E.E_WINDOW, E.IDLE, E.E_STATE, E.E_SND_NXT,
            E.OK, E.OK, E.OK]
    got, _ = check(sender, fire, tx, rx, dack)
    assert got["status"].tolist() == want and got["ack_frame"].tolist() == [E.NO_FRAME] * 9 + [0, 1, 2]
    got, _ = check(sender, fire, tx, rx, dack, slot_stride=57, frame_lead=4)
    slot = [E.E_SLOT if s in (E.OK, E.IDLE) else s for s in want]  # the slot check is the connection's: before IDLE
    assert got["status"].tolist() == slot and got["n_frames"] == 0 and (got["out"] == CANARY).all()


@pytest.mark.parametrize("short", ["max_frames", "zero", "out_bytes"])
def test_no_room_does_nothing(sender, short):
    n = 1025
    tx, rx, dack, _ = table(n, seed=77)
    fire = mask("all", n)
    fire[[3, 500]] = 0
    need = int(((fire != 0) & (dack["armed"] != 0)).sum())
    kw = {"max_frames": dict(max_frames=need - 1), "zero": dict(max_frames=0),
          "out_bytes": dict(max_frames=need, out_bytes=need * 70 - 1)}[short]
    got, _ = check(sender, fire, tx, rx, dack, slot_stride=70, out_size=need * 70 + 64, **kw)
    assert got["n_frames"] == need and got["frames_written"] == 0 and (got["ack_frame"] == E.NO_FRAME).all()
    assert (got["out"] == CANARY).all() and got["dack"].tobytes() == dack.tobytes()
    assert np.array_equal(got["status"] == E.NO_ROOM, (fire != 0) & (dack["armed"] != 0))
    got, _ = check(sender, fire, tx, rx, dack, slot_stride=70, max_frames=need, out_size=need * 70 + 64,
                   out_bytes=need * 70)
    assert got["frames_written"] == need


@pytest.mark.parametrize("stride,lead", [(54, 0), (55, 1), (61, 7), (131, 3)])
@pytest.mark.parametrize("offload", [False, True])
def test_unaligned_slots_and_offload(sender, stride, lead, offload):
    tx, rx, dack, _ = table(130, seed=stride)
    got, _ = check(sender, mask("all", 130), tx, rx, dack, slot_stride=stride, frame_lead=lead,
                   flags=N.DK_TX_OFFLOAD_TCP if offload else 0)
    a = got["off_out"].astype(np.int64)
    csum = got["out"][a + 50].astype(int) << 8 | got["out"][a + 51]
    assert not csum.any() if offload else csum.any()


def test_empty_calls_and_argument_errors(sender):
    import torch

    tx, rx, dack, _ = table(2)
    got, _ = check(sender, np.zeros(0, np.uint8), tx[:0], rx[:0], dack[:0], max_frames=0, out_size=64)
    assert got["n_frames"] == 0
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    d_tx, d_rx, d_dack, d_links = up(tx), up(rx), dack_to_device(dack), up(LINKS)
    d_out = torch.zeros(4096, dtype=torch.uint8, device=dev)
    res, fire = AckEmitResults(2, 2), fire_to_device(np.ones(2, np.uint8))
    odd = torch.zeros(d_dack.numel() + 16, dtype=torch.uint8, device=dev)[8:8 + d_dack.numel()]
    for args, kw in (((d_tx, d_rx, odd, d_links), {}), ((d_tx, d_rx, d_dack, d_links), dict(out_bytes=0xFFFFFF01)),
                     ((d_tx, d_rx, d_dack, d_links[:0]), {})):
        with pytest.raises(Fail) as e:
            ack_timer(sender, fire, *args, d_out, res, slot_stride=64, **kw)
        assert e.value.errno == errno.EINVAL
    torch.cuda.synchronize()
    assert dack_to_host(d_dack).tobytes() == dack.tobytes() and not d_out.any()


def test_loopback_through_receive(sender):
    """The emitted batch through dk_rx_process with every checksum verified: each frame is accepted as TCP and demuxed
    to the flow of the connection it belongs to at the other end."""
    import torch

    from demikernel_amd import Config, RxEngine

    n = 300
    tx, rx, dack, flows = table(n, seed=5)
    fire = mask("second", n)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    res = AckEmitResults(n, n)
    batch = ack_timer_batch(sender, fire_to_device(fire), up(tx), up(rx), dack_to_device(dack), up(LINKS), d_out, res,
                            slot_stride=64)
    conns = np.nonzero((fire != 0) & (dack["armed"] != 0))[0]
    assert batch.n == len(conns) > 0
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    try:
        eng.set_sockets(flows)
        r = eng.results(batch.n, tcp_fields=True)
        eng.receive_batch(batch, r)
        torch.cuda.synchronize()
        h = r.to_numpy()
    finally:
        eng.close()
    assert ((h["meta"] & 0xFF) == N.V["OK_TCP"]).all(), np.bincount(h["meta"] & 0xFF)
    assert np.array_equal(h["flow_id"], conns) and np.array_equal(res.to_numpy()["frame_conn"], conns)
    assert np.array_equal(h["tcp_seq"], tx["snd_nxt"][conns]) and np.array_equal(h["tcp_ack"], rx["receive_next"][conns])
    assert ((h["meta"] >> 16) & 0xFF == 0x10).all() and np.array_equal(h["payload"], np.full(len(conns), 54, np.uint32))
