"""dk_tcp_tx_segment on the MI355X against tests/tx_segment_reference.py (the send_segment loop, pinned on the CPU by
tests/test_tcp_tx_segment_model.py). Every test compares the whole output blob (a canary fill proves nothing outside the
frames is written), every result array and the whole connection table with the model, byte for byte, and checks the
source unchanged."""
import numpy as np
import pytest

import tx_segment_reference as M
from ctl_calls import delayed, stream_pair
from demikernel_amd import Config, RxEngine, synth
from demikernel_amd import _native as N
from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table
from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults, frame_bound, tcp_tx_grid

pytestmark = pytest.mark.gpu

CANARY = 0xA5
LINKS = M.links_table()


@pytest.fixture(scope="module")
def sender():
    s = TcpSender(0)
    yield s
    s.close()


def flows_for(nconns):
    return synth.make_flows(nconns, passive=False)


def run_gpu(sender, src, conn, off, ln, tx, *, slot_stride, frame_lead, max_frames, out_size, out_bytes=None,
            rx_conns=None, flags=0, stream=None, src_bytes=None, links=LINKS, state=None):
    """One call on fresh device arrays (or on `state`, the device arrays a previous call of the test left)."""
    import torch

    dev = torch.device("cuda", 0)
    if state is None:
        state = dict(
            src=torch.from_numpy(np.array(src, np.uint8, copy=True)).to(dev),
            out=torch.full((out_size,), CANARY, dtype=torch.uint8, device=dev),
            tx=sender.conns_to_device(tx),
            links=torch.from_numpy(np.ascontiguousarray(links, N.TX_LINK_DTYPE).view(np.uint8).copy()).to(dev),
            rx=None if rx_conns is None or hasattr(rx_conns, "data_ptr") else
            torch.from_numpy(np.ascontiguousarray(rx_conns).view(np.uint8).copy()).to(dev))
        if hasattr(rx_conns, "data_ptr"):
            state["rx"] = rx_conns
    push = PushList.from_numpy(conn, off, ln)
    res = TcpTxResults(max_frames, len(conn))
    torch.cuda.synchronize()
    sender.segment(state["src"], push, state["tx"], state["links"], state["out"], res, slot_stride=slot_stride,
                   frame_lead=frame_lead, rx_conns=state["rx"], offload_tcp=bool(flags & N.DK_TX_OFFLOAD_TCP),
                   stream=stream, src_bytes=src_bytes, out_bytes=out_bytes, max_frames=max_frames)
    (stream if stream is not None else torch.cuda.current_stream(0)).synchronize()
    got = res.to_numpy()
    got["out"] = state["out"].cpu().numpy()
    got["tx_conns"] = sender.conns_to_host(state["tx"])
    got["src"] = state["src"].cpu().numpy()
    # entries of the per-frame arrays past the frames written are untouched (zero-initialised)
    w = got["frames_written"]
    assert not res.off_out.cpu().numpy()[w:].any() and not res.len_out.cpu().numpy()[w:].any()
    got["state"] = state
    return got


def assert_same(got, exp, src):
    assert got["n_frames"] == exp["n_frames"]
    for k in ("status", "sent", "first_frame", "frame_count", "off_out", "len_out", "frame_buf"):
        g, e = got[k], exp[k]
        assert len(g) == len(e), (k, len(g), len(e))
        assert np.array_equal(g, e), (k, np.nonzero(g != e)[0][:8], g[g != e][:8], e[g != e][:8])
    gt, et = got["tx_conns"], exp["tx_conns"]
    assert gt.tobytes() == et.tobytes(), [(c, k) for c in range(len(gt)) for k in gt.dtype.names if gt[k][c] != et[k][c]][:8]
    if not np.array_equal(got["out"], exp["out"]):
        bad = np.nonzero(got["out"] != exp["out"])[0]
        raise AssertionError(f"{len(bad)} output bytes differ, first at {bad[:8]}: got {got['out'][bad[:8]]} "
                             f"expected {exp['out'][bad[:8]]}")
    assert np.array_equal(got["src"], src), "the source blob was written"


def check(sender, src, conn, off, ln, tx, *, slot_stride=1536, frame_lead=0, max_frames=None, out_size=None, **kw):
    if max_frames is None:
        max_frames = max(frame_bound(ln, max(int(tx["mss"].min()), 1)), 1) + 3
    if out_size is None:
        out_size = max_frames * slot_stride + 64
    rx = kw.get("rx_conns")
    exp = M.segment(src, conn, off, ln, tx, kw.get("links", LINKS), np.full(out_size, CANARY, np.uint8),
                    slot_stride=slot_stride, frame_lead=frame_lead, max_frames=max_frames, rx_conns=rx,
                    flags=kw.get("flags", 0), src_bytes=kw.get("src_bytes"), out_bytes=kw.get("out_bytes"))
    got = run_gpu(sender, src, conn, off, ln, tx, slot_stride=slot_stride, frame_lead=frame_lead, max_frames=max_frames,
                  out_size=out_size, **kw)
    assert_same(got, exp, src)
    return got, exp


# ---------------------------------------------------------------------------------------------------------------------
# 1. cut positions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mss", [1, 2, 15, 16, 17, 536, 1460, 1461])
def test_cut_positions(sender, mss):
    """One connection; buffers of 1, mss - 1, mss, mss + 1, 2 mss, 3 mss + 7 bytes at every source residue mod 16, the
    marker last."""
    sizes = [s for s in (1, mss - 1, mss, mss + 1, 2 * mss, 3 * mss + 7) if s > 0]
    lens, res = [], []
    for r in range(16):
        for k, s in enumerate(sizes):
            lens.append(sizes[(k + r) % len(sizes)])
            res.append((r + 3 * k) % 16)
    for k, s in enumerate(sizes):  # every size at every residue: the rotation above covers 16 of the 96 pairs each
        for r in range(16):
            lens.append(s)
            res.append(r)
    lens.append(0)
    res.append(0)
    src, conn, off, ln = M.pack_push(np.zeros(len(lens)), lens, residues=res)
    tx = M.conns_toward(flows_for(1), mss=mss)
    got, exp = check(sender, src, conn, off, ln, tx)
    assert (exp["status"] == M.SENT).all() and exp["tx_conns"]["fin_sent"][0] == 1
    assert exp["n_frames"] == frame_bound(ln, mss)


# ---------------------------------------------------------------------------------------------------------------------
# 2. budget edges
# ---------------------------------------------------------------------------------------------------------------------
def test_budget_edges(sender):
    """B - C at a buffer's start in {0, 1, mss - 1, mss, mss + 1, len, len + 1}; a marker at B - C = 0 and 1; closed
    windows; cwnd as the binding limit; mss 0; sequence numbers wrapping inside the call."""
    mss, first, length = 100, 130, 250
    conn, lens, wnd, cwnd, una_back, mssv = [], [], [], [], [], []

    def add(bufs, w, cw=0xFFFFFFFF, inflight=0, m=mss):
        c = len(wnd)
        conn.extend([c] * len(bufs))
        lens.extend(bufs)
        wnd.append(w)
        cwnd.append(cw)
        una_back.append(inflight)
        mssv.append(m)

    for e in (0, 1, mss - 1, mss, mss + 1, length, length + 1):
        add([first, length, 7], first + e)
        add([first, length, 7], 1 << 20, cw=first + e + 40, inflight=40)  # the same edge with cwnd binding, 40 in flight
    add([first, 0, 5], first)        # marker at B - C = 0: not sent
    add([first, 0, 5], first + 1)    # at 1: FIN
    add([first, 0], 1 << 20)
    add([50, 0], 0)                  # snd_wnd = 0
    add([50, 0], 30, inflight=31)    # snd_wnd < in flight
    add([50, 0], 1 << 20, cw=30, inflight=31)  # cwnd < in flight
    add([50, 0], 1 << 20, m=0)       # mss 0 never opens the window
    add([0], 1 << 20)                # a lone marker
    n = len(wnd)
    tx = M.conns_toward(flows_for(n), snd_nxt=0xFFFFFF00, snd_wnd=wnd, cwnd=cwnd, mss=mssv)
    tx["snd_una"] = tx["snd_nxt"] - np.asarray(una_back, np.uint32)
    src, c, off, ln = M.pack_push(conn, lens, residues=np.arange(len(lens)) * 7 % 16)
    got, exp = check(sender, src, c, off, ln, tx, slot_stride=160, frame_lead=1, max_frames=len(lens) * 4)
    st = exp["status"]
    assert {M.SENT, M.PARTIAL, M.UNSENT, M.CLOSED} <= set(st.tolist())
    assert (exp["tx_conns"]["snd_nxt"] < 0x1000).any()  # SND.NXT wrapped


# ---------------------------------------------------------------------------------------------------------------------
# 3. shapes of the scans
# ---------------------------------------------------------------------------------------------------------------------
def _random_push(nconns, nbufs, rng, sizes):
    conn = np.sort(rng.integers(0, nconns, nbufs)) if nconns > 1 else np.zeros(nbufs, np.int64)
    if nconns > 4:  # empty connections between busy ones, and one with many buffers
        conn[conn % 3 == 1] += 1
        conn = np.sort(np.minimum(conn, nconns - 1))
    lens = rng.choice(sizes, nbufs)
    lens[rng.random(nbufs) < 0.02] = 0  # a few end-of-send markers: the buffers behind them are closed
    return conn, lens


@pytest.mark.parametrize("nconns,nbufs,grid", [(1, 1, -1), (2, 9, -1), (65, 400, -1), (300, 2500, 3), (1, 65, -1),
                                               (1, 1100, 2), (300, 5000, -1)])
def test_scan_shapes(sender, nconns, nbufs, grid):
    """Connections with 0, 1 or many buffers; push lists past a wave and past a workgroup of the scans; a few thousand
    frames; the emit grid capped so every wave takes several chunks."""
    rng = np.random.default_rng(nconns * 7 + nbufs)
    conn, lens = _random_push(nconns, nbufs, rng, [1, 3, 16, 31, 32, 33, 64, 70])
    tx = M.conns_toward(flows_for(nconns), mss=32, snd_wnd=rng.choice([0, 40, 300, 1 << 20, 1 << 20, 1 << 20], nconns))
    src, c, off, ln = M.pack_push(conn, lens)
    tcp_tx_grid(grid)
    try:
        got, exp = check(sender, src, c, off, ln, tx, slot_stride=96, frame_lead=5)
    finally:
        tcp_tx_grid(-1)
    if nbufs == 5000:
        assert exp["n_frames"] > 2000


@pytest.mark.parametrize("frames", [1, 2, 62, 63, 64, 65])
def test_frame_totals(sender, frames):
    """Frame totals around the emit kernel's 64-frame chunk, and last chunks that end inside a group of four frames
    (the quarter-waves of the copy)."""
    tx = M.conns_toward(flows_for(2), mss=8)
    src, c, off, ln = M.pack_push([0, 1][:min(frames, 2)], [8 * (frames - 1), 3][-min(frames, 2):])
    got, exp = check(sender, src, c, off, ln, tx, slot_stride=64, frame_lead=0, max_frames=80)
    assert exp["n_frames"] == frames


# ---------------------------------------------------------------------------------------------------------------------
# 4. layouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,lead,mss", [(1536, 0, 1460), (2048, 82, 1460), (591, 0, 537), (592, 1, 537)])
def test_layouts(sender, stride, lead, mss):
    """The ring's layout (frames at 2 mod 16), the tightest stride with an odd mss (frames at odd addresses), an odd
    lead."""
    rng = np.random.default_rng(stride)
    lens = [3 * mss + 11, 1, mss, 2 * mss - 1, 0, 700, mss + 1]
    src, c, off, ln = M.pack_push([0, 0, 0, 0, 0, 1, 1], lens, residues=rng.integers(0, 16, len(lens)))
    tx = M.conns_toward(flows_for(2), mss=mss)
    check(sender, src, c, off, ln, tx, slot_stride=stride, frame_lead=lead)


def test_stride_one_byte_short_fails_only_that_connection(sender):
    tx = M.conns_toward(flows_for(3), mss=[537, 538, 537])
    src, c, off, ln = M.pack_push([0, 1, 1, 2], [1000, 1000, 0, 1000])
    got, exp = check(sender, src, c, off, ln, tx, slot_stride=591, frame_lead=0)
    assert list(exp["status"]) == [M.SENT, M.E_CONN, M.E_CONN, M.SENT] and exp["n_frames"] == 4


# ---------------------------------------------------------------------------------------------------------------------
# 5. failures interleaved with good connections
# ---------------------------------------------------------------------------------------------------------------------
def test_failures_interleaved(sender):
    n = 12
    tx = M.conns_toward(flows_for(n), mss=200, rcv_wscale=0)
    rx = conn_table(n, receive_next=np.arange(n) * 1000 + 5, buffer_size=65535)
    tx["state"][1] = N.DK_TCP_CLOSED
    tx["state"][2] = N.DK_TCP_NONE
    tx["link"][3] = 2                 # link out of range
    rx["buffer_size"][4] = 1 << 20    # window overflow (wscale 0)
    tx["fin_sent"][6] = 1
    tx["mss"][9] = 65496              # no IPv4 total length for it
    conn = [0, 0, 1, 2, 3, 4, 4, 5, 5, 5, 6, 7, 7, 7, 8, 9, 10, 11, 11, 12, 40]
    lens = [300, 0, 50, 50, 50, 50, 0, 10, 0, 10, 77, 450, 0, 0, 33, 10, 90, 64, 0, 5, 5]
    src, c, off, ln = M.pack_push(conn, lens)
    off[14] = len(src) - 10           # connection 8: a range outside src_bytes
    got, exp = check(sender, src, c, off, ln, tx, slot_stride=256, frame_lead=2, rx_conns=rx, max_frames=40)
    st = exp["status"]
    assert list(st[2:7]) == [M.E_CONN] * 5 and st[9] == M.CLOSED and st[10] == M.CLOSED and st[13] == M.CLOSED
    assert st[14] == st[15] == M.E_CONN and st[19] == st[20] == M.E_CONN  # conn index out of range
    assert st[0] == st[7] == st[11] == st[16] == st[17] == M.SENT
    # a range error on one buffer fails every buffer of its connection
    off2 = off.copy()
    off2[13] = len(src)
    got, exp = check(sender, src, c, off2, ln, tx, slot_stride=256, frame_lead=2, rx_conns=rx, max_frames=40,
                     src_bytes=len(src) - 1)
    assert list(exp["status"][11:14]) == [M.E_CONN] * 3


# ---------------------------------------------------------------------------------------------------------------------
# 6. capacity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["frames", "bytes"])
def test_capacity_all_or_nothing(sender, short):
    """One frame short in max_frames or in out_bytes: n_frames reports the need, out and the table are untouched; the
    same call with room then succeeds on the same context and the same device arrays."""
    tx = M.conns_toward(flows_for(3), mss=100, snd_wnd=[1 << 20, 150, 1 << 20])
    src, c, off, ln = M.pack_push([0, 0, 1, 1, 2], [950, 0, 200, 5, 100])
    need = 10 + 1 + 2 + 0 + 1
    stride = 160
    kw = dict(max_frames=need - 1) if short == "frames" else dict(max_frames=need, out_bytes=need * stride - 1)
    got, exp = check(sender, src, c, off, ln, tx, slot_stride=stride, frame_lead=3, out_size=need * stride + 16, **kw)
    assert got["n_frames"] == need and got["frames_written"] == 0
    assert (got["out"] == CANARY).all() and got["tx_conns"].tobytes() == tx.tobytes()
    assert list(got["status"]) == [M.NO_ROOM, M.NO_ROOM, M.NO_ROOM, M.UNSENT, M.NO_ROOM]
    exp2 = M.segment(src, c, off, ln, tx, LINKS, np.full(need * stride + 16, CANARY, np.uint8), slot_stride=stride,
                     frame_lead=3, max_frames=need)
    got2 = run_gpu(sender, src, c, off, ln, tx, slot_stride=stride, frame_lead=3, max_frames=need,
                   out_size=need * stride + 16, state=got["state"])
    assert_same(got2, exp2, src)
    assert got2["frames_written"] == need


# ---------------------------------------------------------------------------------------------------------------------
# 7. offload, receive table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offload", [False, True])
@pytest.mark.parametrize("with_rx", [False, True])
def test_offload_and_receive_table(sender, offload, with_rx):
    n = 4
    tx = M.conns_toward(flows_for(n), mss=536, rcv_wscale=[0, 4, 7, 14])
    rx = None
    if with_rx:
        rx = conn_table(n, receive_next=[7, 0xFFFFFFF0, 100, 5], buffer_size=[65535, 1 << 20, 1 << 22, 1 << 29])
        rx["reader_next"] = rx["receive_next"] - np.asarray([0, 1000, 0, 12345], np.uint32)  # unread bytes
    src, c, off, ln = M.pack_push([0, 0, 1, 2, 2, 3], [1500, 0, 536, 537, 1, 2000], residues=[1, 0, 15, 8, 3, 6])
    got, exp = check(sender, src, c, off, ln, tx, slot_stride=640, frame_lead=2, rx_conns=rx,
                     flags=N.DK_TX_OFFLOAD_TCP if offload else 0)
    if offload:
        assert all(not exp["out"][int(o) + 50:int(o) + 52].any() for o in exp["off_out"])
    if with_rx:
        o = int(exp["off_out"][4])  # connection 1's frame: window (2^20 - 1000) >> 4, ack its RCV.NXT
        assert int.from_bytes(exp["out"][o + 48:o + 50].tobytes(), "big") == ((1 << 20) - 1000) >> 4
        assert int.from_bytes(exp["out"][o + 42:o + 46].tobytes(), "big") == 0xFFFFFFF0


# ---------------------------------------------------------------------------------------------------------------------
# 8. streams
# ---------------------------------------------------------------------------------------------------------------------
def test_other_stream_and_back_to_back(sender):
    """A stream that is not the current one; two calls back to back on one context continue the connections."""
    import torch

    s = torch.cuda.Stream(device=0)
    tx = M.conns_toward(flows_for(2), mss=300, snd_wnd=[1000, 1 << 20])
    src, c, off, ln = M.pack_push([0, 0, 1], [700, 700, 40])
    got, exp = check(sender, src, c, off, ln, tx, slot_stride=384, frame_lead=0, max_frames=12, stream=s)
    assert list(exp["status"]) == [M.SENT, M.PARTIAL, M.SENT]
    # the second call sees the first one's SND.NXT: connection 0's window is now full, connection 1 goes on
    exp2 = M.segment(src, c, off, ln, exp["tx_conns"], LINKS, exp["out"], slot_stride=384, frame_lead=0, max_frames=12)
    got2 = run_gpu(sender, src, c, off, ln, None, slot_stride=384, frame_lead=0, max_frames=12, out_size=0,
                   state=got["state"])
    assert_same(got2, exp2, src)
    assert list(exp2["status"]) == [M.UNSENT, M.UNSENT, M.SENT]
    # two calls queued without a wait between them on two streams, the first behind 100 ms of sleep and still pending
    # when the second has been queued: the context orders them (tests/test_gpu_tcp_ctx_streams.py has the other chains)
    st = got["state"]
    push, r1, r2 = PushList.from_numpy(c, off, ln), TcpTxResults(12, 3), TcpTxResults(12, 3)
    st["tx"].copy_(sender.conns_to_device(tx))
    torch.cuda.synchronize()
    A, B, _ = stream_pair()
    ev = delayed(A)
    sender.segment(st["src"], push, st["tx"], st["links"], st["out"], r1, slot_stride=384, stream=A)
    sender.segment(st["src"], push, st["tx"], st["links"], st["out"], r2, slot_stride=384, stream=B)
    assert not ev.query(), "the delay ended while the calls were being issued: a call waited on the host"
    torch.cuda.synchronize()
    assert np.array_equal(r1.to_numpy()["status"], exp["status"]) and np.array_equal(r2.to_numpy()["status"], exp2["status"])
    assert sender.conns_to_host(st["tx"]).tobytes() == exp2["tx_conns"].tobytes()
    assert np.array_equal(st["out"].cpu().numpy(), exp2["out"])


# ---------------------------------------------------------------------------------------------------------------------
# 9. the loop: push bytes -> frames -> dk_rx_process -> dk_tcp_rx_process -> the pushed bytes
# ---------------------------------------------------------------------------------------------------------------------
def test_loop_through_the_receive_path(sender):
    import torch

    nconns = 6
    flows = flows_for(nconns)
    rng = np.random.default_rng(21)
    conn = np.sort(rng.integers(0, nconns, 60))
    lens = rng.choice([1, 2, 99, 1459, 1460, 1461, 2920, 5000], 60)
    conn, lens = np.concatenate([conn, [2, 4]]), np.concatenate([lens, [0, 0]])  # connections 2 and 4 close
    order = np.argsort(conn, kind="stable")
    conn, lens = conn[order], lens[order]
    src, c, off, ln = M.pack_push(conn, lens, residues=rng.integers(0, 16, len(lens)))
    tx = M.conns_toward(flows, mss=1460)
    cap = frame_bound(ln, 1460)
    dev = torch.device("cuda", 0)
    d_src = torch.from_numpy(src).to(dev)
    d_out = torch.zeros(cap * 1536, dtype=torch.uint8, device=dev)
    d_links = torch.from_numpy(np.ascontiguousarray(LINKS).view(np.uint8).copy()).to(dev)
    d_tx = sender.conns_to_device(tx)
    res = TcpTxResults(cap, len(c))
    batch = sender.segment_batch(d_src, PushList.from_numpy(c, off, ln), d_tx, d_links, d_out, res, slot_stride=1536)
    assert batch.n == cap
    # the peer: every checksum verified (no offload), then its TCP receive side on the same stream
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    eng.set_sockets(flows)
    r = eng.results(batch.n, tcp_fields=True)
    eng.receive_batch(batch, r)
    tcp = TcpReceiver(0)
    table = conn_table(nconns, receive_next=tx["snd_nxt"], send_next=tx["rcv_nxt"], buffer_size=1 << 20)
    d_rx = tcp.conns_to_device(table)
    out = TcpOut(batch.n, nconns)
    tcp.process(r, d_rx, out)
    # the other direction, queued behind it with no host step: its ack number is the RCV.NXT the receive just set
    back_tx = M.conns_toward(flows, seed=8, mss=64, rcv_wscale=5)
    back_tx["local_ip"], back_tx["remote_ip"] = flows["local_ip"], flows["remote_ip"]
    back_tx["ports"] = flows["local_port"].astype(np.uint32) | flows["remote_port"].astype(np.uint32) << 16
    d_btx = sender.conns_to_device(back_tx)
    bsrc, bc, boff, bln = M.pack_push(np.arange(nconns), [10] * nconns)
    d_bout = torch.zeros(nconns * 128, dtype=torch.uint8, device=dev)
    bres = TcpTxResults(nconns, nconns)
    sender.segment(torch.from_numpy(bsrc).to(dev), PushList.from_numpy(bc, boff, bln), d_btx, d_links, d_bout, bres,
                   slot_stride=128, rx_conns=d_rx)
    torch.cuda.synchronize()
    got = r.to_numpy()
    assert ((got["meta"] & 0xFF) == N.V["OK_TCP"]).all()
    h = out.to_numpy()
    assert set(np.unique(h["action"])) <= {N.A["DELIVERED"], N.A["FIN"]}
    frames, foff = d_out.cpu().numpy(), batch.off.cpu().numpy().view(np.uint32)
    new_rx = tcp.conns_to_host(d_rx)
    new_tx = sender.conns_to_host(d_tx)
    for k in range(nconns):
        data = b""
        for v in out.delivered(k, h):
            if v["ref"] != N.DK_TCP_REF_EOF:
                o = int(foff[v["ref"]]) + int(v["off"])
                data += frames[o:o + int(v["len"])].tobytes()
        want = b"".join(src[int(off[b]):int(off[b]) + int(ln[b])].tobytes() for b in np.nonzero(c == k)[0])
        assert data == want, k
        assert new_rx["receive_next"][k] == new_tx["snd_nxt"][k]
    assert list(new_rx["state"]) == [N.DK_TCP_CLOSED if k in (2, 4) else N.DK_TCP_ESTABLISHED for k in range(nconns)]
    bexp = M.segment(bsrc, bc, boff, bln, back_tx, LINKS, np.zeros(nconns * 128, np.uint8), slot_stride=128,
                     frame_lead=0, max_frames=nconns, rx_conns=new_rx)
    assert np.array_equal(d_bout.cpu().numpy(), bexp["out"]) and (bexp["status"] == M.SENT).all()
    assert np.array_equal(bres.to_numpy()["status"], bexp["status"])
    for k in range(nconns):
        assert int.from_bytes(bexp["out"][k * 128 + 42:k * 128 + 46].tobytes(), "big") == int(new_tx["snd_nxt"][k])
