"""TCP receive as a byte stream across calls on the MI355X (tests/stream_net.py): every case's recorded batches — a
go-back-N sender that re-cuts its retransmissions, a lossy network, a lazy reader, the out-of-order store carried by
handles — through dk_rx_process and dk_tcp_rx_process on a device table that is downloaded, rewritten and uploaded
between calls. After every call the outputs and the table are first compared bit for bit with the oracle chain's
(so a divergence is reported at the first call that shows it), then StreamChecker (no oracle inside) reassembles the
delivered and stored views from the bytes read back from the device blob. Every case runs through the four forced walks
and once under the engine's own rule on one context; the 254-flow case also with the radix sort forced; one case has its
frames cut on the GPU by dk_tcp_tx_segment."""
import functools

import numpy as np
import pytest

import stream_net as SN
import tx_segment_reference as M
from demikernel_amd import Config, FrameBatch, RxEngine, synth
from demikernel_amd import _native as N
from demikernel_amd.tcp import TcpOut, TcpReceiver
from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults
from oracle import oracle as O
from oracle.oracle import OraclePeer
from test_gpu_tcp import assert_same

pytestmark = pytest.mark.gpu


def replay(name: str, tcp: TcpReceiver):
    """The case's trace on one TcpReceiver; returns the walk and the sort of every call."""
    import torch

    tr = SN.trace(name)
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    eng.set_sockets(tr.flows)
    chk = SN.StreamChecker(tr.irs, tr.case.stream, tr.table0)
    got_t = tr.table0.copy()
    dev = tcp.conns_to_device(got_t)
    walks, sorts = [], []
    for k, call in enumerate(tr.calls):
        n = len(call.off)
        batch = FrameBatch.from_numpy(call.blob, call.off, call.lens, device=0)
        r = eng.results(n, tcp_fields=True)
        eng.receive_batch(batch, r)
        out = TcpOut(n, len(got_t))
        tcp.process(r, dev, out)
        torch.cuda.synchronize()
        got, got_t = out.to_numpy(), tcp.conns_to_host(dev)
        walks.append(tcp.last_walk)
        sorts.append(tcp.last_sort)
        assert_same(got_t, got, call.exp_table, call.exp, f"{name} call {k} ({walks[-1]} walk, {sorts[-1]} sort)")
        chk.feed(got, got_t, batch.blob.cpu().numpy(), call.off, call.lens, call.gidx, call.pay_off, call.pay_len)
        SN.after_call(got_t, call)  # the handle rewrite and the application's reads, as the oracle's table got them
        dev = tcp.conns_to_device(got_t)
    chk.finish(got_t, tr.final_snd_nxt, tr.exempt)
    eng.close()
    return walks, sorts


def rule_sort(tr) -> str:
    return "counting" if len(tr.table0) <= 255 else "radix"  # tcp_kernels.hip kSortMaxRows


@pytest.mark.parametrize("walk", ["lane", "wave", "relay", "scan"])
@pytest.mark.parametrize("name", list(SN.CASES))
def test_streams_forced_walk(name, walk):
    tcp = TcpReceiver(0, walk=walk)
    try:
        walks, sorts = replay(name, tcp)
    finally:
        tcp.close()
    assert set(walks) == {walk} and set(sorts) == {rule_sort(SN.trace(name))}


@functools.lru_cache(maxsize=None)
def rule_run(name: str):
    tcp = TcpReceiver(0)
    try:
        return replay(name, tcp)
    finally:
        tcp.close()


@pytest.mark.parametrize("name", list(SN.CASES))
def test_streams_engine_rule(name):
    """One TcpReceiver for the whole case, no walk forced: the rule changes walk with the batch's shape mid-case. Below
    16 rows the stored fraction plays no part (tcp_kernels.hip pick_walk), so the walk of every call is known."""
    tr = SN.trace(name)
    walks, sorts = rule_run(name)
    print(name, "walks by rule:", walks)
    assert set(sorts) == {rule_sort(tr)}
    rows = len(tr.table0)
    if rows < 16:
        want = ["lane" if len(c.off) < 8 * rows else "scan" if len(c.off) >= 1024 * rows else "wave" for c in tr.calls]
        assert walks == want
    if name.startswith("wide"):
        assert set(walks) == {"lane"}


def test_engine_rule_ran_more_than_one_walk():
    seen = set()
    for name in SN.CASES:
        seen |= set(rule_run(name)[0])
    assert len(seen) > 1 and {"scan", "wave", "lane"} <= seen, seen


def test_wide_254_radix_sort_forced():
    tcp = TcpReceiver(0, radix_sort=True)
    try:
        walks, sorts = replay("wide_254", tcp)
    finally:
        tcp.close()
    assert set(sorts) == {"radix"}


def test_device_sender_streams():
    """The sender on the GPU: each round the host rewinds snd_nxt / snd_una of the sender table to the receiver's
    RCV.NXT and pushes the unsent remainder with that round's MSS (the send window limits the flight); dk_tcp_tx_segment
    cuts it into frames; the network is an index gather of the frame descriptors; the frames go through the receive path
    and the oracle chain in lockstep. S1-S5, and SND.NXT == RCV.NXT at the end."""
    import torch

    case = SN.DEVICE_CASE
    flows, exp_t, irs = SN.initial_table(case)
    nc, L = case.nconns, case.stream
    rng = np.random.default_rng(case.seed)
    dev = torch.device("cuda", 0)
    sender, tcp = TcpSender(0), TcpReceiver(0)
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    eng.set_sockets(flows)
    peer = OraclePeer(synth.ipv4(synth.BOB_IPV4))
    peer.set_flows(flows)
    src = SN.stream_bytes(np.repeat(np.arange(nc), L), np.tile(np.arange(L), nc))  # connection c's stream at c * L
    stride, lead = 192, 2
    cap = nc * (L // min(case.mss) + 2)
    d_src = torch.from_numpy(src).to(dev)
    d_out = torch.zeros(cap * stride, dtype=torch.uint8, device=dev)
    d_links = torch.from_numpy(np.ascontiguousarray(M.links_table()).view(np.uint8).copy()).to(dev)
    tx = M.conns_toward(flows, snd_nxt=irs, rcv_nxt=exp_t["send_next"], mss=64)
    chk = SN.StreamChecker(irs, L, exp_t)
    got_t = exp_t.copy()
    d_rx = tcp.conns_to_device(got_t)
    base, st, hist = 0, {}, np.zeros(len(N.TCP_ACTIONS), np.int64)
    for rnd in range(SN.CALL_CAP + 1):
        opened = np.nonzero(got_t["state"] == N.DK_TCP_ESTABLISHED)[0]
        if not len(opened):
            break
        lossy = rnd < case.lossy
        tx["snd_nxt"][opened] = tx["snd_una"][opened] = got_t["receive_next"][opened]
        tx["fin_sent"][opened] = 0
        tx["mss"] = rng.choice(case.mss, nc)
        tx["snd_wnd"] = tx["mss"] * rng.integers(1, case.flight + 1, nc)
        pc, po, pl = [], [], []
        for c in opened:
            start = (int(got_t["receive_next"][c]) - int(irs[c])) & SN.M32
            if start < L:
                pc.append(c), po.append(c * L + start), pl.append(L - start)
            pc.append(c), po.append(0), pl.append(0)  # the end-of-send marker: FIN
        d_tx = sender.conns_to_device(tx)
        res = TcpTxResults(cap, len(pc))
        sent = sender.segment_batch(d_src, PushList.from_numpy(pc, po, pl), d_tx, d_links, d_out, res,
                                    slot_stride=stride, frame_lead=lead)
        tx = sender.conns_to_host(d_tx)
        h = res.to_numpy()
        assert sent.n == h["frames_written"] > 0
        conn = np.asarray(pc)[h["frame_buf"]]
        rank = np.arange(sent.n) - np.searchsorted(conn, conn)  # a connection's frames are consecutive
        idx = SN.network(conn, rank, lossy, case, rng)
        if not len(idx):
            idx = np.array([0])
        it = torch.from_numpy(idx).to(dev)
        batch = FrameBatch(d_out, sent.off[it].contiguous(), sent.len[it].contiguous())
        n = len(idx)
        r = eng.results(n, tcp_fields=True)
        eng.receive_batch(batch, r)
        out = TcpOut(n, nc)
        tcp.process(r, d_rx, out)
        torch.cuda.synchronize()
        got, got_t = out.to_numpy(), tcp.conns_to_host(d_rx)
        blob, off, lens = d_out.cpu().numpy(), h["off_out"][idx], h["len_out"][idx]
        exp = O.tcp_process(exp_t, peer.process(blob, off, lens))
        assert_same(got_t, got, exp_t, exp, f"device sender call {rnd} ({tcp.last_walk} walk)")
        call = SN.Call(blob, off, lens, (base + idx).astype(np.uint32), np.full(n, 54, np.uint32),
                       lens.astype(np.uint32) - 54, conn[idx], lossy)
        chk.feed(got, got_t, blob, off, lens, call.gidx, call.pay_off, call.pay_len)
        call.reads = SN.reads_after(exp_t, case, lossy, st, rng)
        SN.after_call(exp_t, call)
        SN.after_call(got_t, call)
        d_rx = tcp.conns_to_device(got_t)
        base += sent.n
        hist += np.bincount(got["action"], minlength=len(hist))
    final = (irs.astype(np.uint64) + L + 1).astype(np.uint32)
    chk.finish(got_t, final)
    assert np.array_equal(tx["snd_nxt"], got_t["receive_next"])
    assert hist[N.A["STORED"]] > 0 and hist[N.A["FIN"]] == nc and chk.via_handle > 0, (hist, chk.via_handle)
    for o in (sender, tcp, eng):
        o.close()
