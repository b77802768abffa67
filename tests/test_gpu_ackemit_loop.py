"""A transfer between two endpoints on one MI355X with no frame built or edited on the host: A pushes 16 KiB on each of
4 connections through dk_tcp_tx_segment; B runs dk_rx_process, dk_tcp_rx_process and dk_tcp_ack_emit; B's ACK frames go
straight into A's dk_rx_process, dk_tcp_rx_process and dk_tcp_ack_process, which move SND.UNA so the next round can send.
Each stream is 11 segments of 1,500 bytes: B acknowledges every second one (the delayed ACK), so the last stays
unacknowledged until one dk_tcp_ack_timer call flushes it. Without dk_tcp_ack_emit A stalls after its first flight of
3 segments.

The host reads what an application and a timer wheel read: how much of the pushed buffer went out, what was delivered,
SND.UNA to know when it is done, and deadline_ns to name the expired delayed ACKs."""
import numpy as np
import pytest

import tx_segment_reference as M
from demikernel_amd import (AckEmitResults, Config, PushList, RxEngine, SocketId, TcpAcker, TcpAckOut, TcpSender,
                            TcpTxResults, UnackedQueue, ack_conn_table, ack_emit_batch, dack_conn_table, flow_array,
                            sync_send_next, synth)
from demikernel_amd import _native as N
from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table
from demikernel_amd.tcp_ackemit import ack_timer_batch, dack_to_device, dack_to_host
from demikernel_amd.tcp_rtx import fire_to_device

pytestmark = pytest.mark.gpu

NC, TOTAL, MSS, FLIGHT = 4, 16384, 1500, 3
SEGS = -(-TOTAL // MSS)  # 11: odd, so the last segment's ACK is a delayed one
A_IP, B_IP, B_PORT = synth.ALICE_IPV4, synth.BOB_IPV4, 12345
WSCALE, BUFFER, DELAY = 6, 1 << 20, 40_000_000


def test_transfer_with_both_directions_on_the_device():
    import torch

    assert SEGS % 2 == 1
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2025)
    a_port = [40000 + c for c in range(NC)]
    flows_b = flow_array([SocketId.Active((B_IP, B_PORT), (A_IP, a_port[c])) for c in range(NC)])  # at B
    flows_a = flow_array([SocketId.Active((A_IP, a_port[c]), (B_IP, B_PORT)) for c in range(NC)])  # at A
    isn = rng.integers(0, 1 << 32, NC, dtype=np.uint64).astype(np.uint32)
    isn[0] = (1 << 32) - 9000  # one stream wraps
    irs = rng.integers(0, 1 << 32, NC, dtype=np.uint64).astype(np.uint32)  # B's own sequence numbers (it sends no data)
    d_links = torch.from_numpy(np.ascontiguousarray(M.links_table()).view(np.uint8).copy()).to(dev)

    # A: send sides, ACK state, queue, and the receive side B's ACKs come in on
    sender, eng_a, tcp_a, acker = TcpSender(0), RxEngine(Config(A_IP), device=0), TcpReceiver(0), TcpAcker()
    eng_a.set_sockets(flows_a)
    tx_a = M.conns_toward(flows_b, snd_nxt=isn, rcv_nxt=irs, snd_wnd=65535, cwnd=FLIGHT * MSS, mss=MSS, link=0)
    d_tx_a = sender.conns_to_device(tx_a)
    d_ak = TcpAcker.conns_to_device(ack_conn_table(NC, wl1=irs, wl2=isn, snd_wscale=WSCALE))
    queue = UnackedQueue(NC, 16)
    d_rx_a = tcp_a.conns_to_device(conn_table(NC, receive_next=irs, send_next=isn))
    # B: its receive side, the send side its ACKs are built from, its delayed-ACK state
    eng_b, tcp_b, timer_b = RxEngine(Config(B_IP), device=0), TcpReceiver(0), TcpSender(0)
    eng_b.set_sockets(flows_b)
    d_rx_b = tcp_b.conns_to_device(conn_table(NC, receive_next=isn, send_next=irs, buffer_size=BUFFER))
    d_tx_b = timer_b.conns_to_device(M.conns_toward(flows_a, snd_nxt=irs, rcv_wscale=WSCALE, link=1))
    d_dack = dack_to_device(dack_conn_table(NC, delay_ns=DELAY))

    src = rng.integers(0, 256, NC * TOTAL, dtype=np.uint8)
    d_src = torch.from_numpy(src).to(dev)
    stride, cap = 1600, 8 * NC
    d_out = torch.zeros(cap * stride, dtype=torch.uint8, device=dev)    # A's frames
    d_acks = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)       # B's
    pushed = np.zeros(NC, np.int64)
    received = [bytearray() for _ in range(NC)]
    want_una = ((isn.astype(np.int64) + TOTAL) & 0xFFFFFFFF).astype(np.uint32)
    now, rounds, ack_frames, flushed, aout = 10**9, 0, 0, 0, None

    def into_a(batch):
        """B's frames, as they lie in device memory, through A's receive path and ACK processing."""
        nonlocal aout
        sync_send_next(d_rx_a, d_tx_a)
        ra = eng_a.results(batch.n, tcp_fields=True)
        eng_a.receive_batch(batch, ra)
        out_a, aout = TcpOut(batch.n, NC), TcpAckOut(batch.n, NC)
        tcp_a.process(ra, d_rx_a, out_a)
        acker.process(tcp_a, ra, out_a, d_rx_a, d_tx_a, d_ak, queue, now, aout)
        torch.cuda.synchronize()
        ha = ra.to_numpy()
        assert ((ha["meta"] & 0xFF) == N.V["OK_TCP"]).all(), ha["meta"] & 0xFF
        assert (out_a.to_numpy()["action"] == N.A["NO_DATA"]).all() and (aout.to_numpy()["status"] == 0).all()

    for rnd in range(4 * SEGS):
        una = sender.conns_to_host(d_tx_a)["snd_una"]
        if (una == want_una).all():
            break
        rounds += 1
        pc = [c for c in range(NC) if pushed[c] < TOTAL]
        sent_n = 0
        if pc:
            push = PushList.from_numpy(pc, [c * TOTAL + pushed[c] for c in pc], [TOTAL - pushed[c] for c in pc])
            res = TcpTxResults(cap, len(pc))
            batch = sender.segment_batch(d_src, push, d_tx_a, d_links, d_out, res, slot_stride=stride)
            sent_n = batch.n
            for b, c in enumerate(pc):
                pushed[c] += int(res.to_numpy()["sent"][b])
            queue.append_frames(d_ak, res, push, now, sent_n)
        now += 500000
        if sent_n:  # B receives, delivers and acknowledges
            r = eng_b.results(sent_n, tcp_fields=True)
            eng_b.receive_batch(batch, r)
            out_b = TcpOut(sent_n, NC)
            tcp_b.process(r, d_rx_b, out_b)
            ares = AckEmitResults(cap, NC, sent_n)
            acks = ack_emit_batch(tcp_b, r, out_b, d_rx_b, d_tx_b, d_dack, d_links, now, d_acks, ares, slot_stride=64)
            hb, blob, off = out_b.to_numpy(), d_out.cpu().numpy(), batch.off.cpu().numpy().view(np.uint32)
            assert (hb["action"] == N.A["DELIVERED"]).all() and (ares.to_numpy()["status"] == 0).all()
            for c in range(NC):
                for v in out_b.delivered(c, hb):
                    s = int(off[v["ref"]]) + int(v["off"])
                    received[c] += blob[s:s + int(v["len"])].tobytes()
            now += 500000
            if acks.n:
                ack_frames += acks.n
                into_a(acks)
        else:
            # nothing left to send and something still unacknowledged: B's delayed-ACK timer runs out
            dk = dack_to_host(d_dack)
            assert (dk["armed"] == 1).all() and (una != want_una).all(), (dk, una)
            now = int(dk["deadline_ns"].max())
            fire = ((dk["armed"] != 0) & (dk["deadline_ns"] <= now)).astype(np.uint8)
            ares = AckEmitResults(cap, NC)
            acks = ack_timer_batch(timer_b, fire_to_device(fire), d_tx_b, d_rx_b, d_dack, d_links, d_acks, ares,
                                   slot_stride=64)
            assert acks.n == NC and (ares.to_numpy()["status"] == 0).all()
            flushed += 1
            ack_frames += acks.n
            into_a(acks)
    torch.cuda.synchronize()
    tx_end, ak_end = sender.conns_to_host(d_tx_a), TcpAcker.conns_to_host(d_ak)
    for c in range(NC):
        assert bytes(received[c]) == src[c * TOTAL:(c + 1) * TOTAL].tobytes(), f"connection {c}'s stream"
    assert np.array_equal(tx_end["snd_una"], want_una) and np.array_equal(tx_end["snd_una"], tx_end["snd_nxt"])
    assert (ak_end["q_count"] == 0).all() and (ak_end["rtx_armed"] == 0).all(), ak_end
    assert flushed == 1, flushed
    assert ack_frames == NC * (SEGS // 2 + 1), ack_frames  # one per two segments, and the flush
    assert (dack_to_host(d_dack)["armed"] == 0).all()
    # the window B advertised last, through both scale shifts: its application has read nothing yet
    assert (tx_end["snd_wnd"] == BUFFER - TOTAL).all() and TOTAL % (1 << WSCALE) == 0
    peer_end = tcp_b.conns_to_host(d_rx_b)
    assert np.array_equal(peer_end["receive_next"], want_una) and rounds <= SEGS
    for o in (sender, eng_a, tcp_a, eng_b, tcp_b, timer_b):
        o.close()
