"""A data transfer between two endpoints on one MI355X with the sender's whole steady state on the device, checked
without tests/tcp_ack_reference.py: the sender pushes 64 KiB on each of 4 connections through a send window of
4 x mss; the peer receives and reassembles; the test writes the peer's pure ACKs (tests/frames.py); the sender's receive
path, dk_tcp_rx_process and dk_tcp_ack_process move SND.UNA and the window, so the next round's dk_tcp_tx_segment can send
again. Without dk_tcp_ack_process the sender stalls after the first window.

Each round: TcpSender.segment_batch; UnackedQueue.append_frames (the frames must be in the queue before their ACK
is processed); the peer's RxEngine + TcpReceiver; one pure ACK per connection from the peer's RCV.NXT; the sender's
RxEngine + TcpReceiver + TcpAcker. The host reads what an application reads (how much of its buffer went out, what was
delivered), never a per-segment array of the ACK path."""
import numpy as np
import pytest

import frames as F
import tx_segment_reference as M
from demikernel_amd import (Config, FrameBatch, PushList, RxEngine, SocketId, TcpAcker, TcpAckOut, TcpSender,
                            TcpTxResults, UnackedQueue, ack_conn_table, flow_array, sync_send_next, synth, tx_conn_table)
from demikernel_amd import _native as N
from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table

pytestmark = pytest.mark.gpu

NC, TOTAL, MSS, WINDOW = 4, 65536, 1460, 4 * 1460
ROUNDS = -(-TOTAL // WINDOW) + 2  # what the window arithmetic gives: ceil(65,536 / (4 x 1,460)) + 2 = 14
FIN_CONNS = (1, 3)
A_IP, B_IP, B_PORT = synth.ALICE_IPV4, synth.BOB_IPV4, 12345


def test_transfer_with_acks_on_the_device():
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2024)
    a_port = [40000 + c for c in range(NC)]
    flows_b = flow_array([SocketId.Active((B_IP, B_PORT), (A_IP, a_port[c])) for c in range(NC)])  # at the peer
    flows_a = flow_array([SocketId.Active((A_IP, a_port[c]), (B_IP, B_PORT)) for c in range(NC)])  # at the sender
    isn = rng.integers(0, 1 << 32, NC, dtype=np.uint64).astype(np.uint32)
    isn[0] = (1 << 32) - 30000  # one stream wraps
    irs = rng.integers(0, 1 << 32, NC, dtype=np.uint64).astype(np.uint32)  # the peer's own sequence numbers (no data)

    # the sender: send sides, ACK state, queue, and the receive side its ACKs come in on
    sender, eng_a, tcp_a, acker = TcpSender(0), RxEngine(Config(A_IP), device=0), TcpReceiver(0), TcpAcker()
    eng_a.set_sockets(flows_a)
    tx = M.conns_toward(flows_b, snd_nxt=isn, rcv_nxt=irs, snd_wnd=WINDOW, mss=MSS, rcv_wnd_hdr=65535, link=0)
    d_tx = sender.conns_to_device(tx)
    d_ak = TcpAcker.conns_to_device(ack_conn_table(NC, wl1=irs, wl2=isn))
    queue = UnackedQueue(NC, 16)
    d_rx_a = tcp_a.conns_to_device(conn_table(NC, receive_next=irs, send_next=isn))
    d_links = torch.from_numpy(np.ascontiguousarray(M.links_table()).view(np.uint8).copy()).to(dev)
    # the peer
    eng_b, tcp_b = RxEngine(Config(B_IP), device=0), TcpReceiver(0)
    eng_b.set_sockets(flows_b)
    d_rx_b = tcp_b.conns_to_device(conn_table(NC, receive_next=isn, send_next=irs, buffer_size=1 << 20))

    src = rng.integers(0, 256, NC * TOTAL, dtype=np.uint8)
    d_src = torch.from_numpy(src).to(dev)
    stride, cap = 1536, 8 * NC
    d_out = torch.zeros(cap * stride, dtype=torch.uint8, device=dev)
    pushed = np.zeros(NC, np.int64)  # bytes of each connection's buffer that went out
    fin_out = np.zeros(NC, bool)
    received = [bytearray() for _ in range(NC)]
    rounds = 0
    now = 10**9
    for rnd in range(ROUNDS + 4):
        una = sender.conns_to_host(d_tx)["snd_una"]
        want = (isn.astype(np.int64) + TOTAL + np.isin(np.arange(NC), FIN_CONNS)) & 0xFFFFFFFF
        if (una == want).all():
            break
        rounds += 1
        pc, po, pl = [], [], []
        for c in range(NC):
            if pushed[c] < TOTAL:
                pc.append(c), po.append(c * TOTAL + pushed[c]), pl.append(TOTAL - pushed[c])
            if c in FIN_CONNS and not fin_out[c]:
                pc.append(c), po.append(0), pl.append(0)  # the end-of-send marker
        sent_n = 0
        if pc:
            push = PushList.from_numpy(pc, po, pl)
            res = TcpTxResults(cap, len(pc))
            batch = sender.segment_batch(d_src, push, d_tx, d_links, d_out, res, slot_stride=stride)
            sent_n = batch.n
            h = res.to_numpy()
            for b, c in enumerate(pc):
                if pl[b]:
                    pushed[c] += int(h["sent"][b])
                elif h["status"][b] == N.DK_TCP_TX_SENT:
                    fin_out[c] = True
            queue.append_frames(d_ak, res, push, now, sent_n)
        if sent_n:  # the peer receives
            r = eng_b.results(sent_n, tcp_fields=True)
            eng_b.receive_batch(batch, r)
            out_b = TcpOut(sent_n, NC)
            tcp_b.process(r, d_rx_b, out_b)
            torch.cuda.synchronize()
            hb, blob, off = out_b.to_numpy(), d_out.cpu().numpy(), batch.off.cpu().numpy().view(np.uint32)
            assert set(hb["action"]) <= {N.A["DELIVERED"], N.A["FIN"]}, hb["action"]
            for c in range(NC):
                for v in out_b.delivered(c, hb):
                    if v["ref"] != N.DK_TCP_REF_EOF:
                        s = int(off[v["ref"]]) + int(v["off"])
                        received[c] += blob[s:s + int(v["len"])].tobytes()
        # the peer's ACKs: one per connection, from its RCV.NXT
        rn_b = tcp_b.conns_to_host(d_rx_b)["receive_next"]
        acks = [F.tcp_frame(b"", src=B_IP, dst=A_IP, sport=B_PORT, dport=a_port[c],
                            tcp_kw=dict(seq=int(irs[c]), ack=int(rn_b[c]), flags=0x10, window=WINDOW)) for c in range(NC)]
        ablob, aoff, alens = F.pack(acks)
        now += 500000
        sync_send_next(d_rx_a, d_tx)
        ra = eng_a.results(NC, tcp_fields=True)
        eng_a.receive_batch(FrameBatch.from_numpy(ablob, aoff, alens, device=0), ra)
        out_a, aout = TcpOut(NC, NC), TcpAckOut(NC, NC)
        tcp_a.process(ra, d_rx_a, out_a)
        acker.process(tcp_a, ra, out_a, d_rx_a, d_tx, d_ak, queue, now, aout)
        now += 500000
    torch.cuda.synchronize()
    st = aout.to_numpy()
    assert (st["status"] == 0).all(), st
    tx_end, ak_end = sender.conns_to_host(d_tx), TcpAcker.conns_to_host(d_ak)
    for c in range(NC):  # the peer's delivered views read back as the pushed bytes, in order
        assert bytes(received[c]) == src[c * TOTAL:(c + 1) * TOTAL].tobytes(), f"connection {c}'s stream"
    fin = np.isin(np.arange(NC), FIN_CONNS)
    assert np.array_equal(tx_end["snd_una"], ((isn.astype(np.int64) + TOTAL + fin) & 0xFFFFFFFF).astype(np.uint32))
    assert np.array_equal(tx_end["snd_una"], tx_end["snd_nxt"])
    assert (ak_end["q_count"] == 0).all() and (ak_end["rtx_armed"] == 0).all(), ak_end
    assert rounds <= ROUNDS, rounds
    assert rounds >= -(-TOTAL // WINDOW)  # and the window really limited every round
    assert (tx_end["snd_wnd"] == WINDOW).all()
    # every sample was 0.5 ms: srtt = 0.0005, the RTO sits on its lower clamp
    assert (ak_end["received_sample"] == 1).all() and (ak_end["rto"] == 0.1).all()
    assert np.allclose(ak_end["srtt"], 0.0005, rtol=1e-9, atol=0)
    peer_end = tcp_b.conns_to_host(d_rx_b)
    assert (peer_end["state"][fin] == N.DK_TCP_CLOSED).all() and (peer_end["state"][~fin] == N.DK_TCP_ESTABLISHED).all()
    for o in (sender, eng_a, tcp_a, eng_b, tcp_b):
        o.close()
