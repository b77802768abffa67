"""Two endpoints on the MI355X with empty ARP caches: the client's query for the server is broadcast, the server's
receive engine and dk_arp_process learn the client and answer, the client's dk_arp_process resolves the row and writes
links[], dk_tcp_connect_start sends the SYN with that array, and the handshake completes as in
tests/test_gpu_connect_net.py. Each side's output blob is the other side's receive batch; after setup the host writes
no MAC, ARP frame or link entry. The assertions are on the bytes: the reference's destination-MAC check is warn-only,
so the receive engine gives no verdict for it. In the second part the server stays silent and the client's row fails
with ETIMEDOUT after retry_count + 1 requests, and no SYN is sent."""
import errno

import numpy as np
import pytest

import arp_cases as C
import tcp_listen_cases as LC
from demikernel_amd import Config, FrameBatch, RxEngine, SocketId, flow_array, ipv4
from demikernel_amd import _native as N
from demikernel_amd import arp as ARP
from demikernel_amd import tcp_connect as TC
from demikernel_amd import tcp_listen as TL

pytestmark = pytest.mark.gpu

ALICE, BOB = C.ALICE, C.BOB
AM, BM = C.ALICE_MAC, C.BOB_MAC
STRIDE = 64
RETRIES = 2


def wire(out, got):
    """The call's frames as the other side's batch, on the device."""
    import torch

    w = got["n_frames"]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a[:w]).view(dt).copy()).cuda()  # noqa: E731
    return FrameBatch(out, up(got["off_out"], np.int32), up(got["len_out"], np.int16))


def frames_of(out, got):
    b = out.cpu().numpy()
    return [bytes(b[int(o):int(o) + int(ln)]) for o, ln in zip(got["off_out"][:got["n_frames"]], got["len_out"][:got["n_frames"]])]


class Side:
    def __init__(self, ip, mac, flows):
        import torch

        self.eng = RxEngine(Config(ip), device=0)
        self.eng.set_sockets(flows)
        self.arp = ARP.ArpTable(16, ARP.arp_cfg(ipv4(ip), mac, cache_ttl_ns=C.TTL, request_timeout_ns=C.SEC, retry_count=RETRIES))
        link = np.zeros(1, N.TX_LINK_DTYPE)  # setup: the local address only; the peer's is the ARP peer's to write
        link["src_mac"] = np.frombuffer(mac, np.uint8)
        self.links = ARP.to_device(link)
        self.out = lambda: torch.full((4 * STRIDE,), 0xA5, dtype=torch.uint8, device="cuda:0")

    def close(self):
        self.arp.close()
        self.eng.close()

    def rx(self, batch):
        r = self.eng.results(batch.n, tcp_fields=True, tcp_opts=True)
        self.eng.receive_batch(batch, r)
        return r

    def arp_process(self, batch, rows=None, clock=0):
        import torch

        r, out, res = self.rx(batch), self.out(), ARP.ArpResults(batch.n, 4, 4, 1)
        ARP.arp_process(self.arp, batch, r, rows, self.links, clock, out, res, slot_stride=STRIDE)
        torch.cuda.synchronize()
        return out, res.to_numpy()


@pytest.fixture
def sides():
    cflows = flow_array([SocketId.Active((ALICE, 30000), (BOB, 80))])
    sflows, L, lsn = LC.server([80], max_backlog=8)
    cl, sv = Side(ALICE, AM, cflows), Side(BOB, BM, sflows)
    yield cl, sv, L, lsn
    cl.close()
    sv.close()


def client_rows():
    crow = TC.connector_table(1, flow_id=0, local_ip=ipv4(ALICE), local_port=30000, remote_ip=ipv4(BOB), remote_port=80, link=0)
    q = ARP.query_table(1, ip=ipv4(BOB), link=0, tag=0)
    return crow, TC.to_device(crow), ARP.to_device(q)


def test_arp_then_handshake_with_no_host_made_mac(sides):
    import torch

    cl, sv, L, lsn = sides
    crow, d_conn, d_q = client_rows()
    d_start = ARP.to_device(np.array([0], np.uint32))
    # the client's query: a broadcast request
    out, res = cl.out(), ARP.ArpResults(4, 4, 4, 1)
    ARP.arp_query_start(cl.arp, d_q, d_start, cl.links, 0, out, res, slot_stride=STRIDE)
    torch.cuda.synchronize()
    got = res.to_numpy()
    assert (got["n_frames"], got["n_ready"], int(got["status"][0])) == (1, 0, ARP.OK)
    (request,) = frames_of(out, got)
    assert request[:6] == b"\xff" * 6 and request[6:12] == AM and request[20:22] == b"\x00\x01"
    assert not cl.links.cpu().numpy().view(N.TX_LINK_DTYPE)[0]["dst_mac"].any()
    # the server learns the client and answers
    sout, sgot = sv.arp_process(wire(out, got))
    assert list(sgot["action"]) == [ARP.LEARNED | ARP.INSERTED | ARP.REPLY] and sgot["n_frames"] == 1
    assert sv.arp.as_map() == {ipv4(ALICE): (AM, C.TTL)}
    (reply,) = frames_of(sout, sgot)
    assert reply[:6] == AM and reply[6:12] == BM and reply[20:22] == b"\x00\x02"
    # the client resolves the row and writes links[]
    cout, cgot = cl.arp_process(wire(sout, sgot), rows=d_q)
    assert (cgot["n_frames"], cgot["n_ready"]) == (0, 1)
    y = cgot["ready"][0]
    assert (int(y["row"]), int(y["tag"]), int(y["err"]), bytes(y["mac"])) == (0, 0, 0, BM)
    assert int(ARP.rows_to_host(d_q)[0]["state"]) == ARP.RESOLVED
    # start[] from the ready records' tags; links[] goes to dk_tcp_connect_start as the device left it
    start = ARP.to_device(np.array([int(r["tag"]) for r in cgot["ready"][:cgot["n_ready"]] if not r["err"]], np.uint32))
    gen = TC.to_device(TC.isn_gen(0x1234, 7))
    out, res = cl.out(), TC.ConnectResults(4, 4, 4, 1)
    TC.connect_start(d_conn, start, gen, cl.links, 10, out, res, slot_stride=STRIDE)
    torch.cuda.synchronize()
    got = res.to_numpy()
    assert got["n_frames"] == 1 and int(got["status"][0]) == TC.OK
    (syn,) = frames_of(out, got)
    assert syn[:6] == BM and syn[6:12] == AM and len(syn) == TC.SYN_BYTES and syn[47] == 0x02
    # the server: try_query before it answers the SYN, then the SYN+ACK goes to the MAC its own lookup put into its link
    syn_batch = wire(out, got)
    rx = sv.rx(syn_batch)
    found, macs = ARP.arp_lookup(sv.arp, [ipv4(ALICE)], sv.links, [0])
    assert list(found) == [1] and bytes(macs[0]) == AM
    table = TL.ListenTable(16)
    try:
        d_l, d_map = TL.to_device(L), TL.to_device(lsn)
        sout, sres = sv.out(), TL.ListenResults(1, 4, 4, 1)
        TL.listen_process(table, rx, d_l, d_map, sv.links, 20, sout, sres, slot_stride=STRIDE, backlog_sum=8)
        torch.cuda.synchronize()
        sgot = sres.to_numpy()
        assert list(sgot["action"]) == [TL.SYN_ACCEPTED] and sgot["n_frames"] == 1
        (synack,) = frames_of(sout, sgot)
        assert synack[:6] == AM and synack[6:12] == BM and synack[47] == 0x12
        # the client: ESTABLISHED, and the handshake ACK with the same link
        rx = cl.rx(wire(sout, sgot))
        cmap = TC.to_device(TC.conn_of_flow(1, crow))
        out, res = cl.out(), TC.ConnectResults(1, 4, 4, 1)
        TC.connect_process(rx, d_conn, cmap, cl.links, 30, out, res, slot_stride=STRIDE)
        torch.cuda.synchronize()
        got = res.to_numpy()
        assert list(got["action"]) == [TC.ESTABLISHED] and (got["n_frames"], got["n_ready"]) == (1, 1)
        assert int(got["ready"][0]["err"]) == 0
        (ack,) = frames_of(out, got)
        assert ack[:6] == BM and ack[6:12] == AM and ack[47] == 0x10
        # the server: the handshake completes
        rx = sv.rx(wire(out, got))
        sout, sres = sv.out(), TL.ListenResults(1, 4, 4, 1)
        TL.listen_process(table, rx, d_l, d_map, sv.links, 40, sout, sres, slot_stride=STRIDE, backlog_sum=8)
        torch.cuda.synchronize()
        sgot = sres.to_numpy()
        assert list(sgot["action"]) == [TL.ESTABLISHED] and sgot["n_ready"] == 1 and int(sgot["ready"][0]["err"]) == 0
        assert int(sgot["ready"][0]["rcv_nxt"]) == int(got["ready"][0]["snd_nxt"])
        assert int(sgot["ready"][0]["snd_nxt"]) == int(got["ready"][0]["rcv_nxt"])
    finally:
        table.close()
    # the links as the device left them: the peer's MAC, and the host's src_mac and reserved untouched
    for side, peer, own in ((cl, BM, AM), (sv, AM, BM)):
        lk = side.links.cpu().numpy().view(N.TX_LINK_DTYPE)[0]
        assert (bytes(lk["dst_mac"]), bytes(lk["src_mac"]), int(lk["reserved"])) == (peer, own, 0)


def test_silent_server_fails_the_query_and_no_syn_is_sent(sides):
    import torch

    cl, sv, L, lsn = sides
    crow, d_conn, d_q = client_rows()
    out, res = cl.out(), ARP.ArpResults(4, 4, 4, 1)
    ARP.arp_query_start(cl.arp, d_q, ARP.to_device(np.array([0], np.uint32)), cl.links, 0, out, res, slot_stride=STRIDE)
    torch.cuda.synchronize()
    requests, ready = res.to_numpy()["n_frames"], []
    for k in range(1, RETRIES + 3):
        out, res = cl.out(), ARP.ArpResults(4, 4, 4, 1)
        ARP.arp_timers(cl.arp, d_q, cl.links, k * C.SEC, out, res, slot_stride=STRIDE)
        torch.cuda.synchronize()
        got = res.to_numpy()
        requests += got["n_frames"]
        ready.extend(got["ready"][:got["n_ready"]])
    assert requests == RETRIES + 1 and len(ready) == 1
    assert (int(ready[0]["row"]), int(ready[0]["err"])) == (0, errno.ETIMEDOUT)
    q = ARP.rows_to_host(d_q)[0]
    assert (int(q["state"]), int(q["err"]), int(q["sent"])) == (ARP.FAILED, errno.ETIMEDOUT, RETRIES + 1)
    # no successful record, so start[] is empty: no SYN, and the link still has no destination
    start = [int(r["tag"]) for r in ready if not r["err"]]
    assert start == []
    out, res = cl.out(), TC.ConnectResults(4, 4, 4, 1)
    TC.connect_start(d_conn, torch.zeros(4, dtype=torch.uint8, device="cuda:0"), TC.to_device(TC.isn_gen(1, 1)), cl.links, 5 * C.SEC,
                     out, res, slot_stride=STRIDE, nstart=0)
    torch.cuda.synchronize()
    assert res.to_numpy()["n_frames"] == 0 and (out.cpu().numpy() == 0xA5).all()
    assert int(TC.rows_to_host(d_conn)[0]["state"]) == TC.IDLE
    assert not cl.links.cpu().numpy().view(N.TX_LINK_DTYPE)[0]["dst_mac"].any()
