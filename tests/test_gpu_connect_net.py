"""The handshake as a closed loop on the MI355X: 200 connectors on the device (dk_tcp_connect_*) connect to listeners on
the device (dk_tcp_listen_*) through two receive engines, one per side. No frame is built or parsed on the host: each
side's output blob is the other side's receive batch, and the host only chooses which frame indices of a batch are lost
and advances the two clocks. Every device call is compared whole with its model (the Devices of
tests/test_gpu_tcp_connect.py and tests/test_gpu_tcp_listen.py), so both models predict every outcome:
  * a lost first SYN: the client's timer resends it and the handshake completes;
  * a lost first SYN+ACK: the resent SYN reaches a SYN_RCVD entry and fails that handshake on the server (the listen
    section's documented quirk); the client runs out of SYNs;
  * a lost handshake ACK: the client is established, the server's entry times out; its resent SYN+ACKs are FORWARD frames
    for the client.
At the end the two sides' ready records agree for every established pair, and for a few pairs a data segment cut by
dk_tcp_tx_segment from the client's rows is DELIVERED by dk_tcp_rx_process on the server's rows."""
import errno

import numpy as np
import pytest

import tcp_listen_cases as LC
from demikernel_amd import Config, FrameBatch, RxEngine, SocketId, flow_array, ipv4, synth
from demikernel_amd import _native as N
from demikernel_amd import tcp_connect as TC
from demikernel_amd import tcp_listen as TL
from demikernel_amd.tcp import TcpOut, TcpReceiver
from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults
from test_gpu_tcp_connect import Device as Client
from test_gpu_tcp_listen import Device as Server

pytestmark = pytest.mark.gpu

NC = 200
ALICE, BOB = synth.ALICE_IPV4, LC.BOB
PORTS = [80, 443]
TIMEOUT = 1_000_000


class Wire:
    """Frames that stay on the device: a FrameBatch over the sender's output blob with the lost indices left out, and
    the connector each frame belongs to (from the sender's own result arrays)."""

    def __init__(self, out, got, keep, who):
        import torch

        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).cuda()  # noqa: E731
        self.batch = FrameBatch(out, up(got["off_out"][keep], np.int32), up(got["len_out"][keep], np.int16))
        self.who = [who[j] for j in keep]

    def __len__(self):
        return len(self.who)


def through(eng, wire):
    rx = eng.results(len(wire), tcp_fields=True, tcp_opts=True)
    eng.receive_batch(wire.batch, rx)
    return rx


def test_device_clients_connect_to_device_listeners():
    import torch

    lport = [PORTS[c % 2] for c in range(NC)]
    cflows = flow_array([SocketId.Active((ALICE, 30000 + c), (BOB, lport[c])) for c in range(NC)])
    rows = TC.connector_table(NC, flow_id=np.arange(NC), local_ip=ipv4(ALICE), local_port=30000 + np.arange(NC),
                              remote_ip=LC.BOB_IP, remote_port=np.array(lport), handshake_retries=3,
                              handshake_timeout_ns=TIMEOUT, window_scale=np.arange(NC) % 9,
                              receive_window_size=np.where(np.arange(NC) % 4 == 0, 4000, 0xFFFF),
                              advertised_mss=1400 + np.arange(NC) % 5)
    cl = Client(cflows, rows, TC.conn_of_flow(NC, rows), nonce=0x5EED5EED, counter=0xFFA0, local=ALICE)
    sflows, L, lsn = LC.server(PORTS, max_backlog=[128, 128], handshake_retries=2, handshake_timeout_ns=TIMEOUT,
                               window_scale=[3, 0], nonce=[0xA1B2C3D4, 99], advertised_mss=[1450, 900],
                               receive_window_size=[0xFFFF, 1234])
    srv = Server(sflows, L, lsn, cap=512)
    lost_syn = {c for c in range(NC) if c % 10 == 1}
    lost_synack = {c for c in range(NC) if c % 20 == 2}
    lost_ack = {c for c in range(NC) if c % 25 == 3}
    lost = {("syn", c) for c in lost_syn} | {("synack", c) for c in lost_synack} | {("ack", c) for c in lost_ack}
    now = {"c": 10_000_000, "s": 50_000_000}  # the two clocks
    held, cready, sready = {}, [], []
    try:
        for d, key in ((cl, "c"), (srv, "s")):  # keep each call's output blob on the device
            def keep_out(*a, _orig=d._out, _key=key):
                held[_key] = _orig(*a)
                return held[_key]

            d._out = keep_out
        cl.receive = lambda w: through(cl.eng, w)
        srv.receive = lambda w: (through(srv.eng, w), w.batch)

        def wire_of(side, got, who, kinds):
            """The call's frames as the other side's batch; each (kind, connector) in `lost` is lost once."""
            keep = []
            for j in range(got["n_frames"]):
                k = (kinds[int(got["len_out"][j])], who[j])
                if k in lost:
                    lost.discard(k)
                else:
                    keep.append(j)
            return Wire(held[side], got, keep, who)

        def to_server(w):
            if not len(w):
                return w
            got, exp = srv.process(w, now["s"])
            sready.extend(got["ready"][:got["n_ready"]])
            who = [w.who[i] for i in got["frame_seg"][:got["n_frames"]]]
            return wire_of("s", got, who, {TL.SYNACK_BYTES: "synack", TL.RST_BYTES: "rst"})

        def to_client(w):
            if not len(w):
                return w
            got, exp = cl.process(w, now["c"])
            cready.extend(got["ready"][:got["n_ready"]])
            who = [w.who[i] for i in got["frame_seg"][:got["n_frames"]]]
            return wire_of("c", got, who, {TC.SYN_BYTES: "syn", TC.ACK_BYTES: "ack"})

        def pump(w):
            """From the client's frames until the wire is quiet."""
            while len(w):
                w = to_client(to_server(w))

        got, exp = cl.start(list(range(NC)), now["c"])
        assert got["n_frames"] == NC
        pump(wire_of("c", got, list(got["frame_seg"][:NC]), {TC.SYN_BYTES: "syn"}))
        assert not any(k[0] != "syn" for k in lost) and len(cready) == NC - len(lost_syn | lost_synack)
        for _ in range(4):
            now["c"] += TIMEOUT  # the client's timer first: a resent SYN finds the server's entry still in SYN_RCVD
            got, exp = cl.timers(now["c"], max_frames=NC, max_ready=NC)
            cready.extend(got["ready"][:got["n_ready"]])
            pump(wire_of("c", got, list(got["frame_seg"][:got["n_frames"]]), {TC.SYN_BYTES: "syn"}))
            now["s"] += TIMEOUT
            got, exp, _ = srv.timers(now["s"], max_frames=NC, max_ready=NC)
            sready.extend(got["ready"][:got["n_ready"]])
            trows = srv.table.rows()
            who = [TL.key_fields(int(trows[s]["key"]))[2] - 30000 for s in got["frame_seg"][:got["n_frames"]]]
            pump(to_client(wire_of("s", got, who, {TL.SYNACK_BYTES: "synack"})))
        assert not lost
        got, exp = cl.timers(now["c"] + 10 * TIMEOUT)
        assert (got["n_frames"], got["n_ready"]) == (0, 0)  # nothing is left connecting

        # what became of the two sides
        cby = {int(y["row"]): y for y in cready}
        sby = {int(y["remote_port"]) - 30000: y for y in sready}
        assert len(cby) == len(cready) == NC and len(sby) == len(sready) == NC
        cfail = {c for c, y in cby.items() if y["err"]}
        assert cfail == lost_synack and all(int(cby[c]["cause"]) == TC.CAUSE_EXHAUSTED for c in cfail)
        assert {c for c, y in sby.items() if y["err"] == errno.EBADMSG} == lost_synack  # the resent SYN failed them
        assert {c for c, y in sby.items() if y["err"] == errno.ETIMEDOUT} == lost_ack
        states = cl.model.rows["state"]
        assert all(int(states[c]) == (TC.FAILED if c in lost_synack else TC.ESTAB) for c in range(NC))
        pairs = [c for c in range(NC) if c not in lost_synack | lost_ack]
        assert len(pairs) == NC - 10 - 8 and all(sby[c]["err"] == 0 for c in pairs)
        for c in pairs:
            y, z, l = cby[c], sby[c], c % 2
            assert (int(y["snd_nxt"]), int(y["rcv_nxt"])) == (int(z["rcv_nxt"]), int(z["snd_nxt"]))
            assert (int(y["local_window"]), int(y["remote_window"])) == (int(z["remote_window"]), int(z["local_window"]))
            assert (int(y["local_wscale"]), int(y["remote_wscale"])) == (int(z["remote_wscale"]), int(z["local_wscale"]))
            assert int(y["local_window"]) == int(rows[c]["receive_window_size"]) << int(rows[c]["window_scale"])
            assert int(z["local_window"]) == int(L[l]["receive_window_size"]) << int(L[l]["window_scale"])
            assert (int(y["mss"]), int(z["mss"])) == (int(L[l]["advertised_mss"]), int(rows[c]["advertised_mss"]))

        # a few pairs go on: the client's first data segment is DELIVERED on the server's rows
        pick = pairs[:3] + pairs[-3:]
        txrows = np.concatenate([TC.conn_rows_from_connect_ready(cby[c], cl.model.rows[c])[1] for c in pick])
        rxrows = np.concatenate([TL.conn_rows_from_ready(sby[c], srv.model.listeners[c % 2])[0] for c in pick])
        snd, tcp = TcpSender(0), TcpReceiver(0)
        srv2 = RxEngine(Config(BOB), device=0)
        try:
            srv2.set_sockets(flow_array([SocketId.Active((BOB, lport[c]), (ALICE, 30000 + c)) for c in pick]))
            k = len(pick)
            src = torch.arange(10 * k, dtype=torch.uint8, device="cuda:0")
            push = PushList.from_numpy(np.arange(k), 10 * np.arange(k), np.full(k, 10))
            out = torch.zeros(k * 1536, dtype=torch.uint8, device="cuda:0")  # a slot holds 54 + mss bytes
            res = TcpTxResults(k, k)
            batch = snd.segment_batch(src, push, snd.conns_to_device(txrows), cl.d_links, out, res, slot_stride=1536)
            assert batch.n == k
            rx = srv2.results(k, tcp_fields=True)
            srv2.receive_batch(batch, rx)
            conns = tcp.conns_to_device(rxrows)
            o = TcpOut(k, k)
            tcp.process(rx, conns, o)
            torch.cuda.synchronize()
            assert list(o.to_numpy()["action"]) == [N.A["DELIVERED"]] * k
            after = tcp.conns_to_host(conns)
            assert all(int(after["receive_next"][j]) == (int(cby[c]["snd_nxt"]) + 10) & 0xFFFFFFFF for j, c in enumerate(pick))
        finally:
            snd.close()
            tcp.close()
            srv2.close()
    finally:
        cl.close()
        srv.close()
