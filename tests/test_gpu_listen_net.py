"""The passive open as a closed loop on the MI355X: about 200 host-modelled clients connect to listeners on the device.
No reply is built or parsed on the host: the device's SYN+ACKs and RSTs go through the receive engine again (a second
engine with the clients' address, as loopback), and the clients answer from what it parsed. Some SYN+ACKs are dropped,
so the handshake timer resends them; some clients never answer and end ETIMEDOUT. Every device call is compared whole
with the model (tests/test_gpu_tcp_listen.py's Device), the ready records at the end equal the model's, and for a few of
them the connection's first data segment is DELIVERED by dk_tcp_rx_process on rows built from the ready record."""
import errno

import numpy as np
import pytest

import tcp_listen_cases as C
import tcp_listen_reference as R
from demikernel_amd import Config, FrameBatch, RxEngine, SocketId, flow_array, ipv4, synth
from demikernel_amd import _native as N
from demikernel_amd import tcp_listen as TL
from demikernel_amd.tcp import TcpOut, TcpReceiver
from test_gpu_tcp_listen import Device, receive

pytestmark = pytest.mark.gpu

NCLIENTS = 200
ALICE = synth.ALICE_IPV4
PORTS = [80, 443]


def test_clients_connect_to_the_device():
    import torch

    rng = np.random.default_rng(11)
    timeout = 1_000_000
    flows, L, lsn = C.server(PORTS, max_backlog=[128, 90], handshake_retries=2, handshake_timeout_ns=timeout,
                             window_scale=[3, 0], nonce=[0xA1B2C3D4, 99])
    d = Device(flows, L, lsn, cap=512)
    clients = [(ipv4(ALICE), 30000 + c) for c in range(NCLIENTS)]
    lport = [PORTS[c % 2] for c in range(NCLIENTS)]
    # the clients' side of the wire: one engine that knows every client's connection
    ceng = RxEngine(Config(ALICE), device=0)
    ceng.set_sockets(flow_array([SocketId.Active((ALICE, clients[c][1]), (C.BOB, lport[c])) for c in range(NCLIENTS)]))
    silent = set(int(c) for c in rng.choice(NCLIENTS, 15, replace=False))     # never answer a SYN+ACK
    drops = {c: int(rng.integers(1, 3)) for c in range(NCLIENTS) if c % 6 == 0 and c not in silent}  # SYN+ACKs lost
    isn = [int(x) for x in rng.integers(0, 1 << 32, NCLIENTS)]
    opts = [bytes([2, 4, 5, 0xB4, 3, 3, c % 16]) if c % 3 else b"" for c in range(NCLIENTS)]
    state = ["closed"] * NCLIENTS
    ready_dev, ready_model = [], []
    now = 10_000_000
    try:
        def answer(got, nframes):
            """The replies through the clients' receive engine; the frames the clients send in return."""
            if nframes == 0:
                return []
            import torch as T

            u = lambda a, dt: T.from_numpy(np.ascontiguousarray(a).view(dt))  # noqa: E731
            batch = FrameBatch(d_out_holder[0], u(got["off_out"][:nframes], np.int32).cuda(),
                               u(got["len_out"][:nframes], np.int16).cuda())
            rx = ceng.results(nframes, tcp_fields=True, tcp_opts=True)
            ceng.receive_batch(batch, rx)
            T.cuda.synchronize()
            h = rx.to_numpy()
            back = []
            for j in range(nframes):
                assert h["meta"][j] & 0xFF == N.V["OK_TCP"], (j, h["meta"][j] & 0xFF)
                c = int(h["flow_id"][j])
                fl = (int(h["meta"][j]) >> 16) & 0xFF
                if fl & R.RST:
                    state[c] = "refused"
                    continue
                assert fl == R.SYN | R.ACK and int(h["tcp_ack"][j]) == (isn[c] + 1) & R.M32
                if c in silent:
                    continue
                if drops.get(c, 0) > 0:
                    drops[c] -= 1
                    continue
                if state[c] == "syn_sent":
                    state[c] = "established"
                    srv_isn[c] = int(h["tcp_seq"][j])
                    back.append(C.seg(clients[c], lport[c], R.ACK | (R.PSH if c % 5 == 0 else 0), seq=isn[c] + 1,
                                      ack=srv_isn[c] + 1, payload=b"hi" if c % 5 == 0 else b""))
            return back

        srv_isn = {}
        d_out_holder = [None]
        orig_out = d._out

        def keep_out(*a):
            d_out_holder[0] = orig_out(*a)
            return d_out_holder[0]

        d._out = keep_out

        def step_process(frames):
            got, exp = d.process(frames, now)
            ready_dev.extend(got["ready"][:got["n_ready"]])
            ready_model.extend(zip(exp["ready_keys"], exp["ready"]))
            return answer(got, got["n_frames"])

        def step_timers():
            got, exp, _ = d.timers(now, max_frames=NCLIENTS, max_ready=NCLIENTS)
            ready_dev.extend(got["ready"][:got["n_ready"]])
            ready_model.extend(zip(exp["ready_keys"], exp["ready"]))
            return answer(got, got["n_frames"])

        # the connection storm: every client's SYN in two batches, the second with stray frames of the first's clients
        syns = [C.seg(clients[c], lport[c], R.SYN, seq=isn[c], options=opts[c]) for c in range(NCLIENTS)]
        for c in range(NCLIENTS):
            state[c] = "syn_sent"
        pending = step_process(syns[:120])
        pending = step_process(syns[120:] + pending)
        for _ in range(5):  # the timers until every handshake is over
            now += timeout
            pending = step_timers() + pending
            if pending:
                pending = step_process(pending)
        assert not pending
        # what became of the clients
        ok = [c for c in range(NCLIENTS) if state[c] == "established"]
        refused = [c for c in range(NCLIENTS) if state[c] == "refused"]
        assert len(refused) == NCLIENTS // 2 - 90  # port 443's backlog is 90
        assert len(ok) >= 150 and any(drops.get(c) == 0 for c in ok)  # some were accepted after a resend
        byport = {int(r["remote_port"]): r for r in ready_dev}
        assert len(byport) == len(ready_dev) == len(ready_model)
        for k, e in ready_model:  # the device's records are the model's
            g = byport[TL.key_fields(k)[2]].copy()
            g["slot"] = 0
            assert g.tobytes() == e.tobytes()
        good = {p for p, r in byport.items() if r["err"] == 0}
        assert good == {clients[c][1] for c in ok}
        timed_out = {p for p, r in byport.items() if r["err"] == errno.ETIMEDOUT}
        assert timed_out == {clients[c][1] for c in silent if state[c] != "refused"} and len(timed_out) > 5
        # a few connections go on into the established state: the first data segment is DELIVERED
        pick = ok[:3] + ok[-3:]
        srv = RxEngine(Config(C.BOB), device=0)
        srv.set_sockets(flow_array([SocketId.Active((C.BOB, lport[c]), (ALICE, clients[c][1])) for c in pick]))
        rows = np.concatenate([TL.conn_rows_from_ready(byport[clients[c][1]], d.model.listeners[PORTS.index(lport[c])])[0]
                               for c in pick])
        data = [C.seg(clients[c], lport[c], R.ACK | R.PSH, seq=isn[c] + 1, ack=srv_isn[c] + 1, payload=b"first data")
                for c in pick]
        rx, _batch = receive(srv, data)
        tcp = TcpReceiver(0)
        try:
            conns = tcp.conns_to_device(rows)
            out = TcpOut(len(pick), len(pick))
            tcp.process(rx, conns, out)
            torch.cuda.synchronize()
            assert list(out.to_numpy()["action"]) == [N.A["DELIVERED"]] * len(pick)
            after = tcp.conns_to_host(conns)
            assert all(int(after["receive_next"][j]) == (isn[c] + 1 + 10) & R.M32 for j, c in enumerate(pick))
        finally:
            tcp.close()
            srv.close()
    finally:
        ceng.close()
        d.close()
