"""tests/tcp_connect_reference.py pinned on the CPU: the reference's three connect scripts
(network_simulator/input/tcp/connect/*.pkt, their packet lines quoted below, replayed with the zero ISN generator of the
reference's test build), every SYN's and ACK's bytes against an independent frame builder (tests/frames.py), and the
receive oracle parsing every frame back as DK_V_OK_TCP with the fields that went in."""
import errno

import numpy as np
import pytest

import frames as F
import tcp_connect_cases as C
import tcp_connect_reference as R
from demikernel_amd import SocketId, flow_array, ipv4_str
from demikernel_amd import _native as N
from demikernel_amd import tcp_connect as TC
from test_tcp_listen_model import parse_line

KW = dict(slot_stride=64, max_frames=1024, out_bytes=1 << 20, max_ready=1024)
TIMEOUT = 3_000_000_000

# (file, packet lines in order; "+3": the handshake timer fires, three seconds after the line before)
SCRIPTS = {
    "connect-blocking.pkt": [
        "TCP > S seq 0(0) win 65535 <mss 1450, wscale 0>",
        "TCP < S. seq 0(0) ack 1 win 65535 <mss 1450, wscale 0>",
        "TCP > . seq 1(0) ack 1 win 65535 <nop>"],
    "connect-early-reset.pkt": [
        "TCP > S seq 0(0) win 65535 <mss 1450, wscale 0>",
        "TCP < R. seq 0(0) ack 1 win 65535 <mss 1450, wscale 0>"],
    "connect-refused.pkt": [
        "TCP > S seq 0(0) win 65535 <mss 1450, wscale 0>",
        "+3", "TCP > S seq 0(0) win 65535 <mss 1450, wscale 0>",
        "+3", "TCP > S seq 0(0) win 65535 <mss 1450, wscale 0>",
        "+3", "TCP > S seq 0(0) win 65535 <mss 1450, wscale 0>",
        "+3", "TCP > S seq 0(0) win 65535 <mss 1450, wscale 0>",
        "+3"],
}
WAIT = {"connect-blocking.pkt": 0, "connect-early-reset.pkt": errno.ECONNREFUSED, "connect-refused.pkt": errno.ECONNREFUSED}


def server_view(frames_list, k: int = 0):
    """The client's frames as server k's receive path parses them (the receive oracle with the server's address)."""
    from oracle.oracle import OraclePeer

    s = C.server(k)
    blob, off, lens = F.pack(frames_list)
    peer = OraclePeer(s[0])
    peer.set_flows(flow_array([SocketId.Active((ipv4_str(s[0]), s[1]), (C.BOB, C.lport(k)))]))
    return peer.process(blob, off, lens)


def check_sent(frames_list, want_lines, name):
    assert len(frames_list) == len(want_lines), name
    if not want_lines:
        return
    got = server_view(frames_list)
    for j, w in enumerate(want_lines):
        assert got["meta"][j] & 0xFF == N.V["OK_TCP"] and got["flow_id"][j] == 0
        assert (got["meta"][j] >> 16) & 0xFF == w["flags"], (name, hex(got["meta"][j]))
        assert (got["tcp_seq"][j], got["tcp_ack"][j]) == (w["seq"], w["ack"]), name
        assert got["tcp_win"][j] & 0xFFFF == w["win"] and got["payload"][j] >> 16 == 0, name
        rec = got["tcp_opts"][j]
        opts = [(int(o["kind"]), int(o["u16"]) or int(o["u8"])) for o in rec["opt"][:rec["num"]]]
        if w["flags"] & R.SYN:
            assert opts == [(N.DK_TCPOPT_MSS, 1450), (N.DK_TCPOPT_WS, 0)]
        else:
            assert got["meta"][j] >> 28 == 5  # "<nop>": the reference writes no option at all


def script_run(name):
    """Replays a script: yields ("start" | "frame" | "timer", argument, expected lines out)."""
    lines = [l if l == "+3" else parse_line(l.replace(", ", ",")) for l in SCRIPTS[name]]
    steps, k = [], 0
    while k < len(lines):
        ln = lines[k]
        if k == 0:
            step = ["start", None]
        elif ln == "+3":
            step = ["timer", None]
            k += 1
        else:
            assert ln["dir"] == "<"
            step = ["frame", ln]
            k += 1
        want = []
        while k < len(lines) and lines[k] != "+3" and lines[k]["dir"] == ">":
            want.append(lines[k])
            k += 1
        steps.append(step + [want])
    return steps


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_connect_script(name):
    flows, rows, cmap = C.client(1, extra_flows=())
    m = R.ConnectModel(rows, isn=R.zero_isn)
    now, ready, sent = 0, [], 0
    for what, ln, want in script_run(name):
        if what == "start":
            out = m.start([0], now, C.LINKS, **KW)
        elif what == "timer":
            now += TIMEOUT
            assert m.timers(now - 1, C.LINKS, **KW)["n_frames"] == 0  # not before the deadline
            out = m.timers(now, C.LINKS, **KW)
        else:
            fr = C.seg(0, ln["flags"], seq=ln["seq"], ack=ln["ack"], win=ln["win"], options=ln["opts"])
            out = m.process(C.oracle_rx([fr], flows), cmap, now, C.LINKS, **KW)
        check_sent(out["frames"], want, name)
        sent += len(out["frames"])
        ready += list(out["ready"])
    assert len(ready) == 1 and ready[0]["err"] == WAIT[name] and ready[0]["row"] == 0
    if name == "connect-blocking.pkt":
        assert (ready[0]["rcv_nxt"], ready[0]["snd_nxt"], ready[0]["mss"]) == (1, 1, 1450)
        assert (ready[0]["local_window"], ready[0]["remote_window"]) == (65535, 65535)
        assert m.rows[0]["state"] == TC.ESTAB and m.rows[0]["syns_left"] == 4
    elif name == "connect-early-reset.pkt":
        assert ready[0]["cause"] == TC.CAUSE_RST and m.rows[0]["state"] == TC.FAILED
    else:
        assert sent == 5 and ready[0]["cause"] == TC.CAUSE_EXHAUSTED  # handshake_retries = 5: five SYNs in all
        assert m.rows[0]["state"] == TC.FAILED and m.rows[0]["err"] == errno.ECONNREFUSED


def _run_mixed():
    flows, rows, cmap, nonce, counter, patch, frames = C.mixed_batch()
    m = C.started(rows, nonce, counter, which=range(140))
    for r, st in patch.items():
        m.rows[r]["state"] = st
    rx = C.oracle_rx(frames, flows)
    before = m.rows.copy()
    out = m.process(rx, cmap, C.NOW, C.LINKS, **KW)
    return flows, cmap, frames, rx, before, out, m


def test_mixed_batch_reaches_every_action_and_state():
    flows, cmap, frames, rx, before, out, m = _run_mixed()
    assert 290 <= len(frames) <= 310 and len(before) == 150
    assert set(int(a) for a in out["action"]) == set(range(7))
    assert set(int(s) for s in m.rows["state"]) == set(range(5))
    verdicts = set(int(v) & 0xFF for v in rx["meta"])
    assert {N.V["OK_UDP"], N.V["TCP_CSUM"], N.V["TCP_NOSOCK"]} <= verdicts
    assert (out["action"][(rx["meta"] & 0xFF) != N.V["OK_TCP"]] == TC.SKIP).all()
    causes = {(int(y["err"]), int(y["cause"])) for y in out["ready"]}
    assert causes == {(0, 0), (errno.ECONNREFUSED, TC.CAUSE_RST), (errno.ECONNREFUSED, TC.CAUSE_EXHAUSTED)}
    # the rule order, by the case builder's kinds
    first = {}
    for i, r in enumerate(out["row"]):
        first.setdefault(int(r), int(out["action"][i]))
    assert first[2] == TC.RETRY_SYN and first[3] == TC.REFUSED and first[14] == TC.RETRY_SYN and first[5] == TC.ESTABLISHED
    assert first[4] == TC.EXHAUSTED  # its one SYN was the first: the stray segment ends the loop
    assert first[0] == TC.ESTABLISHED and first[1] == TC.REFUSED
    # a frame at a time gives what the batch gives
    m1 = R.ConnectModel(before)
    acts, sent, rec = [], [], []
    for fr in frames:
        o = m1.process(C.oracle_rx([fr], flows), cmap, C.NOW, C.LINKS, **KW)
        acts.append(int(o["action"][0]))
        sent += o["frames"]
        rec += [(int(y["row"]), int(y["err"]), int(y["cause"])) for y in o["ready"]]
    assert acts == [int(a) for a in out["action"]] and sent == out["frames"]
    assert rec == [(int(y["row"]), int(y["err"]), int(y["cause"])) for y in out["ready"]]
    assert m1.rows.tobytes() == m.rows.tobytes()


def test_frame_bytes_against_an_independent_builder_and_parse_back():
    flows, cmap, frames, rx, before, out, m = _run_mixed()
    assert len(out["frames"]) > 40
    for f, fr in enumerate(out["frames"]):
        i = out["frame_seg"][f]
        r = int(out["row"][i])
        row, act = before[r], int(out["action"][i])
        link = C.LINKS[int(row["link"])]
        if act == TC.RETRY_SYN:
            flags, seq, ack = R.SYN, int(row["local_isn"]), 0
            opts = bytes([2, 4]) + int(row["advertised_mss"]).to_bytes(2, "big") + bytes([3, 3, int(row["window_scale"])])
            assert len(fr) == TC.SYN_BYTES
        else:
            assert act == TC.ESTABLISHED and len(fr) == TC.ACK_BYTES
            flags, seq, ack, opts = R.ACK, int(row["local_isn"]) + 1, int(rx["tcp_seq"][i]) + 1, b""
        ipw = int(row["ip_word"])
        want = F.tcp_frame(src=int(row["local_ip"]), dst=int(row["remote_ip"]), options=opts, sport=int(row["local_port"]),
                           dport=int(row["remote_port"]), ttl=(ipw >> 16) & 0xFF, ident=ipw & 0xFFFF,
                           dscp=ipw >> 26, ecn=(ipw >> 24) & 3,
                           tcp_kw=dict(seq=seq & R.M32, ack=ack & R.M32, flags=flags, window=int(row["receive_window_size"])))
        want = bytes(link["dst_mac"]) + bytes(link["src_mac"]) + want[12:]
        assert fr == want, (f, i, TC.ACTIONS[act])
        got = server_view([fr], r)
        assert got["meta"][0] & 0xFF == N.V["OK_TCP"] and (got["meta"][0] >> 16) & 0xFF == flags
        assert (got["tcp_seq"][0], got["tcp_ack"][0]) == (seq & R.M32, ack & R.M32)
        assert got["tcp_win"][0] == row["receive_window_size"] and got["payload"][0] >> 16 == 0
        assert got["src_ip"][0] == row["local_ip"]


def test_negotiation():
    flows, rows, cmap = C.client(4, extra_flows=(), window_scale=[14, 3, 3, 14], receive_window_size=[65535, 100, 100, 65535])
    m = C.started(rows, isn=R.zero_isn)
    fr = [C.seg(0, R.SYN | R.ACK, seq=9, ack=1, win=65535, options=bytes([3, 3, 14])),
          C.seg(1, R.SYN | R.ACK, seq=9, ack=1, win=7),                                   # no option at all
          C.seg(2, R.SYN | R.ACK, seq=9, ack=1, win=7, options=bytes([3, 3, 15])),        # 15 is taken as 14
          C.seg(3, R.SYN | R.ACK, seq=0xFFFFFFFF, ack=1, win=2, options=bytes([2, 4, 1, 0, 2, 4, 2, 0]))]  # the last MSS wins
    out = m.process(C.oracle_rx(fr, flows), cmap, 0, C.LINKS, **KW)
    y = out["ready"]
    assert [(int(r["mss"]), int(r["local_wscale"]), int(r["remote_wscale"])) for r in y] == \
        [(536, 14, 14), (536, 0, 0), (536, 3, 14), (512, 0, 0)]
    assert [(int(r["local_window"]), int(r["remote_window"])) for r in y] == \
        [(65535 << 14, 65535 << 14), (100, 7), (800, 7 << 14), (65535, 2)]
    assert int(y[3]["rcv_nxt"]) == 0 and all(int(r["snd_nxt"]) == 1 for r in y)


def test_stray_segments_cost_retries_and_budget_edges():
    """The reference's quirk: every EAGAIN takes a pass of the loop. An accept after k EAGAINs succeeds with k up to
    syns_left and fails one past it."""
    for syns_left, k, ok in ((0, 0, True), (0, 1, False), (1, 1, True), (1, 2, False), (3, 3, True), (3, 4, False)):
        flows, rows, cmap = C.client(1, extra_flows=(), handshake_retries=syns_left + 1)
        m = C.started(rows, isn=R.zero_isn)
        fr = [C.seg(0, R.ACK, ack=5)] * k + [C.seg(0, R.SYN | R.ACK, ack=1), C.seg(0, R.ACK | R.PSH, ack=1, payload=b"z")]
        out = m.process(C.oracle_rx(fr, flows), cmap, 7, C.LINKS, **KW)
        acts = [int(a) for a in out["action"]]
        if ok:
            assert acts == [TC.RETRY_SYN] * k + [TC.ESTABLISHED, TC.FORWARD]
            assert m.rows[0]["syns_left"] == syns_left - k
        else:
            assert acts == [TC.RETRY_SYN] * syns_left + [TC.EXHAUSTED] + [TC.ORPHANED] * (k - syns_left - 1 + 2)
            assert m.rows[0]["state"] == TC.FAILED
        assert m.rows[0]["deadline_ns"] == (7 + TIMEOUT if min(k, syns_left) else C.NOW - 10 + TIMEOUT)


def test_start_counter_duplicates_and_checks():
    flows, rows, cmap = C.client(8, window_scale=[0, 15, 0, 0, 0, 0, 0, 0], link=[0, 0, 9, 0, 0, 0, 0, 0],
                                 handshake_retries=[5, 5, 5, 0, 1, 5, 5, 5])
    rows["state"][5] = TC.CLOSED
    m = R.ConnectModel(rows, nonce=0xABCD, counter=0xFFFE)
    start = [0, 1, 2, 99, 3, 0, 4, 5, 6]
    out = m.start(start, 100, C.LINKS, **KW)
    assert list(out["status"]) == [TC.OK, TC.E_WSCALE, TC.E_LINK, TC.E_ROW, TC.OK, TC.E_STATE, TC.OK, TC.E_STATE, TC.OK]
    assert m.counter == (0xFFFE + len(start)) & 0xFFFF and out["frame_seg"] == [0, 6, 8]
    for k, r in ((0, 0), (4, 3), (6, 4), (8, 6)):  # entry k's counter value, whatever became of the entries before it
        assert m.rows[r]["local_isn"] == R.crc_isn(rows[r], 0xABCD, 0xFFFE + k)
    assert [int(s) for s in m.rows["state"]] == [TC.CONNECTING, TC.IDLE, TC.IDLE, TC.FAILED, TC.CONNECTING, TC.CLOSED,
                                                 TC.CONNECTING, TC.IDLE]
    assert [int(m.rows[r]["syns_left"]) for r in (0, 3, 4)] == [4, 0, 0]
    assert len(out["ready"]) == 1 and (int(out["ready"][0]["row"]), int(out["ready"][0]["frame"])) == (3, 4)
    assert int(out["ready"][0]["cause"]) == TC.CAUSE_EXHAUSTED
    assert m.rows[1].tobytes() == rows[1].tobytes() and m.rows[2].tobytes() == rows[2].tobytes()
    out = m.start([7], 100, C.LINKS, slot_stride=61, max_frames=4, out_bytes=1000, max_ready=4)
    assert list(out["status"]) == [TC.E_SLOT] and m.rows[7]["state"] == TC.IDLE
    crc = C.find_row_with_big_crc(rows, 0xABCD)
    m = R.ConnectModel(rows, nonce=0xABCD, counter=0xFFFF)
    m.start([0], 0, C.LINKS, **KW)
    assert m.rows[0]["local_isn"] == (crc + 0xFFFF) & R.M32 < 0xFFFF  # crc + counter wrapped 2^32


def test_offload_and_capacity():
    flows, rows, cmap = C.client(3, extra_flows=(), handshake_retries=[5, 5, 0])
    plain = R.ConnectModel(rows).start([0], 0, C.LINKS, **KW)["frames"][0]
    off = R.ConnectModel(rows).start([0], 0, C.LINKS, flags=N.DK_TX_OFFLOAD_TCP, **KW)["frames"][0]
    assert off[50:52] == b"\0\0" != plain[50:52] and plain[:50] == off[:50] and plain[52:] == off[52:]
    for short in ("max_frames", "out_bytes", "max_ready"):
        m = R.ConnectModel(rows, counter=9)
        kw = dict(KW, max_frames=2, out_bytes=128, max_ready=1)
        kw[short] -= 1
        o = m.start([0, 1, 2], 0, C.LINKS, **kw)
        assert not o["fits"] and (o["n_frames"], o["n_ready"]) == (2, 1) and set(o["status"]) == {TC.NO_ROOM}
        assert m.rows.tobytes() == rows.tobytes() and m.counter == 9
        kw[short] += 1
        assert m.start([0, 1, 2], 0, C.LINKS, **kw)["fits"] and m.counter == 12
