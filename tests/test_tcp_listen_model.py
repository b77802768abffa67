"""tests/tcp_listen_reference.py pinned on the CPU: the reference's nine accept scripts
(network_simulator/input/tcp/accept/*.pkt, their packet lines quoted below, replayed with the zero ISN generator of the
reference's test build), the CRC's catalogue check value against a bit-by-bit implementation, every reply's bytes
against an independent frame builder (tests/frames.py) and tests/tx_reference.py, and the receive oracle parsing every
reply back as DK_V_OK_TCP with the fields that went in."""
import errno
import re

import numpy as np
import pytest

import frames as F
import tcp_listen_cases as C
import tcp_listen_reference as R
import tx_reference as TR
from demikernel_amd import SocketId, flow_array, ipv4_str
from demikernel_amd import _native as N
from demikernel_amd import tcp_listen as TL

PORT = 80
REM = C.remote(1)
KW = dict(slot_stride=64, max_frames=1024, out_bytes=1 << 20, max_ready=1024)

# ---- the accept scripts: (file, packet lines in order; "timeout" = the handshake timer fires between two lines) --------
SCRIPTS = {
    "accept-blocking-1.pkt": [
        "TCP < S seq 0(0) win 65535 <mss 1450,wscale 0>",
        "TCP > S. seq 0(0) ack 1 win 65535 <mss 1450,wscale 0>",
        "TCP < . seq 1(0) ack 1 win 65535 <nop>"],
    "accept-blocking-2.pkt": [
        "TCP < S seq 0(0) win 65535 <mss 1450,wscale 0>",
        "TCP > S. seq 0(0) ack 1 win 65535 <mss 1450,wscale 0>",
        "timeout",
        "TCP > S. seq 0(0) ack 1 win 65535 <mss 1450,wscale 0>",
        "TCP < . seq 1(0) ack 1 win 65535 <nop>"],
    "accept-refuse-1.pkt": [
        "TCP < . seq 0(0) ack 1 win 65535 <mss 1450,wscale 0>",
        "TCP > R. seq 1(0) ack 2 <nop>"],
    "accept-refuse-2.pkt": [
        "TCP < P seq 0(0) win 65535 <mss 1450,wscale 0>",
        "TCP > R. seq 0(0) ack 28 <nop>"],
    "accept-refuse-3.pkt": [
        "TCP < R seq 0(0) win 65535 <mss 1450,wscale 0>",
        "TCP > R. seq 0(0) ack 28 <nop>"],
    "accept-refuse-4.pkt": [
        "TCP < P. seq 0(0) win 65535 <mss 1450,wscale 0>",
        "TCP > R. seq 0(0) ack 1 <nop>"],
    "accept-refuse-5.pkt": [
        "TCP < R. seq 0(0) win 65535 <mss 1450,wscale 0>",
        "TCP > R. seq 0(0) ack 1 <nop>"],
    "accept-refuse-6.pkt": [
        "TCP < S. seq 0(0) win 65535 <mss 1450,wscale 0>",
        "TCP > R. seq 0(0) ack 1 <nop>"],
    "accept-syn-carrying-data.pkt": [
        "TCP < S seq 0(1000) win 65535 <mss 1450,wscale 0>",
        "TCP > S. seq 0(0) ack 1 win 65535 <mss 1450,wscale 0>",
        "TCP < . seq 1(0) ack 1 win 65535 <nop>"],
}
# every refuse script goes on with the same successful handshake
for _k, _v in SCRIPTS.items():
    if "refuse" in _k:
        _v += SCRIPTS["accept-blocking-1.pkt"]
FLAG_BITS = {"S": R.SYN, ".": R.ACK, "P": R.PSH, "R": R.RST, "F": R.FIN}


def parse_line(line: str) -> dict:
    m = re.fullmatch(r"TCP ([<>]) (\S+) seq (\d+)\((\d+)\)(?: ack (\d+))?(?: win (\d+))? <(.*)>", line)
    assert m, line
    flags = 0
    for ch in m.group(2):
        flags |= FLAG_BITS[ch]
    opts = b""
    for o in m.group(7).split(","):
        o = o.strip()
        if o == "nop":
            opts += bytes([1])
        elif o.startswith("mss"):
            opts += bytes([2, 4]) + int(o.split()[1]).to_bytes(2, "big")
        elif o.startswith("wscale"):
            opts += bytes([3, 3, int(o.split()[1])])
    return {"dir": m.group(1), "flags": flags, "seq": int(m.group(3)), "len": int(m.group(4)),
            "ack": int(m.group(5) or 0), "win": int(m.group(6) or 0), "opts": opts}


def client_view(frames_list, rem=REM, lport=PORT):
    """The replies as the remote's receive path parses them (the receive oracle with the remote's address)."""
    from oracle.oracle import OraclePeer

    blob, off, lens = F.pack(frames_list)
    peer = OraclePeer(rem[0])
    peer.set_flows(flow_array([SocketId.Active((ipv4_str(rem[0]), rem[1]), (C.BOB, lport))]))
    return peer.process(blob, off, lens)


def test_crc_check_value_and_bitwise():
    def bitwise(data: bytes) -> int:  # the catalogue's definition, a bit at a time over the message
        reg = 0
        for byte in data:
            for bit in range(7, -1, -1):
                top = (reg >> 31) & 1
                reg = ((reg << 1) & R.M32)
                if top ^ ((byte >> bit) & 1):
                    reg ^= 0x04C11DB7
        return reg ^ 0xFFFFFFFF

    assert bitwise(b"123456789") == 0x765E7680 == R.crc32_cksum(b"123456789")
    rng = np.random.default_rng(1)
    for _ in range(64):
        d = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        assert bitwise(d) == R.crc32_cksum(d)
    L = TL.listener_table(1, local_ip=C.BOB_IP, local_port=80, nonce=0x01020304)[0]
    b = R.isn_bytes(L, REM[0], REM[1])
    assert len(b) == 16 and b[4:6] == REM[1].to_bytes(2, "big") and b[10:12] == (80).to_bytes(2, "big")
    assert b[:4] == bytes(int(x) for x in ipv4_str(REM[0]).split(".")) and b[12:] == bytes([1, 2, 3, 4])


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_accept_script(name):
    flows, L, lsn = C.server([PORT], max_backlog=1)  # listen(500, 1)
    m = R.ListenModel(L, 64, isn=R.zero_isn)
    now = 0
    lines = [l if l == "timeout" else parse_line(l) for l in SCRIPTS[name]]
    k = 0
    ready = []
    while k < len(lines):
        ln = lines[k]
        if ln == "timeout":
            now += int(L[0]["handshake_timeout_ns"])
            out = m.timers(now, C.LINKS, **KW)
            k += 1
        else:
            assert ln["dir"] == "<"
            fr = C.seg(REM, PORT, ln["flags"], seq=ln["seq"], ack=ln["ack"], win=ln["win"], options=ln["opts"],
                       payload=b"d" * ln["len"])
            out = m.process(C.oracle_rx([fr], flows), lsn, now, C.LINKS, **KW)
            k += 1
        ready += list(out["ready"])
        want = []
        while k < len(lines) and lines[k] != "timeout" and lines[k]["dir"] == ">":
            want.append(lines[k])
            k += 1
        assert len(out["frames"]) == len(want), (name, k)
        if want:
            got = client_view(out["frames"])
            for j, w in enumerate(want):
                assert got["meta"][j] & 0xFF == N.V["OK_TCP"] and got["flow_id"][j] == 0
                assert (got["meta"][j] >> 16) & 0xFF == w["flags"], (name, k, hex(got["meta"][j]))
                assert (got["tcp_seq"][j], got["tcp_ack"][j]) == (w["seq"], w["ack"]), (name, k)
                assert got["tcp_win"][j] & 0xFFFF == w["win"], (name, k)
                opts = [(o["kind"], int(o["u16"]) or int(o["u8"])) for o in got["tcp_opts"][j]["opt"][:got["tcp_opts"][j]["num"]]]
                if w["flags"] & R.SYN:
                    assert opts == [(N.DK_TCPOPT_MSS, 1450), (N.DK_TCPOPT_WS, 0)] or opts == [(2, 1450), (3, 0)]
                else:
                    assert got["meta"][j] >> 28 == 5  # "<nop>": no option entry; the reference writes none at all
    # "wait(500, ...) = 0": the accept completes
    assert len(ready) == 1 and ready[0]["err"] == 0
    assert (ready[0]["rcv_nxt"], ready[0]["snd_nxt"], ready[0]["mss"]) == (1, 1, 1450)
    assert (ready[0]["local_window"], ready[0]["remote_window"]) == (65535, 65535)
    assert m.listeners[0]["inflight"] == 1 and m.listeners[0]["isn_counter"] == 0


def _run_mixed():
    flows, L, lsn, warm, frames = C.mixed_batch()
    m = R.ListenModel(L, 1024)
    w = m.process(C.oracle_rx(warm, flows), lsn, C.NOW - 10, C.LINKS, **KW)
    rx = C.oracle_rx(frames, flows)
    out = m.process(rx, lsn, C.NOW, C.LINKS, **KW)
    return flows, L, lsn, warm, frames, w, rx, out, m


def test_mixed_batch_reaches_every_action_and_state():
    *_, w, rx, out, m = _run_mixed()
    assert [int(x) for x in np.bincount(w["action"], minlength=9)][:5] == [0, 9, 3, 0, 2]
    seen = set(int(a) for a in out["action"])
    assert seen == set(range(9)), sorted(seen)
    assert {e["state"] for e in m.conns.values()} == {TL.SYN_RCVD, TL.ESTAB, TL.FAILED}
    verdicts = set(int(v) & 0xFF for v in rx["meta"])
    assert {N.V["OK_UDP"], N.V["TCP_CSUM"], N.V["TCP_NOSOCK"]} <= verdicts
    assert (out["action"][(rx["meta"] & 0xFF) != 0] == TL.SKIP).all()
    errs = [int(r["err"]) for r in out["ready"]]
    assert errno.EBADMSG in errs and 0 in errs
    # a frame at a time gives what the batch gives
    flows, L, lsn, warm, frames, *_ = _run_mixed()
    m1 = R.ListenModel(L, 1024)
    m1.process(C.oracle_rx(warm, flows), lsn, C.NOW - 10, C.LINKS, **KW)
    acts, reps = [], []
    for fr in frames:
        o = m1.process(C.oracle_rx([fr], flows), lsn, C.NOW, C.LINKS, **KW)
        acts.append(int(o["action"][0]))
        reps += o["frames"]
    assert acts == [int(a) for a in out["action"]] and reps == out["frames"]
    assert m1.conns == m.conns and m1.listeners.tobytes() == m.listeners.tobytes()


def test_reply_bytes_against_an_independent_builder_and_parse_back():
    flows, L, lsn, warm, frames, w, rx, out, m = _run_mixed()
    assert len(out["frames"]) > 60
    for f, fr in enumerate(out["frames"]):
        i = out["frame_seg"][f]
        l = int(lsn[rx["flow_id"][i]])
        row = L[l]
        rem = (int(rx["src_ip"][i]), int(rx["ports"][i]) & 0xFFFF)
        act = int(out["action"][i])
        link = C.LINKS[int(row["link"])]
        if act == TL.SYN_ACCEPTED:
            e = m.conns[TL.key(l, *rem)]
            flags, seq, ack, win = R.SYN | R.ACK, e["local_isn"], e["remote_isn"] + 1, int(row["receive_window_size"])
            opts = bytes([2, 4]) + int(row["advertised_mss"]).to_bytes(2, "big") + bytes([3, 3, int(row["window_scale"])])
            assert len(fr) == TL.SYNACK_BYTES
        else:
            assert act in (TL.RST_FLAGS, TL.RST_BACKLOG) and len(fr) == TL.RST_BYTES
            flags, win, opts = R.RST | R.ACK, 0, b""
            if (int(rx["meta"][i]) >> 16) & R.ACK:
                seq, ack = int(rx["tcp_ack"][i]), int(rx["tcp_ack"][i]) + 1
            else:
                seq, ack = 0, int(rx["tcp_seq"][i]) + R.compute_size(rx, i)
        want = F.tcp_frame(src=int(row["local_ip"]), dst=rem[0], options=opts, sport=int(row["local_port"]), dport=rem[1],
                           tcp_kw=dict(seq=seq & R.M32, ack=ack & R.M32, flags=flags, window=win), ttl=255)
        want = bytes(link["dst_mac"]) + bytes(link["src_mac"]) + want[12:]
        assert fr == want, (f, i, TL.ACTIONS[act])
        # and tests/tx_reference.py from dk_tx_segs-packed fields, the form dk_tx_serialize is tested in
        rec = TR.opts_record([("mss", int(row["advertised_mss"])), ("ws", int(row["window_scale"]))]) if opts else None
        ob = TR.tcp_option_bytes(rec[0]) if opts else b""
        assert fr == TR.headers(b"", 6, int(row["local_ip"]), rem[0], int(row["local_port"]) | rem[1] << 16,
                                meta=flags << 16, seq=seq & R.M32, ack=ack & R.M32, winurg=win, options=ob,
                                dst_mac=bytes(link["dst_mac"]), src_mac=bytes(link["src_mac"]))
        got = client_view([fr], rem, int(row["local_port"]))
        assert got["meta"][0] & 0xFF == N.V["OK_TCP"] and (got["meta"][0] >> 16) & 0xFF == flags
        assert (got["tcp_seq"][0], got["tcp_ack"][0], got["tcp_win"][0]) == (seq & R.M32, ack & R.M32, win)
        assert got["payload"][0] >> 16 == 0 and got["src_ip"][0] == row["local_ip"]


def test_offload_writes_a_zero_checksum():
    flows, L, lsn = C.server([PORT])
    m = R.ListenModel(L, 64)
    out = m.process(C.oracle_rx([C.seg(REM, PORT, R.SYN, seq=5)], flows), lsn, 0, C.LINKS, flags=N.DK_TX_OFFLOAD_TCP, **KW)
    assert out["frames"][0][50:52] == b"\0\0"
    m = R.ListenModel(L, 64)
    plain = m.process(C.oracle_rx([C.seg(REM, PORT, R.SYN, seq=5)], flows), lsn, 0, C.LINKS, **KW)["frames"][0]
    assert plain[50:52] != b"\0\0" and plain[:50] == out["frames"][0][:50] and plain[52:] == out["frames"][0][52:]


def test_backlog_and_counter():
    flows, L, lsn = C.server([PORT, 81], max_backlog=[2, 1], isn_counter=[0xFFFE, 0])
    m = R.ListenModel(L, 64)
    fr = [C.seg(C.remote(k), PORT, R.SYN, seq=k) for k in range(4)] + [C.seg(C.remote(9), 81, R.SYN)] * 2
    fr.insert(3, C.seg(C.remote(0), PORT, R.SYN, seq=0))  # remote 0 again behind the point where the room ran out
    out = m.process(C.oracle_rx(fr, flows), lsn, 0, C.LINKS, **KW)
    A = TL
    assert [int(a) for a in out["action"]] == [A.SYN_ACCEPTED, A.SYN_ACCEPTED, A.RST_BACKLOG, A.BAD_ACK, A.RST_BACKLOG,
                                              A.SYN_ACCEPTED, A.BAD_ACK]
    assert [int(x) for x in m.listeners["inflight"]] == [2, 1] and int(m.listeners["isn_counter"][0]) == 0
    isns = [m.conns[TL.key(0, *C.remote(k))]["local_isn"] for k in range(2)]
    assert isns == [C.isn_of(L[0], C.remote(0), 0xFFFE), C.isn_of(L[0], C.remote(1), 0xFFFF)]
    rem = C.find_remote_with_big_crc(L[0])
    out = R.ListenModel(C.server([PORT], isn_counter=0xFFFF)[1], 64)
    o = out.process(C.oracle_rx([C.seg(rem, PORT, R.SYN)], flows), lsn, 0, C.LINKS, **KW)
    assert int(o["action"][0]) == TL.SYN_ACCEPTED
    assert out.conns[TL.key(0, *rem)]["local_isn"] < 0xFFFF  # crc + 0xFFFF wrapped 2^32


def test_capacity_is_all_or_nothing():
    flows, L, lsn, warm, frames, w, rx, out, m = _run_mixed()
    for short in ("max_frames", "out_bytes", "max_ready"):
        m2 = R.ListenModel(L, 1024)
        m2.process(C.oracle_rx(warm, flows), lsn, C.NOW - 10, C.LINKS, **KW)
        before = (dict(m2.conns), m2.listeners.tobytes())
        kw = dict(KW, max_frames=out["n_frames"], out_bytes=out["n_frames"] * 64, max_ready=out["n_ready"])
        kw[short] -= 1
        o = m2.process(rx, lsn, C.NOW, C.LINKS, **kw)
        assert not o["fits"] and (o["n_frames"], o["n_ready"]) == (out["n_frames"], out["n_ready"])
        assert (m2.conns, m2.listeners.tobytes()) == before and set(o["status"]) == {TL.NO_ROOM}
        kw[short] += 1
        assert m2.process(rx, lsn, C.NOW, C.LINKS, **kw)["fits"]
