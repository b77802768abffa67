"""dk_tcp_ack_emit / dk_tcp_ack_timer on the CPU: tests/tcp_ackemit_reference.py, the restatement the GPU tests compare
against, pinned three ways, and the ABI additions against the C compiler. No GPU work.

  * against the oracle: on the crafted batches of tests/tcp_batches.py and every recorded call of tests/stream_net.py
    its own process_packet loop gives the oracle's actions, views and final table, which pins the RCV.NXT it puts into
    each ACK (it is the loop's own, read where the reference reads it);
  * by hand: one case per row of dk_tcp.h's table, with the expected ACKs (triggering frame, ack number, window) and
    `armed` written out literally;
  * frame validity: every frame it builds parses through the oracle's TcpHeader::parse_and_strip with its checksum
    verified, and carries the fields it was built from.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import stream_net as SN
import tcp_ackemit_reference as E
import tcp_batches as TB
from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_ackemit import dack_conn_table
from demikernel_amd.tcp_tx import tx_conn_table
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_tcp.h")
LINKS = np.zeros(1, N.TX_LINK_DTYPE)
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
NOW, DELAY = 7_000_000_123, 40_000_000
A = N.A


def run(rx, table, *, armed=0, tx=None, dack=None, **kw):
    nc = len(table)
    tx = tx_conn_table(nc, snd_nxt=table["send_next"]) if tx is None else tx
    dack = dack_conn_table(nc, delay_ns=DELAY, armed=armed, deadline_ns=99) if dack is None else dack
    n = len(rx["meta"])
    kw.setdefault("slot_stride", 64)
    kw.setdefault("max_frames", n)
    out = np.full(max(kw["max_frames"], 1) * kw["slot_stride"] + 16, 0xA5, np.uint8)
    return E.ack_emit(rx, table, tx, dack, LINKS, NOW, out, **kw)


def same_as_oracle(rx, table, got, ctx):
    t = np.ascontiguousarray(table, O.TCP_CONN_DTYPE).copy()
    exp = O.tcp_process(t, rx)
    assert np.array_equal(got["action"], exp["action"]), (ctx, np.nonzero(got["action"] != exp["action"])[0][:8])
    for k in ("ref", "off", "len"):
        assert np.array_equal(got["view"][k], exp["view"][k]), (ctx, k)
    assert got["rx_conns"].tobytes() == t.tobytes(), f"{ctx}: the final table"
    return exp


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TB.LAYOUTS)
def test_actions_views_and_table_on_crafted_batches(name):
    table, rx, f, stray = TB.case(name, 6000, 40, seed=3)
    got = run(rx, table, tx=tx_conn_table(40, snd_nxt=table["send_next"], rcv_wscale=14))  # 2^26 bytes of buffer
    exp = same_as_oracle(rx, table, got, name)
    # every stray is beyond the window: an ACK at once; the in-order segments ACK every second time
    act = exp["action"]
    acked = got["ack_frame"] != E.NO_FRAME
    assert acked[act == A["OUT_OF_WINDOW"]].all() and not acked[act == A["SKIP"]].any()
    assert got["n_frames"] == int(acked.sum()) == len(got["desc"])
    # an ACK's number is the RCV.NXT of its moment: 1 + 10 bytes per segment delivered before it on its row
    for c in np.unique(f[(f < 40)])[:8]:
        mine = np.nonzero(f == c)[0]
        rn = 1 + TB.PAYLOAD * np.cumsum(act[mine] == A["DELIVERED"])
        d = {i: a for i, cc, a, w in got["desc"] if cc == c}
        assert all(d[i] == rn[k] for k, i in enumerate(mine) if i in d)


@pytest.mark.parametrize("name", list(SN.CASES))
def test_actions_views_and_table_on_recorded_streams(name):
    tr = SN.trace(name)
    peer = O.OraclePeer(synth.ipv4(synth.BOB_IPV4))
    peer.set_flows(tr.flows)
    hist = np.zeros(13, np.int64)
    acks = 0
    for k, call in enumerate(tr.calls):
        rx = peer.process(call.blob, call.off, call.lens)
        tx = tx_conn_table(len(call.start), snd_nxt=call.start["send_next"], rcv_wscale=2)  # up to 64 KiB of buffer
        got = run(rx, call.start, armed=k & 1, tx=tx)
        assert np.array_equal(got["action"], call.exp["action"]), (name, k)
        for fld in ("ref", "off", "len"):
            assert np.array_equal(got["view"][fld], call.exp["view"][fld]), (name, k, fld)
        assert got["rx_conns"].tobytes() == call.exp_table.tobytes(), (name, k)
        hist += np.bincount(got["action"], minlength=13)
        acks += got["n_frames"]
        # no ACK is ahead of the table's final RCV.NXT, and a connection's ACK numbers never go back
        last = {}
        for i, c, rn, w in got["desc"]:
            assert ((int(call.exp_table["receive_next"][c]) - rn) & E.M32) < 1 << 31
            assert ((rn - last.get(c, rn)) & E.M32) < 1 << 31
            last[c] = rn
    assert acks > 0 and hist[A["DELIVERED"]] > 0 and hist[A["STORED"]] > 0
    if name == "strays":
        assert all(hist[A[k]] > 0 for k in ("RST", "SYN", "NO_ACK", "ACK_UNSENT", "UNPROCESSED", "FIN"))


# ---------------------------------------------------------------------------------------------------------------------
# 2. by hand: one connection at RCV.NXT 1000, reader caught up, SND.NXT 500
# ---------------------------------------------------------------------------------------------------------------------
def batch(segs):
    """segs: (seq, payload bytes, tcp flags, ack number[, flow]) -> the dk_rx result arrays."""
    n = len(segs)
    rx = {k: np.zeros(n, np.uint32) for k in ("meta", "flow_id", "tcp_seq", "tcp_ack", "payload")}
    for i, s in enumerate(segs):
        seq, ln, fl, ack = s[:4]
        rx["meta"][i] = 6 << 8 | fl << 16 | 0x50 << 24
        rx["flow_id"][i] = s[4] if len(s) > 4 else 0
        rx["tcp_seq"][i], rx["tcp_ack"][i], rx["payload"][i] = seq & E.M32, ack, 54 | ln << 16
    return rx


def hand(segs, armed, *, rn=1000, bufsz=4000, **kw):
    table = conn_table(1, receive_next=rn, send_next=500, buffer_size=bufsz)
    got = run(batch(segs), table, armed=armed, **kw)
    same_as_oracle(batch(segs), table, got, "hand")
    acks = [(i, a, w) for i, c, a, w in got["desc"]]
    return got, [N.TCP_ACTIONS[a] for a in got["action"]], acks, int(got["dack"]["armed"][0]), int(got["dack"]["deadline_ns"][0])


def test_delivered_toggles_and_mid_batch_ack_numbers():
    segs = [(1000 + 10 * k, 10, ACK | PSH, 500) for k in range(4)]
    got, act, acks, armed, deadline = hand(segs, 0)
    assert act == ["DELIVERED"] * 4
    # armed 0 -> 1 -> ACK -> 1 -> ACK: the first ACK carries 1020, not the batch's final 1040
    assert acks == [(1, 1020, 3980), (3, 1040, 3960)] and armed == 0 and deadline == NOW + DELAY
    assert got["ack_frame"].tolist() == [E.NO_FRAME, 0, E.NO_FRAME, 1] and got["n_acks"].tolist() == [2]
    got, act, acks, armed, deadline = hand(segs, 1)
    assert acks == [(0, 1010, 3990), (2, 1030, 3970)] and armed == 1 and deadline == NOW + DELAY
    got, act, acks, armed, deadline = hand(segs[:1], 1)
    assert acks == [(0, 1010, 3990)] and armed == 0 and deadline == 99  # cleared: the deadline stays as it was


def test_no_data_toggles():
    segs = [(1000, 0, ACK, 500)] * 3
    got, act, acks, armed, deadline = hand(segs, 0)
    assert act == ["NO_DATA"] * 3 and acks == [(1, 1000, 4000)] and armed == 1


def test_stored_acks_then_arms():
    hole = (1010, 10, ACK | PSH, 500)
    for armed0 in (0, 1):
        got, act, acks, armed, deadline = hand([hole], armed0)
        # send_ack clears the deadline, then the tail of process_packet finds it None and arms it
        assert act == ["STORED"] and acks == [(0, 1000, 4000)] and armed == 1 and deadline == NOW + DELAY
    segs = [hole, hole, (1000, 10, ACK | PSH, 500), (1020, 0, ACK, 500)]
    got, act, acks, armed, deadline = hand(segs, 0)
    assert act == ["STORED", "STORE_DUP", "DELIVERED", "NO_DATA"]
    # the segment that fills the hole finds armed 1 (the quirk) and ACKs past the recovered bytes
    assert acks == [(0, 1000, 4000), (1, 1000, 4000), (2, 1020, 3980)] and armed == 1


def test_duplicate_and_out_of_window():
    old, far = (900, 50, ACK | PSH, 500), (1000 + 4000, 10, ACK | PSH, 500)
    for seg, name in ((old, "DUPLICATE"), (far, "OUT_OF_WINDOW")):
        got, act, acks, armed, deadline = hand([seg], 1)
        assert act == [name] and acks == [(0, 1000, 4000)] and armed == 0 and deadline == 99
        got, act, acks, armed, deadline = hand([seg], 0)
        assert acks == [(0, 1000, 4000)] and armed == 0
        rst = (seg[0], seg[1], seg[2] | RST, seg[3])
        for armed0 in (0, 1):  # with RST set: no ACK, nothing changes
            got, act, acks, armed, deadline = hand([rst], armed0)
            assert act == [name] and acks == [] and armed == armed0 and deadline == 99
            assert got["dack"].tobytes() == dack_conn_table(1, delay_ns=DELAY, armed=armed0, deadline_ns=99).tobytes()
    # a stray between data: its ACK carries the RCV.NXT of its arrival
    segs = [(1000, 10, ACK | PSH, 500), far, (1010, 10, ACK | PSH, 500), old]
    got, act, acks, armed, deadline = hand(segs, 0)
    assert act == ["DELIVERED", "OUT_OF_WINDOW", "DELIVERED", "DUPLICATE"]
    assert acks == [(1, 1010, 3990), (3, 1020, 3980)] and armed == 0


def test_fin():
    segs = [(1000, 10, ACK | PSH | FIN, 500), (1011, 10, ACK, 500)]
    for armed0 in (0, 1):
        got, act, acks, armed, deadline = hand(segs, armed0)
        # after RCV.NXT moved over the FIN; the function returns before the toggle: never armed
        assert act == ["FIN", "UNPROCESSED"] and acks == [(0, 1011, 3989)] and armed == 0 and deadline == 99
    # an out-of-order FIN is stored (ACK, armed); the data that reaches it closes
    segs = [(1010, 0, ACK | FIN, 500), (1000, 10, ACK | PSH, 500)]
    got, act, acks, armed, deadline = hand(segs, 0)
    assert act == ["STORED", "FIN"] and acks == [(0, 1000, 4000), (1, 1011, 3989)] and armed == 0


def test_ack_unsent():
    got, act, acks, armed, deadline = hand([(1000, 10, ACK | PSH, 501)], 1)
    assert act == ["ACK_UNSENT"] and acks == [(0, 1000, 4000)] and armed == 0
    got, act, acks, armed, deadline = hand([(1000, 10, ACK | PSH, 501)], 0)
    assert acks == [(0, 1000, 4000)] and armed == 0 and deadline == 99


def test_rows_without_an_ack():
    segs = [(1000, 0, ACK | SYN, 500), (1000, 5, PSH, 500), (1000, 0, ACK | RST, 500), (1000, 5, ACK, 500),
            (1000, 5, ACK, 500, 7)]
    for armed0 in (0, 1):
        got, act, acks, armed, deadline = hand(segs, armed0)
        assert act == ["SYN", "NO_ACK", "RST", "UNPROCESSED", "SKIP"]
        assert acks == [] and armed == armed0 and deadline == 99 and got["n_frames"] == 0
        assert (got["out"] == 0xA5).all() and (got["ack_frame"] == E.NO_FRAME).all()


def test_window_closes_and_front_trims():
    # 100 bytes of buffer: 60 + 40 fill it; a retransmission that overlaps RCV.NXT is trimmed, a trimmed SYN counts one
    segs = [(1000, 60, ACK | PSH, 500), (1060, 40, ACK | PSH, 500), (1100, 0, ACK, 500), (1100, 0, ACK, 500)]
    got, act, acks, armed, deadline = hand(segs, 1, bufsz=100)
    assert act == ["DELIVERED", "DELIVERED", "NO_DATA", "NO_DATA"]
    assert acks == [(0, 1060, 40), (2, 1100, 0)] and armed == 1
    segs = [(990, 30, ACK | PSH, 500), (1010, 15, ACK | PSH, 500), (1024, 10, ACK | PSH | SYN, 500)]
    got, act, acks, armed, deadline = hand(segs, 1)
    assert act == ["DELIVERED"] * 3 and got["view"]["off"].tolist() == [64, 64, 54]
    assert acks == [(0, 1020, 3980), (2, 1035, 3965)]
    # through 2^32
    segs = [(0xFFFFFFF8 + 8 * k, 8, ACK | PSH, 500) for k in range(3)]
    got, act, acks, armed, deadline = hand(segs, 1, rn=0xFFFFFFF8)
    assert acks == [(0, 0, 3992), (2, 16, 3976)]


def test_connection_failures_capacity_and_timer():
    nc = 8
    table = conn_table(nc, receive_next=1000, send_next=500, buffer_size=4000)
    tx = tx_conn_table(nc, snd_nxt=500)
    tx["state"][1] = N.DK_TCP_CLOSED
    table["send_next"][2] = 499
    tx["link"][3] = 1
    tx["rcv_wscale"][4] = 15
    table["buffer_size"][5] = 1 << 16   # full open, it does not fit 16 bits at scale 0
    tx["state"][6], table["send_next"][6] = N.DK_TCP_NONE, 1  # E_STATE comes first
    tx["rcv_wscale"][7], table["buffer_size"][7] = 14, 0xFFFF << 14
    segs = [(1000 + 10 * k, 10, ACK | PSH, 500 if c != 2 else 499, c) for c in range(nc) for k in range(2)]
    got = run(batch(segs), table, armed=1, tx=tx)
    want = [E.OK, E.E_STATE, E.E_SND_NXT, E.E_LINK, E.E_WSCALE, E.E_WINDOW, E.E_STATE, E.OK]
    assert got["status"].tolist() == want and got["n_acks"].tolist() == [1, 0, 0, 0, 0, 0, 0, 1]
    assert got["frame_conn"].tolist() == [0, 7] and got["frame_seg"].tolist() == [0, 14]
    d0 = dack_conn_table(nc, delay_ns=DELAY, armed=1, deadline_ns=99)
    for c in range(1, 7):
        assert got["dack"][c].tobytes() == d0[c].tobytes()
    a = int(got["off_out"][1])
    assert int.from_bytes(got["out"][a + 48:a + 50].tobytes(), "big") == (0xFFFF << 14) - 10 >> 14
    slot = run(batch(segs), table, armed=1, tx=tx, frame_lead=11)
    assert slot["status"].tolist() == [E.E_SLOT, E.E_STATE, E.E_SND_NXT, E.E_LINK, E.E_WSCALE, E.E_WINDOW, E.E_STATE,
                                       E.E_SLOT] and slot["n_frames"] == 0
    for kw in (dict(max_frames=1), dict(max_frames=2, out_bytes=127)):
        short = run(batch(segs), table, armed=1, tx=tx, **kw)
        assert short["n_frames"] == 2 and (short["ack_frame"] == E.NO_FRAME).all() and (short["out"] == 0xA5).all()
        assert short["status"].tolist() == [E.NO_ROOM] + want[1:7] + [E.NO_ROOM] and short["dack"].tobytes() == d0.tobytes()
    # the timer: armed connections the host names send one ACK from the table as it stands
    fire = np.array([1, 1, 1, 1, 1, 1, 0, 1], np.uint8)
    dk = d0.copy()
    dk["armed"][7] = 0
    out = np.full(8 * 64, 0xA5, np.uint8)
    t = E.ack_timer(fire, tx, table, dk, LINKS, out, slot_stride=64, max_frames=8)
    assert t["status"].tolist() == [E.OK, E.E_STATE, E.E_SND_NXT, E.E_LINK, E.E_WSCALE, E.E_WINDOW, E.NOT_FIRED, E.IDLE]
    assert t["n_frames"] == 1 and t["ack_frame"].tolist() == [0] + [E.NO_FRAME] * 7
    assert t["dack"]["armed"].tolist() == [0, 1, 1, 1, 1, 1, 1, 0] and (t["dack"]["deadline_ns"] == 99).all()
    assert int.from_bytes(t["out"][42:46].tobytes(), "big") == 1000
    t = E.ack_timer(fire, tx, table, dk, LINKS, out, slot_stride=64, max_frames=0)
    assert t["status"][0] == E.NO_ROOM and t["dack"].tobytes() == dk.tobytes() and (t["out"] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. frame validity
# ---------------------------------------------------------------------------------------------------------------------
def test_frames_parse_with_valid_checksums():
    import tx_segment_reference as M

    nc = 12
    flows = synth.make_flows(nc, passive=False)
    rng = np.random.default_rng(5)
    rn = rng.integers(0, 1 << 32, nc, dtype=np.uint64)
    rn[::4] = 0xFFFFFFF0
    tx = M.conns_toward(flows, seed=6)
    tx["rcv_wscale"] = rng.integers(0, 15, nc)
    table = conn_table(nc, receive_next=rn, send_next=tx["snd_nxt"], buffer_size=60000)
    segs = [(int(rn[c]) + 100 * k, 100, ACK | PSH, int(tx["snd_nxt"][c]), c) for k in range(5) for c in range(nc)]
    links = M.links_table()
    dack = dack_conn_table(nc, armed=1)
    out = np.zeros(len(segs) * 96, np.uint8)
    got = E.ack_emit(batch(segs), table, tx, dack, links, NOW, out, slot_stride=96, frame_lead=3, max_frames=len(segs))
    assert got["n_frames"] == 3 * nc
    for f, (i, c, ack, wnd) in enumerate(got["desc"]):
        a = int(got["off_out"][f])
        fr = got["out"][a:a + 54].tobytes()
        T = tx[c]
        assert fr[:12] == bytes(links[int(T["link"])]["dst_mac"]) + bytes(links[int(T["link"])]["src_mac"])
        v, (src, dst, proto, po, pl) = O.ipv4_parse(fr[14:])
        assert v == -1 and (proto, po, pl) == (6, 20, 20) and O.ipv4_checksum(fr[14:34]) == int.from_bytes(fr[24:26], "big")
        v, (nopt, plen) = O.tcp_parse(src, dst, fr[34:], False)
        assert v == -1 and nopt == 0 and plen == 0, (f, v)
        assert int.from_bytes(fr[38:42], "big") == int(T["snd_nxt"]) and int.from_bytes(fr[42:46], "big") == ack
        assert fr[47] == ACK and int.from_bytes(fr[48:50], "big") == wnd >> int(T["rcv_wscale"])
        bad = bytearray(fr[34:])
        bad[7] ^= 1
        assert O.tcp_parse(src, dst, bytes(bad), False)[0] == N.V["TCP_CSUM"]
    off = E.ack_emit(batch(segs), table, tx, dack, links, NOW, out, slot_stride=96, max_frames=len(segs),
                     flags=N.DK_TX_OFFLOAD_TCP)
    assert all(not off["out"][int(a) + 50:int(a) + 52].any() for a in off["off_out"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_constants(tmp_path):
    """sizeof / offsetof and the enum values from the C compiler == the ctypes mirrors, the numpy dtype and the
    Python constants."""
    structs = {"dk_tcp_dack_conn": N.DkTcpDackConn, "dk_tcp_ackemit_results": N.DkTcpAckEmitResults}
    names = [f"DK_TCP_ACKEMIT_{s}" for s in N.TCP_ACKEMIT_STATUSES]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for sname, cls in structs.items():
        lines.append(f'printf("size.{sname} %zu\\n", sizeof({sname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{sname}.{fname} %zu\\n", offsetof({sname}, {fname}));')
    for nm in names:
        lines.append(f'printf("{nm} %d\\n", (int){nm});')
    lines.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.splitlines())
    for sname, cls in structs.items():
        assert int(got[f"size.{sname}"]) == ctypes.sizeof(cls), sname
        for fname, _ in cls._fields_:
            assert int(got[f"{sname}.{fname}"]) == getattr(cls, fname).offset, (sname, fname)
    assert int(got["size.dk_tcp_dack_conn"]) == 32 == N.DACK_CONN_DTYPE.itemsize == E.DACK_DTYPE.itemsize
    for fname, _ in N.DkTcpDackConn._fields_:
        assert N.DACK_CONN_DTYPE.fields[fname][1] == getattr(N.DkTcpDackConn, fname).offset == E.DACK_DTYPE.fields[fname][1]
    assert [f for f, _ in N.DkTcpAckEmitResults._fields_] == N.TCP_ACKEMIT_RESULT_FIELDS
    for i, s in enumerate(N.TCP_ACKEMIT_STATUSES):
        assert int(got[f"DK_TCP_ACKEMIT_{s}"]) == i == getattr(E, s), s
    assert N.DK_TCP_ACKEMIT_NO_FRAME == E.NO_FRAME == 0xFFFFFFFF
    hdr = open(HEADER).read()
    assert re.search(r"int dk_tcp_ack_emit\(dk_tcp_ctx\* ctx", hdr) and re.search(r"int dk_tcp_ack_timer\(dk_tcp_tx_ctx\* ctx", hdr)
    assert "#define DK_RX_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "dk_rx.h")).read()
    lib = N.load_library()
    assert lib.dk_tcp_ack_emit and lib.dk_tcp_ack_timer and lib.dk_diag_tcp_ack_emit_set_form
