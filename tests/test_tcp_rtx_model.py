"""dk_tcp_retransmit on the CPU: tests/tcp_rtx_reference.py, the restatement the GPU tests compare against, replayed over
every recording of tests/ack_net.py, whose host retransmits by hand (ack_net.resend, the timer's back-off), and the ABI
additions (struct layout, constants) against the C compiler. No GPU work.

Each round the restatement is called on the tables as the recording had them, with fire = TIMEOUT for the connections
whose timer the recording fired (rto_set) and FAST for the rest of its retransmissions. Its state writes must be the
recording's (tx_time := NONE at the fronts, rto, rtx_base_ns) bit for bit, and every frame must carry the sequence
number, ack number, flags, window and payload of ack_net.resend's frame for that connection. The tables are carried
from round to round by the recording's own steps and must meet the state every recorded ACK call started from."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ack_net as AN
import tcp_rtx_reference as X
from demikernel_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_tcp.h")

# timer / fast retransmissions and resent FINs of each recording, and whether a round has both kinds together
EXPECT = {"one_long": (12, 9, 0, False), "few": (6, 32, 0, True), "many": (69, 51, 0, True),
          "wide_300": (476, 196, 17, True), "fin_lost": (7, 3, 3, False), "piggy": (8, 6, 0, True)}


def fire_of(r, rows: int) -> np.ndarray:
    fire = np.zeros(rows, np.uint8)
    fire[r.rtx] = X.FIRE_FAST
    fire[r.rto_set[0]] = X.FIRE_TIMEOUT
    return fire


def fields(frame: bytes):
    tot = int.from_bytes(frame[16:18], "big")
    return (int.from_bytes(frame[38:42], "big"), int.from_bytes(frame[42:46], "big"), frame[47],
            int.from_bytes(frame[48:50], "big"), frame[54:14 + tot])


def replay(name: str) -> dict:
    tr = AN.trace(name)
    rows, cap = len(tr.tx0), tr.cap
    tx, ak = tr.tx0.copy(), tr.ak0.copy()
    pool = {"off": np.zeros(rows * cap, np.uint32), "len": np.zeros(rows * cap, np.uint32),
            "tx_time": np.zeros(rows * cap, np.uint64)}
    out0 = np.full(rows * tr.stride, 0xA5, np.uint8)
    seen = dict(timer=0, fast=0, fin=0, both=0, burst=0)
    for rnd, r in enumerate(tr.rounds):
        ctx = f"{name} round {rnd}"
        tx["mss"] = r.mss
        fire = fire_of(r, rows)
        assert len(set(r.rtx.tolist())) == len(r.rtx) and set(r.rto_set[0].tolist()) <= set(r.rtx.tolist()), ctx
        got = X.retransmit(tr.src, fire, tx, ak, pool, r.t_send, tr.links, out0, slot_stride=tr.stride,
                           max_frames=rows)
        # the state the recording's host left: the fronts' tx_time, the timer's rto and base
        want_ak, want_tt = ak.copy(), pool["tx_time"].copy()
        want_tt[ak["q_first"][r.rtx]] = AN.NONE
        want_ak["rto"][r.rto_set[0]] = r.rto_set[1]
        want_ak["rtx_base_ns"][r.base_set[0]] = r.base_set[1]
        assert got["ack_conns"].tobytes() == want_ak.tobytes(), f"{ctx}: the ACK table"
        assert np.array_equal(got["pool"]["tx_time"], want_tt), f"{ctx}: tx_time"
        assert all(np.array_equal(got["pool"][k], pool[k]) for k in ("off", "len")), f"{ctx}: off / len"
        want_st = np.where(fire != 0, X.SENT, X.NOT_FIRED)
        assert np.array_equal(got["status"], want_st), f"{ctx}: statuses {got['status'][fire != 0]}"
        assert got["n_frames"] == len(r.rtx) == len(got["off_out"]), ctx
        assert np.array_equal(got["frame_conn"], np.sort(r.rtx)), f"{ctx}: frames are not in connection order"
        for f, c in enumerate(got["frame_conn"]):
            e = int(ak["q_first"][c])
            off, ln = int(pool["off"][e]), int(pool["len"][e])
            a = int(got["off_out"][f])
            assert (a, int(got["len_out"][f]), int(got["frame"][c])) == (f * tr.stride, 54 + ln, f), ctx
            mine = got["out"][a:a + 54 + ln].tobytes()
            assert fields(mine) == fields(AN.resend(tr, tx, int(c), off, ln)), f"{ctx}: connection {c}'s frame"
            seen["fin"] += ln == 0
            assert (int(c), off + ln, ln == 0) in r.rtx_keys, f"{ctx}: not the entry the recording resent"
        used = np.zeros(len(out0), bool)
        for a, ln in zip(got["off_out"], got["len_out"]):
            used[int(a):int(a) + int(ln)] = True
        assert (got["out"][~used] == 0xA5).all(), f"{ctx}: bytes outside the frames"
        nt, nf = len(r.rto_set[0]), len(r.rtx) - len(r.rto_set[0])
        seen["timer"] += nt
        seen["fast"] += nf
        seen["both"] += bool(nt and nf)
        seen["burst"] = max(seen["burst"], len(r.rtx))
        # the recording's own steps to the next round
        ak, pool = got["ack_conns"], got["pool"]
        if r.seg is not None:
            tx = r.seg["tx_conns"].copy()
            AN.append_frames(ak, pool, cap, *r.sends, r.t_send)
        if r.ack is not None:
            s = r.ack.start
            assert tx.tobytes() == s["tx"].tobytes() and ak.tobytes() == s["ak"].tobytes(), \
                f"{ctx}: the tables are not those the recorded ACK call started from"
            assert all(np.array_equal(pool[k], s["pool"][k]) for k in pool), f"{ctx}: the pool"
            e = r.ack.exp
            tx, ak, pool = e["tx_conns"].copy(), e["ack_conns"].copy(), {k: v.copy() for k, v in e["pool"].items()}
    assert tr.done
    return seen


@pytest.mark.parametrize("name", list(AN.CASES))
def test_restatement_replays_the_recording(name):
    tr = AN.trace(name)
    seen = replay(name)
    print(name, seen)
    assert seen["timer"] + seen["fast"] == tr.stats["timer_rtx"] + tr.stats["fast_rtx"]
    assert (seen["timer"], seen["fast"]) == (tr.stats["timer_rtx"], tr.stats["fast_rtx"])
    assert seen["timer"] and seen["fast"], "a case without one of the two kinds"
    timer, fast, fin, both = EXPECT[name]
    assert (seen["timer"], seen["fast"], int(seen["fin"]), bool(seen["both"])) == (timer, fast, fin, both), seen
    if name == "wide_300":
        assert seen["burst"] == 221


def test_status_order_and_idle():
    """The checks in the header's order on hand-made rows: the connection's own, IDLE, then the front entry's."""
    from demikernel_amd.tcp_ack import ack_conn_table
    from demikernel_amd.tcp_tx import tx_conn_table

    n = 12
    tx = tx_conn_table(n, snd_nxt=1000, snd_una=900, rcv_wnd_hdr=100)
    ak = ack_conn_table(n, q_first=np.arange(n), q_count=1)
    ak["rtx_armed"] = 1
    pool = {"off": np.arange(n, dtype=np.uint32) * 10, "len": np.full(n, 10, np.uint32),
            "tx_time": np.full(n, 7, np.uint64)}
    links = np.zeros(1, N.TX_LINK_DTYPE)
    src = np.arange(200, dtype=np.uint8)
    fire = np.full(n, X.FIRE_TIMEOUT, np.uint8)
    fire[0], fire[1], fire[11] = 0, 3, X.FIRE_FAST
    tx["state"][2] = N.DK_TCP_CLOSED
    ak["q_first"][3] = n            # beyond the pool
    pool["off"][4] = 195            # beyond src
    pool["len"][5] = 11             # 54 + 11 > 64
    tx["link"][6] = 1
    ak["q_count"][8] = 0            # IDLE
    ak["rtx_armed"][9] = 0          # IDLE under TIMEOUT
    ak["rtx_armed"][11] = 0         # FAST does not need the timer
    tx["state"][1] = N.DK_TCP_CLOSED  # E_FIRE comes before E_STATE
    ak["q_count"][6] = 0            # E_LINK before IDLE
    got = X.retransmit(src, fire, tx, ak, pool, 55, links, np.zeros(64 * n, np.uint8), slot_stride=64, max_frames=n)
    want = [X.NOT_FIRED, X.E_FIRE, X.E_STATE, X.E_QUEUE, X.E_RANGE, X.E_SLOT, X.E_LINK, X.SENT, X.IDLE, X.IDLE,
            X.SENT, X.SENT]
    assert got["status"].tolist() == want
    assert got["frame"].tolist() == [X.NO_FRAME] * 7 + [0, X.NO_FRAME, X.NO_FRAME, 1, 2]
    sent = np.array([7, 10, 11])
    assert (got["pool"]["tx_time"][sent] == X.NONE).all() and (np.delete(got["pool"]["tx_time"], sent) == 7).all()
    assert got["ack_conns"]["rto"].tolist() == [1.0] * 7 + [2.0, 1.0, 1.0, 2.0, 1.0]
    assert got["ack_conns"]["rtx_base_ns"].tolist() == [0] * 7 + [55, 0, 0, 55, 0]
    assert got["ack_conns"]["rtx_armed"][11] == 0
    # one frame short: nothing is done
    short = X.retransmit(src, fire, tx, ak, pool, 55, links, np.zeros(64 * n, np.uint8), slot_stride=64, max_frames=2)
    assert short["n_frames"] == 3 and (short["frame"] == X.NO_FRAME).all() and not short["out"].any()
    assert short["status"].tolist() == [X.NO_ROOM if s == X.SENT else s for s in want]
    assert short["ack_conns"].tobytes() == ak.tobytes() and np.array_equal(short["pool"]["tx_time"], pool["tx_time"])
    # the window that does not fit 16 bits, from a receive table
    from demikernel_amd.tcp import conn_table
    rx = conn_table(n, receive_next=5, buffer_size=1 << 20)
    rx["buffer_size"][7] = 1000
    w = X.retransmit(src, fire, tx, ak, pool, 55, links, np.zeros(64 * n, np.uint8), slot_stride=64, max_frames=n,
                     rx_conns=rx)
    assert w["status"].tolist() == [X.NOT_FIRED, X.E_FIRE, X.E_STATE, X.E_QUEUE, X.E_WINDOW, X.E_WINDOW, X.E_LINK,
                                    X.SENT, X.E_WINDOW, X.E_WINDOW, X.E_WINDOW, X.E_WINDOW]
    assert X.back_off(0.04) == 0.1 and X.back_off(30.0) == 60.0 and X.back_off(45.0) == 60.0
    assert X.back_off(29.999999999999996) == 2 * 29.999999999999996 < 60.0


def test_rtx_struct_layout_and_constants(tmp_path):
    """sizeof / offsetof and the enum values from the C compiler == the ctypes mirror and the Python constants."""
    cls = N.DkTcpRtxResults
    names = [f"DK_TCP_RTX_{s}" for s in N.TCP_RTX_STATUSES] + ["DK_TCP_RTX_NONE", "DK_TCP_RTX_TIMEOUT",
                                                               "DK_TCP_RTX_FAST"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(dk_tcp_rtx_results));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("f.{fname} %zu\\n", offsetof(dk_tcp_rtx_results, {fname}));')
    for nm in names:
        lines.append(f'printf("{nm} %d\\n", (int){nm});')
    lines.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"f.{fname}"]) == getattr(cls, fname).offset, fname
    assert [f for f, _ in cls._fields_] == N.TCP_RTX_RESULT_FIELDS
    for i, s in enumerate(N.TCP_RTX_STATUSES):
        assert int(got[f"DK_TCP_RTX_{s}"]) == i == getattr(N, f"DK_TCP_RTX_{s}") == getattr(X, s), s
    assert [int(got[k]) for k in names[-3:]] == [N.DK_TCP_RTX_NONE, N.DK_TCP_RTX_TIMEOUT, N.DK_TCP_RTX_FAST] == [0, 1, 2]
    assert N.DK_TCP_RTX_NO_FRAME == X.NO_FRAME == 0xFFFFFFFF
    hdr = open(HEADER).read()
    assert re.search(r"int dk_tcp_retransmit\(dk_tcp_tx_ctx\* ctx", hdr)
    assert "#define DK_RX_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "dk_rx.h")).read()
    assert N.load_library().dk_tcp_retransmit
