"""tests/tcp_ack_reference.py pinned on the CPU against answers derived by hand from the reference (rto.rs:40-79,
sender.rs:406-508) and dk_tcp_ack_process's contract (include/dk_tcp.h), and the layout of the new structs from the C
compiler against the ctypes mirror."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tcp_ack_cases as C
import tcp_ack_reference as R
from demikernel_amd import _native as N
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_ack import ack_conn_table
from demikernel_amd.tcp_tx import tx_conn_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, S = R.NONE, 10**9


def run(segs, *, una=1000, nxt=None, wnd=5000, wl1=0, wl2=0, wscale=0, queue=(), now=10 * S, nconns=1, **bad):
    """One connection (row 0 of `nconns`), segments (seq, ack, win[, action]); queue: (off, len, tx_time) entries."""
    nxt = (una + sum(e[1] or 1 for e in queue)) & R.M32 if nxt is None else nxt
    tx = tx_conn_table(nconns, snd_nxt=nxt, snd_una=una, snd_wnd=wnd)
    rx = conn_table(nconns, send_next=nxt)
    ak = ack_conn_table(nconns, wl1=wl1, wl2=wl2, snd_wscale=wscale, q_first=0, q_count=0)
    ak["q_count"][0] = len(queue)
    for k, v in bad.items():
        t, f = k.split("__")
        {"tx": tx, "rx": rx, "ak": ak}[t][f][0] = v
    pool = {"off": np.array([e[0] for e in queue], np.uint32), "len": np.array([e[1] for e in queue], np.uint32),
            "tx_time": np.array([e[2] for e in queue], np.uint64)}
    a = np.array([tuple(s) + (R.NO_DATA,) * (4 - len(s)) for s in segs], np.int64).reshape(len(segs), 4)
    act = a[:, 3]
    return R.ack_process(np.zeros(len(segs), np.uint32), act, a[:, 0] & R.M32, a[:, 1] & R.M32, a[:, 2], rx, tx, ak,
                         pool, now), (tx, ak, pool)


def test_rto_answers_by_hand():
    r = R.Rto()
    assert (r.srtt, r.rttvar, r.rto, r.received_sample) == (1.0, 0.0, 1.0, False)
    r.add_sample_ns(S // 2)  # first sample 0.5 s: srtt = rtt, rttvar = rtt / 2, rto = 0.5 + 4 * 0.25
    assert (r.srtt, r.rttvar, r.rto) == (0.5, 0.25, 1.5)
    r.add_sample_ns(3 * S // 10)  # 0.3 s: rttvar = 0.75 * 0.25 + 0.25 * |0.5 - 0.3|, srtt = 0.875 * 0.5 + 0.125 * 0.3
    assert r.rttvar == 0.75 * 0.25 + 0.25 * abs(0.5 - 0.3) and abs(r.rttvar - 0.2375) < 1e-15
    assert r.srtt == 0.875 * 0.5 + 0.125 * 0.3 and abs(r.srtt - 0.475) < 1e-15
    assert r.rto == r.srtt + 4.0 * r.rttvar
    r = R.Rto()
    r.add_sample_ns(1000000)  # 1 ms: 0.001 + max(0.001, 0.002) = 0.003 -> the lower clamp
    assert (r.srtt, r.rttvar, r.rto) == (0.001, 0.0005, 0.1)
    r = R.Rto()
    r.add_sample_ns(100 * S)  # 100 s: 100 + 200 -> the upper clamp
    assert (r.srtt, r.rttvar, r.rto) == (100.0, 50.0, 60.0)
    r = R.Rto()
    r.add_sample_ns(2 * S + 250000000)  # as_secs_f64: whole seconds + nanos / 1e9
    assert r.srtt == 2.0 + 250000000 / 1e9 == 2.25


def test_rtt_beyond_32_bits_by_hand():
    r = R.Rto()
    r.add_sample_ns(2**32 + 1)  # 4,294,967,297 ns: 4 s + 294,967,297 ns
    assert r.srtt == 4.0 + 294967297 / 1e9 == 4.294967297 and r.rto == 4.294967297 + 4.0 * (4.294967297 / 2.0)
    r = R.Rto()
    r.add_sample_ns(2**53 + 1)  # 9,007,199,254,740,993 ns: not an f64; whole seconds and nanoseconds apart are
    assert r.srtt == 9007199.0 + 254740993 / 1e9 == 9007199.254740993 and r.rto == 60.0
    r = R.Rto()
    r.add_sample_ns(2**64 - 2)
    assert r.srtt == 18446744073.0 + 709551614 / 1e9


def extremes_with(change, now):
    """The reference over tcp_ack_cases.extremes(now) with every sample d replaced by change(d)."""
    case = C.extremes(now)
    h = C.host_actions(case)
    plain = R.Rto.add_sample_ns
    try:
        if change is not None:
            R.Rto.add_sample_ns = lambda self, d: plain(self, change(d))
        return case, R.ack_process(h["flow_id"], h["action"], h["tcp_seq"], h["tcp_ack"], h["tcp_win"], case["rx"],
                                   case["tx"], case["ak"], case["pool"], now)
    finally:
        R.Rto.add_sample_ns = plain


@pytest.mark.parametrize("now", C.EXTREME_NOWS)
def test_extremes_scenario_and_its_guards(now):
    """The RTT / RTO extremes batch of the GPU tests does what it was built for, and tells the two wrong kernels it is
    there for from a right one: d cut to 32 bits, and now - tx taken as an int64 (negative from 2^63: saturated)."""
    case, exp = extremes_with(None, now)
    C.check_extremes(case, exp)
    _, masked = extremes_with(lambda d: d & 0xFFFFFFFF, now)
    _, signed = extremes_with(lambda d: d if d < 2**63 else 0, now)
    for c in (0, 1, 3):
        assert masked["ack_conns"]["srtt"][c] != exp["ack_conns"]["srtt"][c], c
        assert signed["ack_conns"]["srtt"][c] != exp["ack_conns"]["srtt"][c], c
    # a transmit time above now gives the sample 0, not a huge one
    if now + 1 < R.NONE:
        assert any(t != R.NONE and t > now for t in case["scripts"][0].tx_times)


def test_ack_splits_an_entry_then_pops_it_without_a_sample():
    q = [(100, 300, 9 * S), (400, 200, 9 * S + S // 2)]
    r, _ = run([(7, 1100, 4000)], queue=q)  # 100 of entry 0's 300 bytes
    a = r["ack_conns"][0]
    assert r["acked"][0] == 100 and r["samples"][0] == 1 and r["bytes_acked"][0] == 100 and r["new_acks"][0] == 1
    assert (a["q_first"], a["q_count"]) == (0, 2)
    assert (r["pool"]["off"][0], r["pool"]["len"][0], r["pool"]["tx_time"][0]) == (200, 200, NONE)
    assert (a["srtt"], a["rttvar"], a["rto"]) == (1.0, 0.5, 3.0)  # one sample of 10 s - 9 s
    assert (a["rtx_armed"], a["rtx_base_ns"]) == (1, 10 * S)  # the trimmed front has no transmit time: now
    assert r["tx_conns"]["snd_una"][0] == 1100
    # the next call's ACK pops the rest of it: no sample (Karn), the deadline from the next entry's transmit time
    q2 = [(200, 200, NONE), (400, 200, 9 * S + S // 2)]
    r2, _ = run([(7, 1300, 4000)], una=1100, queue=q2, ak__received_sample=1, ak__srtt=1.0, ak__rttvar=0.5, ak__rto=3.0)
    a = r2["ack_conns"][0]
    assert r2["samples"][0] == 0 and (a["srtt"], a["rttvar"], a["rto"]) == (1.0, 0.5, 3.0)
    assert (a["q_first"], a["q_count"], a["rtx_armed"], a["rtx_base_ns"]) == (1, 1, 1, 9 * S + S // 2)
    # both ACKs in one call: the entry is sampled once
    r3, _ = run([(7, 1100, 4000), (7, 1300, 4000), (7, 1500, 4000)], queue=q)
    a = r3["ack_conns"][0]
    assert list(r3["acked"]) == [100, 200, 200] and r3["samples"][0] == 2 and (a["q_first"], a["q_count"]) == (2, 0)
    assert (a["rtx_armed"], a["rtx_base_ns"]) == (0, 0)
    e = R.Rto()
    e.add_sample(1.0), e.add_sample(0.5)
    assert (a["srtt"], a["rttvar"], a["rto"]) == (e.srtt, e.rttvar, e.rto)


def test_marker_swallows_the_remainder():
    q = [(0, 100, NONE), (0, 0, 9 * S)]
    r, _ = run([(7, 1101, 4000)], queue=q)  # 100 bytes + the FIN's sequence number
    a = r["ack_conns"][0]
    assert r["acked"][0] == 101 and r["samples"][0] == 1 and (a["q_first"], a["q_count"], a["rtx_armed"]) == (2, 0, 0)
    # a remainder above 1 at the marker is swallowed whole; entries behind the marker stay
    q = [(0, 100, NONE), (0, 0, NONE), (5, 50, 8 * S)]
    r, _ = run([(7, 1140, 4000)], queue=q, nxt=1200)
    a = r["ack_conns"][0]
    assert r["status"][0] == R.OK and (a["q_first"], a["q_count"]) == (2, 1) and r["samples"][0] == 0
    assert (a["rtx_armed"], a["rtx_base_ns"]) == (1, 8 * S) and r["tx_conns"]["snd_una"][0] == 1140


def test_window_update_three_branches():
    q = [(0, 1000, NONE)]
    # wl1 < seq: taken
    r, _ = run([(50, 1010, 300)], queue=q, wl1=40, wl2=900, wscale=2)
    assert (r["tx_conns"]["snd_wnd"][0], r["ack_conns"]["wl1"][0], r["ack_conns"]["wl2"][0]) == (1200, 50, 1010)
    # wl1 == seq and wl2 <= ack: taken
    r, _ = run([(40, 1010, 300)], queue=q, wl1=40, wl2=900)
    assert (r["tx_conns"]["snd_wnd"][0], r["ack_conns"]["wl1"][0], r["ack_conns"]["wl2"][0]) == (300, 40, 1010)
    # wl1 > seq: not taken, SND.UNA still moves
    r, _ = run([(30, 1010, 300)], queue=q, wl1=40, wl2=900)
    assert (r["tx_conns"]["snd_wnd"][0], r["ack_conns"]["wl1"][0], r["ack_conns"]["wl2"][0]) == (5000, 40, 900)
    assert r["tx_conns"]["snd_una"][0] == 1010
    # an ACK that is not new never updates the window
    r, _ = run([(60, 1000, 300)], queue=q, wl1=40, wl2=900)
    assert r["tx_conns"]["snd_wnd"][0] == 5000 and r["ack_conns"]["wl1"][0] == 40 and r["dup_acks"][0] == 1
    # a reordered pair: the later segment has the lower seq and the higher ack: its window is not taken
    r, _ = run([(50, 1010, 300), (45, 1020, 77)], queue=q, wl1=40, wl2=900)
    assert (r["tx_conns"]["snd_wnd"][0], r["ack_conns"]["wl1"][0], r["ack_conns"]["wl2"][0]) == (300, 50, 1010)
    assert r["tx_conns"]["snd_una"][0] == 1020 and r["new_acks"][0] == 2


def test_duplicate_and_old_ack():
    q = [(0, 1000, 9 * S)]
    r, _ = run([(7, 1100, 10), (7, 1100, 10), (7, 1050, 10), (7, 1100, 10, 6), (7, 1100, 10, 11)], queue=q)
    assert list(r["acked"][:2]) == [100, 0] and r["acked"][2] == (1050 - 1100) & R.M32 >= 1 << 31
    assert list(r["acked"][3:]) == [0, 0]  # DUPLICATE and ACK_UNSENT segments never reach process_ack
    assert (r["new_acks"][0], r["dup_acks"][0], r["bytes_acked"][0], r["samples"][0]) == (1, 1, 100, 1)


def test_every_failure_status_leaves_the_connection_alone():
    q = [(0, 100, 9 * S)]
    cases = {R.E_STATE: dict(tx__state=N.DK_TCP_CLOSED), R.E_SND_NXT: dict(rx__send_next=7),
             R.E_FLIGHT: dict(una=1000, nxt=(1000 + (1 << 31)) & R.M32), R.E_WSCALE: dict(wscale=15),
             R.E_WL2: dict(wl2=1001), R.E_QUEUE: dict(ak__q_first=1)}
    for status, kw in cases.items():
        r, (tx, ak, pool) = run([(7, 1050, 10)], queue=q, **kw)
        assert r["status"][0] == status, status
        assert r["acked"][0] == 0 and r["new_acks"][0] == r["dup_acks"][0] == r["bytes_acked"][0] == r["samples"][0] == 0
        assert r["tx_conns"].tobytes() == tx.tobytes() and r["ack_conns"].tobytes() == ak.tobytes()
        assert all(np.array_equal(r["pool"][k], pool[k]) for k in pool)
    # the queue runs dry: after a first ACK that was fine
    r, (tx, ak, pool) = run([(7, 1050, 10), (7, 1200, 10)], queue=q, nxt=1300)
    assert r["status"][0] == R.E_DRY and list(r["acked"]) == [0, 0] and r["new_acks"][0] == 0
    assert r["tx_conns"].tobytes() == tx.tobytes() and r["ack_conns"].tobytes() == ak.tobytes()
    assert all(np.array_equal(r["pool"][k], pool[k]) for k in pool)
    assert R.E_DRY == 7 and len(N.TCP_ACK_STATUSES) == 8


def test_the_2_31_deviation():
    # SND.UNA == SND.NXT, an ack exactly 2^31 behind: "new" by the sign of the wrapping difference, old here
    assert R.seq_lt(5000, (5000 - (1 << 31)) & R.M32)
    r, (tx, ak, _) = run([(7, (5000 - (1 << 31)) & R.M32, 10)], una=5000, nxt=5000)
    assert r["status"][0] == R.OK and r["acked"][0] == 1 << 31 and r["new_acks"][0] == 0 and r["dup_acks"][0] == 0
    assert r["tx_conns"].tobytes() == tx.tobytes() and r["ack_conns"].tobytes() == ak.tobytes()
    # with data in flight the same ack compares old in the reference too
    r, _ = run([(7, (5000 - (1 << 31)) & R.M32, 10)], una=4000, nxt=5000, queue=[(0, 1000, NONE)])
    assert r["new_acks"][0] == 0 and r["acked"][0] == ((5000 - (1 << 31)) - 4000) & R.M32


def test_sequence_numbers_wrap_through_zero():
    una = (1 << 32) - 300
    q = [(0, 200, NONE), (200, 200, NONE), (400, 200, NONE)]
    r, _ = run([((1 << 32) - 5, una + 250, 9), (3, una + 500, 11)], una=una, queue=q, wl1=(1 << 32) - 10,
               wl2=una - 20)
    a = r["ack_conns"][0]
    assert list(r["acked"]) == [250, 250] and r["tx_conns"]["snd_una"][0] == 200  # through zero
    assert (a["wl1"], a["wl2"], r["tx_conns"]["snd_wnd"][0]) == (3, 200, 11)  # wl1 and wl2 wrapped with it
    assert (a["q_first"], a["q_count"]) == (2, 1) and (r["pool"]["off"][2], r["pool"]["len"][2]) == (500, 100)
    # wl1 just above zero, a segment just below it: the lower seq does not update
    r, _ = run([((1 << 32) - 5, una + 250, 9)], una=una, queue=q, wl1=2, wl2=una)
    assert r["tx_conns"]["snd_wnd"][0] == 5000 and r["ack_conns"]["wl1"][0] == 2


def test_untouched_rows_and_unprocessed_frames():
    r, (tx, ak, _) = run([(7, 1050, 10, 12), (7, 1050, 10, 0)], queue=[(0, 100, 9 * S)], nconns=3)
    assert list(r["status"]) == [0, 0, 0] and not r["acked"].any() and not r["new_acks"].any()
    assert r["tx_conns"].tobytes() == tx.tobytes() and r["ack_conns"].tobytes() == ak.tobytes()


def test_new_struct_layout_matches_ctypes(tmp_path):
    """sizeof / offsetof of dk_tcp_ack_conn, dk_tcp_unacked and dk_tcp_ack_out from the C compiler == the ctypes
    mirror and the numpy dtype; the status enum and the NONE constant == the Python lists."""
    hdr = os.path.join(ROOT, "include", "dk_tcp.h")
    structs = {"dk_tcp_ack_conn": N.DkTcpAckConn, "dk_tcp_unacked": N.DkTcpUnacked, "dk_tcp_ack_out": N.DkTcpAckOut}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{hdr}"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("none %llu\\n", (unsigned long long)DK_TCP_TX_TIME_NONE);')
    lines.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(c)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)
    assert ctypes.sizeof(N.DkTcpAckConn) == N.ACK_CONN_DTYPE.itemsize == 64
    for fname, _ in N.DkTcpAckConn._fields_:
        assert N.ACK_CONN_DTYPE.fields[fname][1] == getattr(N.DkTcpAckConn, fname).offset, fname
    assert int(got["none"]) == N.DK_TCP_TX_TIME_NONE == R.NONE
    text = open(hdr).read()
    for i, name in enumerate(N.TCP_ACK_STATUSES):
        assert re.search(rf"DK_TCP_ACK_{name} = {i}[,\s]", text), name
    assert [f for f, _ in N.DkTcpAckOut._fields_] == N.TCP_ACK_OUT_FIELDS


def test_ack_process_is_exported_and_bound():
    lib = N.load_library()
    for name in ("dk_tcp_ack_process", "dk_diag_tcp_ack_set_form", "dk_diag_tcp_ack_last_form"):
        assert getattr(lib, name).argtypes is not None


def test_ack_process_rejects_calls_without_a_gpu():
    """Argument checks come before any device work: a null context is EINVAL everywhere."""
    lib = N.load_library()
    assert lib.dk_tcp_ack_process(None, None, 0, None, None, None, None, 0, None, 0, 0, None, None) == 22
    assert lib.dk_diag_tcp_ack_set_form(None, 0) == 22 and lib.dk_diag_tcp_ack_last_form(None) == -1


if __name__ == "__main__":
    raise SystemExit(pytest.main([__file__, "-q"]))
