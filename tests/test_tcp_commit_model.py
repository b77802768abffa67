"""dk_tcp_tx_commit / dk_tcp_rtx_piggyback on the CPU: the numpy model (tests/tcp_commit_reference.py) against
ack_net.append_frames over tx_segment_reference.segment outputs, hand cases of the placement rule at its edges, the
identity the kernels' closed form of an entry's offset rests on, and the ABI additions (struct layout against the C
compiler, constants against the header, the symbols, EINVAL decided before any GPU work)."""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import ack_net as A
import tcp_commit_reference as C
import tx_segment_reference as M
from demikernel_amd import _native as N
from demikernel_amd import synth, tcp_commit
from demikernel_amd.tcp_ack import ack_conn_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_tcp.h")
NOW = 77 * 10**9


def random_case(seed: int, nconns: int = 7, cap: int = 48):
    """A segmentation call over random pushes (several buffers per connection, markers, closed windows, a connection
    without buffers) and queues that are empty, in the middle of their region or at its end."""
    rng = np.random.default_rng(seed)
    flows = synth.make_flows(nconns, passive=False, seed=seed)
    mss = rng.integers(3, 40, nconns)
    wnd = mss * rng.integers(0, 12, nconns) + rng.integers(0, 5, nconns)  # some windows end inside a segment
    tx = M.conns_toward(flows, seed=seed, mss=mss, snd_wnd=wnd, link=0)
    conn, lens = [], []
    for c in range(nconns):
        for _ in range(int(rng.integers(0, 4))):
            conn.append(c), lens.append(int(rng.integers(0, 6) and rng.integers(1, 200)))
    src, pc, po, pl = M.pack_push(conn, lens, seed=seed)
    seg = M.segment(src, pc, po, pl, tx, M.links_table(), np.zeros(512 * 128, np.uint8), slot_stride=128, frame_lead=0,
                    max_frames=512)
    assert (seg["status"] != M.NO_ROOM).all()
    cnt = np.bincount(pc[seg["frame_buf"]].astype(np.int64), minlength=nconns)
    qc = np.minimum(rng.integers(0, 30, nconns), cap - cnt)
    qc[rng.random(nconns) < 0.3] = 0
    slack = cap - qc
    qf = np.arange(nconns) * cap + (rng.random(nconns) * (slack + 1)).astype(np.int64)
    at_end = rng.random(nconns) < 0.3
    qf[at_end] = (np.arange(nconns) * cap + slack)[at_end]  # the live range ends where the region ends
    ak = ack_conn_table(nconns, q_first=qf, q_count=qc)
    ak["rtx_armed"] = rng.integers(0, 2, nconns) * rng.integers(1, 9, nconns)
    ak["rtx_base_ns"] = rng.integers(1, 10**9, nconns)
    pool = {"off": rng.integers(0, 1 << 32, nconns * cap, dtype=np.uint64).astype(np.uint32),
            "len": rng.integers(0, 1 << 16, nconns * cap, dtype=np.uint64).astype(np.uint32),
            "tx_time": rng.integers(0, 1 << 62, nconns * cap, dtype=np.uint64)}
    return (pc, po, pl), seg, tx, ak, pool, cap


@pytest.mark.parametrize("seed", range(12))
def test_model_matches_append_frames(seed):
    push, seg, _, ak, pool, cap = random_case(seed)
    exp = C.tx_commit(push[0], push[1], seg, ak, pool, cap, NOW)
    ak2, pool2 = ak.copy(), {k: v.copy() for k, v in pool.items()}
    ak2["rtx_armed"] = ak["rtx_armed"] != 0  # append_frames ORs 1 into the flag; armed is armed
    A.append_frames(ak2, pool2, cap, *A.sent_entries(push, seg), NOW)
    assert (exp["status"] == C.OK).all()
    e = exp["ack_conns"]
    assert np.array_equal(e["q_count"], ak2["q_count"])
    assert np.array_equal(e["rtx_armed"] != 0, ak2["rtx_armed"] != 0)
    assert np.array_equal(e["rtx_base_ns"], ak2["rtx_base_ns"])
    sent = exp["k"] > 0
    assert np.array_equal(e["rtx_armed"][~sent], ak["rtx_armed"][~sent]) and e[~sent].tobytes() == ak[~sent].tobytes()
    for c in range(len(ak)):
        a, b, n = int(e["q_first"][c]), int(ak2["q_first"][c]), int(e["q_count"][c])
        for k in pool:  # q_first legitimately differs: append_frames always compacts
            assert np.array_equal(exp["pool"][k][a:a + n], pool2[k][b:b + n]), (c, k)
    mask = C.live_mask(exp, cap, len(pool["off"]))
    untouched = mask & ~np.repeat(sent, cap)
    for k in pool:
        assert np.array_equal(exp["pool"][k][untouched], pool[k][untouched])


@pytest.mark.parametrize("seed", range(12))
def test_every_frame_of_a_buffer_but_its_last_carries_mss(seed):
    """What the kernels' closed form rests on: a window-limited short frame closes the window, so nothing follows it,
    and the payload bytes of b's frames before f are (f - first_frame[b]) * (len_out[first_frame[b]] - 54)."""
    push, seg, tx, _, _, _ = random_case(seed)
    pc, po, _ = push
    flen = seg["len_out"].astype(np.int64) - 54
    for b in range(len(pc)):
        f0, n = int(seg["first_frame"][b]), int(seg["frame_count"][b])
        if seg["status"][b] in (M.SENT, M.PARTIAL):
            assert (flen[f0:f0 + n - 1] == int(tx["mss"][pc[b]])).all(), b
    f = np.arange(len(flen))
    ff = seg["first_frame"].astype(np.int64)[seg["frame_buf"]]
    closed = (po.astype(np.int64)[seg["frame_buf"]] + (f - ff) * flen[ff]) & 0xFFFFFFFF
    _, off, lens = A.sent_entries(push, seg)
    assert np.array_equal(closed, off) and np.array_equal(lens, flen)


def hand(q_first, q_count, k, cap=10, c=1, nconns=3, armed=0, now=NOW):
    """Connection c of nconns pushes one buffer that became k frames of 5 bytes (the last 2); the others push nothing."""
    ak = ack_conn_table(nconns, q_first=[0, q_first, 999][:nconns], q_count=[0, q_count, 0][:nconns])
    ak["rtx_armed"][c], ak["rtx_base_ns"][c] = armed, 123
    nq = nconns * cap + 4
    pool = {"off": np.arange(nq, dtype=np.uint32) + 1000, "len": np.arange(nq, dtype=np.uint32) + 2000,
            "tx_time": np.arange(nq, dtype=np.uint64) + 3000}
    res = {"status": np.array([C.SENT]), "first_frame": np.array([0]), "frame_count": np.array([k]),
           "len_out": np.array([59] * (k - 1) + [56], np.uint16)}
    return ak, pool, C.tx_commit([c], [400], res, ak, pool, cap, now), cap


def test_placement_rule_at_its_edges():
    # exactly to the region's end: in place
    ak, pool, e, cap = hand(q_first=13, q_count=4, k=3)
    assert (e["status"][1], e["appended"][1], e["ack_conns"]["q_first"][1], e["ack_conns"]["q_count"][1]) == (0, 3, 13, 7)
    assert e["pool"]["off"][17:20].tolist() == [400, 405, 410] and e["pool"]["len"][17:20].tolist() == [5, 5, 2]
    assert (e["pool"]["tx_time"][17:20] == NOW).all() and np.array_equal(e["pool"]["off"][:17], pool["off"][:17])
    assert (e["ack_conns"]["rtx_armed"][1], e["ack_conns"]["rtx_base_ns"][1]) == (1, NOW)
    # one more frame: the live entries move to the region's start, in order
    ak, pool, e, cap = hand(q_first=13, q_count=4, k=4)
    assert (e["ack_conns"]["q_first"][1], e["ack_conns"]["q_count"][1]) == (10, 8)
    assert e["pool"]["off"][10:18].tolist() == [1013, 1014, 1015, 1016, 400, 405, 410, 415]
    assert e["pool"]["tx_time"][10:14].tolist() == [3013, 3014, 3015, 3016]
    # an empty queue restarts at the region's start, whatever q_first said
    ak, pool, e, cap = hand(q_first=4_000_000_000, q_count=0, k=2)
    assert (e["status"][1], e["ack_conns"]["q_first"][1], e["ack_conns"]["q_count"][1]) == (0, 10, 2)
    # full to the brim is fine, one more is E_FULL and changes nothing
    ak, pool, e, cap = hand(q_first=12, q_count=6, k=4)
    assert (e["status"][1], e["ack_conns"]["q_count"][1], e["ack_conns"]["q_first"][1]) == (0, 10, 10)
    ak, pool, e, cap = hand(q_first=12, q_count=6, k=5)
    assert (e["status"][1], e["appended"][1]) == (C.E_FULL, 0) and e["ack_conns"].tobytes() == ak.tobytes()
    assert all(np.array_equal(e["pool"][k], pool[k]) for k in pool)
    # E_QUEUE: more entries than the region holds; a live range that starts before or ends behind the region
    for qf, qc in ((10, 11), (9, 3), (18, 3), (4_294_967_290, 8)):
        ak, pool, e, cap = hand(q_first=qf, q_count=qc, k=1)
        assert (e["status"][1], e["appended"][1]) == (C.E_QUEUE, 0) and e["ack_conns"].tobytes() == ak.tobytes(), (qf, qc)
    # an armed timer, whatever nonzero value says so, keeps its base
    ak, pool, e, cap = hand(q_first=10, q_count=1, k=1, armed=7)
    assert (e["ack_conns"]["rtx_armed"][1], e["ack_conns"]["rtx_base_ns"][1]) == (7, 123)
    # rows without frames are never touched, malformed ones included (connection 2's q_first is 999)
    assert e["ack_conns"][[0, 2]].tobytes() == ak[[0, 2]].tobytes() and e["status"].tolist() == [0, 0, 0]


def test_dack_rule():
    dack = np.zeros(3, N.DACK_CONN_DTYPE)
    dack["armed"], dack["deadline_ns"], dack["delay_ns"] = [1, 5, 1], [11, 12, 13], 40
    ak, pool, _, cap = hand(q_first=12, q_count=6, k=5)  # E_FULL: the frames left all the same
    res = {"status": np.array([C.SENT]), "first_frame": np.array([0]), "frame_count": np.array([5]),
           "len_out": np.array([59] * 5, np.uint16)}
    e = C.tx_commit([1], [0], res, ak, pool, cap, NOW, dack=dack)
    assert e["status"][1] == C.E_FULL and e["dack"]["armed"].tolist() == [1, 0, 1]
    assert e["dack"]["deadline_ns"].tolist() == [11, 12, 13] and e["dack"][[0, 2]].tobytes() == dack[[0, 2]].tobytes()
    d = C.rtx_piggyback([N.DK_TCP_RTX_SENT, N.DK_TCP_RTX_IDLE, N.DK_TCP_RTX_NO_ROOM], dack)
    assert d["armed"].tolist() == [0, 5, 1] and d["deadline_ns"].tolist() == [11, 12, 13]


# ---------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_commit_struct_layout_matches_ctypes(tmp_path):
    structs = {"dk_tcp_commit_out": N.DkTcpCommitOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, (cname, fname)


def test_commit_constants_match_header():
    hdr = open(HEADER).read()
    for i, name in enumerate(N.TCP_COMMIT_STATUSES):
        assert re.search(rf"DK_TCP_COMMIT_{name} = {i}[,\s]", hdr), name
        assert getattr(N, f"DK_TCP_COMMIT_{name}") == i == getattr(tcp_commit, name) == getattr(C, name)
    assert (C.SENT, C.PARTIAL, C.RTX_SENT) == (N.DK_TCP_TX_SENT, N.DK_TCP_TX_PARTIAL, N.DK_TCP_RTX_SENT)
    assert C.NONE == N.DK_TCP_TX_TIME_NONE
    assert "#define DK_RX_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "dk_rx.h")).read()  # additive
    lib = N.load_library()
    for fn in ("dk_tcp_tx_commit", "dk_tcp_rtx_piggyback", "dk_diag_tcp_commit_set_form",
               "dk_diag_tcp_commit_last_form"):
        assert getattr(lib, fn)
    diag = open(os.path.join(ROOT, "include", "dk_diag.h")).read()
    assert "dk_diag_tcp_commit_set_form" in diag and "dk_diag_tcp_commit_last_form" in diag


def test_null_pointers_and_bad_arguments_are_einval():
    lib = N.load_library()
    p, r, q, o, rr = N.DkTcpTxPush(), N.DkTcpTxResults(), N.DkTcpUnacked(), N.DkTcpCommitOut(), N.DkTcpRtxResults()
    ref = ctypes.byref
    commit = lib.dk_tcp_tx_commit
    assert commit(None, ref(p), 0, ref(r), 0, None, 0, ref(q), 0, 0, None, 1, ref(o), None) == errno.EINVAL
    assert commit(None, None, 0, None, 0, None, 0, None, 0, 0, None, 1, None, None) == errno.EINVAL
    assert commit(None, ref(p), 0, ref(r), 0, None, 4, ref(q), 7, 2, None, 1, ref(o), None) == errno.EINVAL  # 4 * 2 > 7
    assert commit(None, ref(p), 0, ref(r), 0, None, 1 << 31, ref(q), 0xFFFFFFFF, 4, None, 1, ref(o), None) == errno.EINVAL
    assert commit(None, ref(p), 0, ref(r), 0, None, 0, ref(q), 0, 0, None, N.DK_TCP_TX_TIME_NONE, ref(o), None) == errno.EINVAL
    assert lib.dk_tcp_rtx_piggyback(None, ref(rr), None, 0, None) == errno.EINVAL
    assert lib.dk_tcp_rtx_piggyback(None, None, None, 0, None) == errno.EINVAL
    assert lib.dk_diag_tcp_commit_set_form(None, 0) == errno.EINVAL
    assert lib.dk_diag_tcp_commit_last_form(None) == -1
