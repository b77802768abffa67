"""dk_tcp_tx_segment on the CPU: the ABI additions (struct layouts, constants, the frame bound helper) and the pinning
of tests/tx_segment_reference.py, the plain-Python send_segment loop the GPU tests compare against: hand-written cases
from sender.rs, and its frames through the receive oracle and the TCP oracle, whose delivered views must read back the
pushed bytes. No GPU work."""
import ctypes
import os
import re
import subprocess

import numpy as np

import tx_segment_reference as M
from demikernel_amd import _native as N
from demikernel_amd import ipv4, synth
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_tx import frame_bound, tx_conn_table
from oracle import oracle as O
from oracle.oracle import OraclePeer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_tcp.h")


def test_tcp_tx_struct_layout_matches_ctypes(tmp_path):
    """sizeof / offsetof from the C compiler == the ctypes mirrors and the numpy connection record."""
    structs = {"dk_tcp_tx_conn": N.DkTcpTxConn, "dk_tcp_tx_push": N.DkTcpTxPush, "dk_tcp_tx_layout": N.DkTcpTxLayout,
               "dk_tcp_tx_results": N.DkTcpTxResults}
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
    assert ctypes.sizeof(N.DkTcpTxConn) == N.TX_CONN_DTYPE.itemsize == 64
    for fname, _ in N.DkTcpTxConn._fields_:
        assert N.TX_CONN_DTYPE.fields[fname][1] == getattr(N.DkTcpTxConn, fname).offset, fname
    assert [f for f, _ in N.DkTcpTxResults._fields_] == N.TCP_TX_RESULT_FIELDS


def test_tcp_tx_constants_match_header():
    hdr = open(HEADER).read()
    for i, name in enumerate(N.TCP_TX_STATUSES):
        assert re.search(rf"DK_TCP_TX_{name} = {i}[,\s]", hdr), name
        assert getattr(N, f"DK_TCP_TX_{name}") == i == getattr(M, name)
    assert M.ESTABLISHED == N.DK_TCP_ESTABLISHED
    assert "#define DK_RX_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "dk_rx.h")).read()
    lib = N.load_library()
    assert lib.dk_tcp_tx_segment and lib.dk_tcp_tx_ctx_create and lib.dk_diag_tcp_tx_set_grid


def test_frame_bound():
    """sum of max(1, ceil(len / mss)); markers count one frame; mss 0 never sends."""
    lens = [0, 1, 1459, 1460, 1461, 2920, 4387, 0xFFFFFFFF]
    want = sum(max(1, -(-l // 1460)) for l in lens)
    assert frame_bound(lens, 1460) == want == 1 + 1 + 1 + 1 + 2 + 2 + 4 + 2941759
    assert frame_bound(lens, 1) == sum(max(1, l) for l in lens)
    assert frame_bound([], 1460) == 0 and frame_bound(lens, 0) == 0
    # it bounds the model's need for any window
    src, conn, off, ln = M.pack_push([0, 0, 0, 1], [5000, 0, 7, 1461])
    tx = tx_conn_table(2, snd_wnd=1 << 20, mss=[536, 1460])
    r = M.segment(src, conn, off, ln, tx, M.links_table(), np.zeros(1 << 16, np.uint8), slot_stride=1536, frame_lead=0,
                  max_frames=64)
    assert r["n_frames"] <= frame_bound(ln, 536)


def _cb(**kw):
    c = dict(snd_una=1000, snd_nxt=1000, snd_wnd=65535, cwnd=0xFFFFFFFF, mss=1460)
    c.update(kw)
    return c


def test_send_segment_hand_cases():
    """sender.rs:124-208 by hand."""
    # a buffer larger than the open window: `open` bytes, PSH suppressed, the rest stays
    c = _cb()
    assert M.send_segment(4000, False, c) == (1460, 1000, M.ACK, 1460) and c["snd_nxt"] == 2460
    assert M.send_segment(2540, False, c) == (1460, 2460, M.ACK, 1460)
    # the piece that ends the buffer carries PSH
    assert M.send_segment(1080, False, c) == (1080, 3920, M.ACK | M.PSH, 1080) and c["snd_nxt"] == 5000
    # a buffer of exactly `open` bytes is not "larger": PSH
    c = _cb()
    assert M.send_segment(1460, False, c) == (1460, 1000, M.ACK | M.PSH, 1460)
    c = _cb(snd_wnd=700)
    assert M.send_segment(700, False, c) == (700, 1000, M.ACK | M.PSH, 700)
    assert M.send_segment(1, False, c) is None  # and the window is then full
    # the end-of-send marker: FIN, one sequence number
    c = _cb()
    assert M.send_segment(0, True, c) == (0, 1000, M.ACK | M.FIN, 1) and c["snd_nxt"] == 1001
    # window 0, window < in flight, cwnd < in flight: nothing, not even a FIN
    for kw in (dict(snd_wnd=0), dict(snd_wnd=99, snd_nxt=1100), dict(cwnd=99, snd_nxt=1100), dict(mss=0)):
        c = _cb(**kw)
        assert M.send_segment(10, False, c) is None and M.send_segment(0, True, c) is None
        assert c["snd_nxt"] == kw.get("snd_nxt", 1000)
    # in flight counts against both windows; cwnd can be the binding limit
    c = _cb(snd_nxt=1100, snd_wnd=5000, cwnd=600)
    assert M.open_window(1000, 1100, 5000, 600, 1460) == 500
    assert M.send_segment(900, False, c) == (500, 1100, M.ACK, 500)
    assert M.send_segment(400, False, c) is None
    # sequence numbers wrap
    c = _cb(snd_una=0xFFFFFF00, snd_nxt=0xFFFFFF00)
    assert M.send_segment(1460, False, c) == (1460, 0xFFFFFF00, M.ACK | M.PSH, 1460) and c["snd_nxt"] == 1460 - 256
    assert M.open_window(0xFFFFFF00, c["snd_nxt"], 65535, 0xFFFFFFFF, 1460) == 1460


def test_header_window():
    rx = conn_table(1, receive_next=5000, buffer_size=65535)[0]
    assert M.header_window(rx, 0) == 65535
    rx["reader_next"] = 4000  # 1000 bytes unread
    assert M.header_window(rx, 0) == 64535 and M.header_window(rx, 3) == 64535 >> 3
    rx["buffer_size"] = 1 << 20
    # 1,047,576 bytes of window: 130,947 at shift 3 does not fit 16 bits, 65,473 at shift 4 does
    assert M.header_window(rx, 0) is None and M.header_window(rx, 3) is None and M.header_window(rx, 4) == 65473


def test_batch_contract_by_hand():
    """Statuses, frame numbering, FIN and the all-or-nothing capacity rule on a three-connection push list."""
    flows = synth.make_flows(3, passive=False)
    tx = M.conns_toward(flows, snd_wnd=[4000, 1 << 20, 1 << 20], mss=1000, snd_nxt=[10, 20, 30], rcv_nxt=7,
                        rcv_wnd_hdr=99)
    tx["state"][2] = N.DK_TCP_CLOSED
    #        conn 0: 2500 (3 frames), 2000 (1500 fit: 2 frames, partial), 5 (unsent)
    #        conn 1: 10, marker, 10 (closed)      conn 2: not established
    src, conn, off, ln = M.pack_push([0, 0, 0, 1, 1, 1, 2], [2500, 2000, 5, 10, 0, 10, 4])
    out = np.full(16 * 1536, 0xA5, np.uint8)
    r = M.segment(src, conn, off, ln, tx, M.links_table(), out, slot_stride=1536, frame_lead=2, max_frames=16)
    assert r["n_frames"] == 7
    assert list(r["status"]) == [M.SENT, M.PARTIAL, M.UNSENT, M.SENT, M.SENT, M.CLOSED, M.E_CONN]
    assert list(r["sent"]) == [2500, 1500, 0, 10, 1, 0, 0]
    assert list(r["first_frame"]) == [0, 3, 5, 5, 6, 7, 7] and list(r["frame_count"]) == [3, 2, 0, 1, 1, 0, 0]
    assert list(r["frame_buf"]) == [0, 0, 0, 1, 1, 3, 4]
    assert list(r["len_out"]) == [1054, 1054, 554, 1054, 554, 64, 54]
    assert list(r["off_out"]) == [f * 1536 + 2 for f in range(7)]
    assert list(r["tx_conns"]["snd_nxt"]) == [4010, 31, 30] and list(r["tx_conns"]["fin_sent"]) == [0, 1, 0]
    flags = [int(r["out"][o + 47]) for o in r["off_out"]]
    assert flags == [M.ACK, M.ACK, M.ACK | M.PSH, M.ACK, M.ACK, M.ACK | M.PSH, M.ACK | M.FIN]
    seqs = [int.from_bytes(r["out"][o + 38:o + 42].tobytes(), "big") for o in r["off_out"]]
    assert seqs == [10, 1010, 2010, 2510, 3510, 20, 30]
    assert all(int.from_bytes(r["out"][o + 42:o + 46].tobytes(), "big") == 7 for o in r["off_out"])
    assert all(int.from_bytes(r["out"][o + 48:o + 50].tobytes(), "big") == 99 for o in r["off_out"])
    # nothing outside the frames
    mask = np.ones(out.size, bool)
    for o, l in zip(r["off_out"], r["len_out"]):
        mask[o:o + l] = False
    assert (r["out"][mask] == 0xA5).all()
    # one frame short, in frames or in bytes: the need is reported, nothing moves
    for kw in (dict(max_frames=6), dict(max_frames=16, out_bytes=7 * 1536 - 1)):
        s = M.segment(src, conn, off, ln, tx, M.links_table(), out, slot_stride=1536, frame_lead=2, **kw)
        assert s["n_frames"] == 7 and (s["out"] == 0xA5).all() and np.array_equal(s["tx_conns"], tx)
        assert list(s["status"]) == [M.NO_ROOM, M.NO_ROOM, M.UNSENT, M.NO_ROOM, M.NO_ROOM, M.CLOSED, M.E_CONN]
        assert not s["sent"].any() and len(s["off_out"]) == 0
        assert list(s["first_frame"]) == list(r["first_frame"]) and list(s["frame_count"]) == list(r["frame_count"])


def test_frames_deliver_the_pushed_bytes_through_the_oracles():
    """The model's frames through the receive oracle (every checksum verified) and the TCP oracle: every frame is
    delivered, and per connection the delivered views concatenate to the bytes that were pushed (then EOF where a FIN
    went out)."""
    nconns = 5
    flows = synth.make_flows(nconns, passive=False)
    rng = np.random.default_rng(11)
    conn = np.sort(rng.integers(0, nconns, 40)).astype(np.uint32)
    lens = rng.choice([1, 2, 99, 535, 536, 537, 1072, 3000], 40)
    fin_at = {1: None, 3: None}
    conn = np.concatenate([conn, [1, 3]])
    lens = np.concatenate([lens, [0, 0]])
    order = np.argsort(conn, kind="stable")
    conn, lens = conn[order], lens[order]
    src, conn, off, ln = M.pack_push(conn, lens, residues=rng.integers(0, 16, len(lens)))
    tx = M.conns_toward(flows, mss=536)
    frames_max = frame_bound(ln, 536)
    out = np.zeros(frames_max * 640, np.uint8)
    r = M.segment(src, conn, off, ln, tx, M.links_table(), out, slot_stride=640, frame_lead=3, max_frames=frames_max)
    assert (r["status"] == M.SENT).all() and r["n_frames"] == frames_max
    peer = OraclePeer(ipv4(synth.BOB_IPV4))
    peer.set_flows(flows)
    rx = peer.process(r["out"], r["off_out"], r["len_out"])
    assert ((rx["meta"] & 0xFF) == N.V["OK_TCP"]).all()
    assert np.array_equal(rx["flow_id"], conn[r["frame_buf"]])
    table = conn_table(nconns, receive_next=tx["snd_nxt"], send_next=tx["rcv_nxt"], buffer_size=1 << 20)
    t = O.tcp_process(table, rx)
    assert set(np.unique(t["action"])) <= {N.A["DELIVERED"], N.A["FIN"]}
    for c in range(nconns):
        a, k = int(t["deliv_start"][c]), int(t["deliv_count"][c])
        got = b""
        for v in t["deliv"][a:a + k]:
            if v["ref"] != N.DK_TCP_REF_EOF:
                o = int(r["off_out"][v["ref"]]) + int(v["off"])
                got += r["out"][o:o + int(v["len"])].tobytes()
        want = b"".join(src[int(off[b]):int(off[b]) + int(ln[b])].tobytes() for b in np.nonzero(conn == c)[0])
        assert got == want, c
        assert (int(table["receive_next"][c]) - int(tx["snd_nxt"][c])) % 2**32 == len(want) + (c in fin_at)
        assert table["receive_next"][c] == r["tx_conns"]["snd_nxt"][c]
