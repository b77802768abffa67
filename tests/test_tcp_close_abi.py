"""The ABI additions of the close section of include/dk_tcp.h on the CPU: struct layouts against the C compiler,
constants against the header, the symbols, and the argument rules that need no device."""
import ctypes
import errno
import os
import re
import subprocess

import demikernel_amd
from demikernel_amd import _native as N
from demikernel_amd import tcp_close as TCL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_tcp.h")


def test_close_struct_layout_matches_ctypes(tmp_path):
    structs = {"dk_tcp_closer": N.DkTcpCloser, "dk_tcp_cls_done": N.DkTcpClsDone, "dk_tcp_cls_results": N.DkTcpClsResults}
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
    for cname, dt in (("dk_tcp_closer", N.CLOSER_DTYPE), ("dk_tcp_cls_done", N.CLS_DONE_DTYPE)):
        assert int(got[cname]) == dt.itemsize
        for fname in dt.names:
            assert int(got[f"{cname}.{fname}"]) == dt.fields[fname][1], (cname, fname)
    assert (int(got["dk_tcp_closer"]), int(got["dk_tcp_cls_done"])) == (32, 32)


def test_close_constants_match_header():
    hdr = open(HEADER).read()
    for names in (N.TCP_CLS_STATES, N.TCP_CLS_STATUSES):
        for i, name in enumerate(names):
            assert re.search(rf"DK_TCP_CLS_{name} = {i}[,\s]", hdr), name
            assert getattr(TCL, name) == i
    assert [TCL.STATES.index(s) for s in ("IDLE", "FIN_WAIT_1", "FIN_WAIT_2", "CLOSING", "TIME_WAIT", "LAST_ACK", "CLOSED",
                                          "FAULT")] == list(range(8))
    for name, bit in N.TCP_CLS_ACTION_BITS.items():
        assert re.search(rf"#define DK_TCP_CLS_{name} {bit}u\s", hdr), name
        assert getattr(TCL, name) == bit
    assert N.TCP_CLS_ACTION_BITS == {"POPPED": 1, "ACK_OK": 2, "ACK_UNSENT": 4, "FIN": 8, "FAULT_BIT": 16, "UNPROCESSED": 32}
    for name, val in (("NONE", "0xFFFFFFFFu"), ("TIME_WAIT_NS", "4000000000ull"), ("RETIRED", "1u"), ("ACK_BYTES", "54u")):
        assert re.search(rf"#define DK_TCP_CLS_{name} {val}\s", hdr), name
        assert getattr(N, f"DK_TCP_CLS_{name}") == int(val.rstrip("ul"), 0)
    assert "#define DK_RX_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "dk_rx.h")).read()  # additive
    lib = N.load_library()
    assert lib.dk_rx_abi_version() == 4
    for fn, _, _ in N.TCP_CLOSE_FUNCTIONS:
        assert getattr(lib, fn)
    for name in ("closer_table", "close_start", "close_process", "close_timers", "CloseResults"):
        assert getattr(demikernel_amd, name) is getattr(TCL, name)
    assert "Not modelled: the persist timer" in hdr and "FIN-WAIT / LAST-ACK" not in hdr


def test_host_table():
    rows = TCL.closer_table(3, linger_ns=[1, 2, 3])
    assert list(rows["state"]) == [TCL.IDLE] * 3 and list(rows["linger_ns"]) == [1, 2, 3]
    assert list(TCL.closer_table(2)["linger_ns"]) == [4_000_000_000] * 2


def test_argument_rules_without_a_device():
    """EINVAL before any GPU work: null required pointers, misaligned tables, n or nclose >= 2^31, out_bytes over the
    limit, nlinks == 0."""
    lib = N.load_library()
    r, lay = N.DkRxResults(), N.DkTcpTxLayout(64, 0)
    words = (ctypes.c_uint32 * 2)()
    w0, w1 = ctypes.addressof(words), ctypes.addressof(words) + 4
    buf = (ctypes.c_uint8 * 256)()
    a = (ctypes.addressof(buf) + 63) & ~63  # a 64-byte aligned address: never dereferenced by the checks
    ok = N.DkTcpClsResults(n_frames=w0, n_done=w1, status=a, fin_frame=a)
    E = errno.EINVAL
    L, R_, O = ctypes.byref(lay), ctypes.byref(r), ctypes.byref(ok)
    big = 0xFFFFFF00 + 1  # DK_RX_MAX_BLOB + 1
    # dk_tcp_close_start(rows, rx_conns, tx_conns, nconns, close, nclose, status, push_conn, push_off, push_len, n_markers, s)
    start = lib.dk_tcp_close_start
    assert start(None, None, None, 0, None, 0, None, None, None, None, None, None) == E       # null n_markers
    assert start(None, a, a, 1, None, 0, None, None, None, None, w0, None) == E               # null rows
    assert start(a, None, a, 1, None, 0, None, None, None, None, w0, None) == E               # null rx_conns
    assert start(a, a, None, 1, None, 0, None, None, None, None, w0, None) == E               # null tx_conns
    assert start(a + 8, a, a, 1, None, 0, None, None, None, None, w0, None) == E              # misaligned rows
    assert start(a, a + 4, a, 1, None, 0, None, None, None, None, w0, None) == E              # misaligned rx_conns
    assert start(a, a, a + 2, 1, None, 0, None, None, None, None, w0, None) == E              # misaligned tx_conns
    assert start(a, a, a, 1, None, 1, a, a, a, a, w0, None) == E                              # null close[]
    assert start(a, a, a, 1, a, 1, None, a, a, a, w0, None) == E                              # null status
    assert start(a, a, a, 1, a, 1, a, None, a, a, w0, None) == E                              # null push_conn
    assert start(a, a, a, 1, a, 1, a, a, None, a, w0, None) == E                              # null push_off
    assert start(a, a, a, 1, a, 1, a, a, a, None, w0, None) == E                              # null push_len
    assert start(a, a, a, 1, a, 1 << 31, a, a, a, a, w0, None) == E                           # nclose >= 2^31
    # dk_tcp_close_process(rx, n, rows, rx_conns, tx_conns, dack, nconns, action_in, links, nlinks, now, out, out_bytes,
    #                      layout, max_frames, max_done, flags, results, stream)
    proc = lib.dk_tcp_close_process
    assert proc(None, 0, None, None, None, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E       # null rx
    assert proc(R_, 0, None, None, None, None, 0, None, None, 1, 0, None, 0, L, 0, 0, 0, O, None) == E      # null links
    assert proc(R_, 0, None, None, None, None, 0, None, a, 0, 0, None, 0, L, 0, 0, 0, O, None) == E         # nlinks == 0
    assert proc(R_, 0, None, None, None, None, 0, None, a, 1, 0, None, 0, None, 0, 0, 0, O, None) == E      # null layout
    assert proc(R_, 0, None, None, None, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, None, None) == E      # null results
    none = N.DkTcpClsResults(status=a, fin_frame=a)
    assert proc(R_, 0, None, None, None, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, ctypes.byref(none), None) == E
    assert proc(R_, 0, None, None, None, None, 0, None, a, 1, 0, None, big, L, 0, 0, 0, O, None) == E       # out_bytes
    assert proc(R_, 1 << 31, None, None, None, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E   # n >= 2^31
    assert proc(R_, 0, None, a, a, None, 1, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E               # null rows
    assert proc(R_, 0, a, None, a, None, 1, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E               # null rx_conns
    assert proc(R_, 0, a, a, None, None, 1, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E               # null tx_conns
    nostat = N.DkTcpClsResults(n_frames=w0, n_done=w1, fin_frame=a)
    assert proc(R_, 0, a, a, a, None, 1, None, a, 1, 0, None, 0, L, 0, 0, 0, ctypes.byref(nostat), None) == E
    nofin = N.DkTcpClsResults(n_frames=w0, n_done=w1, status=a)
    assert proc(R_, 0, a, a, a, None, 1, None, a, 1, 0, None, 0, L, 0, 0, 0, ctypes.byref(nofin), None) == E
    assert proc(R_, 0, a + 8, a, a, None, 1, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E              # misaligned rows
    assert proc(R_, 0, a, a + 4, a, None, 1, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E              # ... rx_conns
    assert proc(R_, 0, a, a, a + 2, None, 1, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E              # ... tx_conns
    assert proc(R_, 0, a, a, a, a + 1, 1, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                 # ... dack
    assert proc(R_, 1, None, None, None, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E         # null rx arrays
    full = N.DkRxResults(meta=a, flow_id=a, tcp_seq=a, tcp_ack=a)
    assert proc(ctypes.byref(full), 1, None, None, None, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E  # per-frame
    for missing in ("meta", "flow_id", "tcp_seq", "tcp_ack"):
        part = N.DkRxResults(**{k: a for k in ("meta", "flow_id", "tcp_seq", "tcp_ack") if k != missing})
        allout = N.DkTcpClsResults(n_frames=w0, n_done=w1, status=a, fin_frame=a, action=a, state_after=a, ack_action=a,
                                   reply_frame=a)
        assert proc(ctypes.byref(part), 1, None, None, None, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0,
                    ctypes.byref(allout), None) == E, missing
    # dk_tcp_close_timers(rows, tx_conns, nconns, now, done, max_done, n_done, status, stream)
    tim = lib.dk_tcp_close_timers
    assert tim(None, None, 0, 0, None, 0, None, None, None) == E                                            # null n_done
    assert tim(None, None, 1, 0, None, 0, w0, a, None) == E                                                 # null rows
    assert tim(a, None, 1, 0, None, 0, w0, None, None) == E                                                 # null status
    assert tim(a, None, 1, 0, None, 1, w0, a, None) == E                                                    # null done
    assert tim(a + 8, None, 1, 0, a, 1, w0, a, None) == E                                                   # misaligned rows
    assert tim(a, a + 4, 1, 0, a, 1, w0, a, None) == E                                                      # ... tx_conns
