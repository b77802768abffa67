"""The ABI additions of the active-open section of include/dk_tcp.h on the CPU: struct layouts against the C compiler,
constants against the header, the symbols, and the argument rules that need no device."""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np

import demikernel_amd
from demikernel_amd import _native as N
from demikernel_amd import tcp_connect as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_tcp.h")


def test_connect_struct_layout_matches_ctypes(tmp_path):
    structs = {"dk_tcp_connector": N.DkTcpConnector, "dk_tcp_isn_gen": N.DkTcpIsnGen, "dk_tcp_con_ready": N.DkTcpConReady,
               "dk_tcp_con_results": N.DkTcpConResults}
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
    for cname, dt in (("dk_tcp_connector", N.CONNECTOR_DTYPE), ("dk_tcp_isn_gen", N.ISN_GEN_DTYPE),
                      ("dk_tcp_con_ready", N.CON_READY_DTYPE)):
        assert int(got[cname]) == dt.itemsize
        for fname in dt.names:
            assert int(got[f"{cname}.{fname}"]) == dt.fields[fname][1], (cname, fname)
    assert (int(got["dk_tcp_connector"]), int(got["dk_tcp_isn_gen"]), int(got["dk_tcp_con_ready"])) == (64, 8, 48)


def test_connect_constants_match_header():
    hdr = open(HEADER).read()
    for names in (N.TCP_CON_STATES, N.TCP_CON_ACTIONS, N.TCP_CON_CAUSES, N.TCP_CON_STATUSES):
        for i, name in enumerate(names):
            assert re.search(rf"DK_TCP_CON_{name} = {i}[,\s]", hdr), name
            assert getattr(TC, name) == i
    for name, val in (("NONE", "0xFFFFFFFFu"), ("FALLBACK_MSS", "536u"), ("SYN_BYTES", "62u"), ("ACK_BYTES", "54u")):
        assert re.search(rf"#define DK_TCP_CON_{name} {val}\s", hdr), name
        assert getattr(N, f"DK_TCP_CON_{name}") == int(val.rstrip("u"), 0)
    assert "#define DK_RX_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "dk_rx.h")).read()  # additive
    lib = N.load_library()
    for fn, _, _ in N.TCP_CONNECT_FUNCTIONS:
        assert getattr(lib, fn)
    for name in ("connector_table", "conn_of_flow", "ConnectResults", "connect_start", "connect_process", "connect_timers",
                 "conn_rows_from_connect_ready"):
        assert getattr(demikernel_amd, name) is getattr(TC, name)


def test_host_tables():
    rows = TC.connector_table(3, flow_id=[4, 2, 7], local_port=[1, 2, 3])
    assert list(rows["state"]) == [TC.IDLE] * 3 and list(rows["handshake_retries"]) == [5] * 3
    m = TC.conn_of_flow(9, rows)
    assert list(m) == [TC.NONE, TC.NONE, 1, TC.NONE, 0, TC.NONE, TC.NONE, 2, TC.NONE]
    r = np.zeros(1, TC.READY_DTYPE)[0]
    r["rcv_nxt"], r["snd_nxt"], r["local_window"], r["remote_window"], r["mss"], r["local_wscale"] = 11, 22, 4096, 800, 1400, 3
    rows["remote_ip"], rows["remote_port"], rows["local_ip"] = 0x0100000A, 443, 0x0200000A
    rx, tx = TC.conn_rows_from_connect_ready(r, rows[1])
    assert (rx["receive_next"][0], rx["reader_next"][0], rx["send_next"][0], rx["buffer_size"][0]) == (11, 11, 22, 4096)
    assert (tx["snd_una"][0], tx["snd_nxt"][0], tx["snd_wnd"][0], tx["mss"][0], tx["rcv_wscale"][0]) == (22, 22, 800, 1400, 3)
    assert tx["ports"][0] == 2 | 443 << 16 and tx["remote_ip"][0] == 0x0100000A and tx["rcv_wnd_hdr"][0] == 512


def test_argument_rules_without_a_device():
    """EINVAL before any GPU work: null required pointers, misaligned rows, n >= 2^31, out_bytes over the limit,
    nlinks == 0."""
    lib = N.load_library()
    r, o, lay = N.DkRxResults(), N.DkTcpConResults(), N.DkTcpTxLayout(64, 0)
    words = (ctypes.c_uint32 * 2)()
    ok = N.DkTcpConResults(n_frames=ctypes.addressof(words), n_ready=ctypes.addressof(words) + 4)
    buf = (ctypes.c_uint8 * 256)()
    a = (ctypes.addressof(buf) + 63) & ~63  # a 64-byte aligned address: never dereferenced by the checks
    E = errno.EINVAL
    L, R_, O = ctypes.byref(lay), ctypes.byref(r), ctypes.byref(ok)
    big = 0xFFFFFF00 + 1  # DK_RX_MAX_BLOB + 1
    # dk_tcp_connect_start
    start = lib.dk_tcp_connect_start
    assert start(None, 0, None, 0, a, a, 1, 0, None, 0, L, 0, 0, 0, ctypes.byref(o), None) == E   # null n_frames / n_ready
    assert start(None, 0, None, 0, a, a, 1, 0, None, 0, None, 0, 0, 0, O, None) == E              # null layout
    assert start(None, 0, None, 0, a, a, 1, 0, None, 0, L, 0, 0, 0, None, None) == E              # null results
    assert start(None, 0, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E              # null isn_gen
    assert start(None, 0, None, 0, a, None, 1, 0, None, 0, L, 0, 0, 0, O, None) == E              # null links
    assert start(None, 0, None, 0, a, a, 0, 0, None, 0, L, 0, 0, 0, O, None) == E                 # nlinks == 0
    assert start(None, 1, None, 0, a, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                 # null rows
    assert start(a + 8, 1, None, 0, a, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                # misaligned rows
    assert start(a, 1, None, 1, a, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                    # null start[]
    assert start(a, 1, a, 1 << 31, a, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                 # nstart >= 2^31
    assert start(a, 1, a, 1, a, a, 1, 0, None, big, L, 0, 0, 0, O, None) == E                     # out_bytes
    assert start(a, 1, a, 1, a, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                       # null status
    # dk_tcp_connect_process
    proc = lib.dk_tcp_connect_process
    assert proc(None, 0, None, 0, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E      # null rx
    assert proc(R_, 0, None, 0, None, 0, None, None, 1, 0, None, 0, L, 0, 0, 0, O, None) == E     # null links
    assert proc(R_, 0, None, 0, None, 0, None, a, 0, 0, None, 0, L, 0, 0, 0, O, None) == E        # nlinks == 0
    assert proc(R_, 0, a + 4, 1, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E       # misaligned rows
    assert proc(R_, 1 << 31, None, 0, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E  # n >= 2^31
    assert proc(R_, 0, None, 0, None, 0, None, a, 1, 0, None, big, L, 0, 0, 0, O, None) == E      # out_bytes
    assert proc(R_, 1, None, 0, None, 0, None, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E        # null rx arrays
    assert proc(R_, 0, None, 0, None, 0, None, a, 1, 0, None, 0, None, 0, 0, 0, O, None) == E     # null layout
    # dk_tcp_connect_timers
    tim = lib.dk_tcp_connect_timers
    assert tim(None, 0, None, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                            # null links
    assert tim(None, 0, a, 0, 0, None, 0, L, 0, 0, 0, O, None) == E                               # nlinks == 0
    assert tim(None, 1, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                               # null rows
    assert tim(a + 1, 1, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                              # misaligned rows
    assert tim(a, 1, a, 1, 0, None, big, L, 0, 0, 0, O, None) == E                                # out_bytes
    assert tim(a, 1, a, 1, 0, None, 0, L, 0, 0, 0, O, None) == E                                  # null status
    assert tim(None, 0, a, 1, 0, None, 0, L, 0, 0, 0, None, None) == E                            # null results
