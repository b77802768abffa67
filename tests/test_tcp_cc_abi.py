"""The ABI additions of the congestion-control section of include/dk_tcp.h on the CPU: struct layouts against the C
compiler, constants against the header, the symbols, and EINVAL for null pointers (returned before any GPU work)."""
import ctypes
import errno
import os
import re
import subprocess

from demikernel_amd import _native as N
from demikernel_amd import tcp_cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_tcp.h")


def test_cc_struct_layout_matches_ctypes(tmp_path):
    structs = {"dk_tcp_cc_conn": N.DkTcpCcConn, "dk_tcp_cc_ack_out": N.DkTcpCcAckOut,
               "dk_tcp_timers_out": N.DkTcpTimersOut}
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
    assert int(got["dk_tcp_cc_conn"]) == N.CC_CONN_DTYPE.itemsize == 64
    for fname, _ in N.DkTcpCcConn._fields_:
        assert N.CC_CONN_DTYPE.fields[fname][1] == getattr(N.DkTcpCcConn, fname).offset, fname
    assert int(got["dk_tcp_cc_conn.ca_start_ns"]) == 40


def test_cc_constants_match_header():
    hdr = open(HEADER).read()
    for i, name in enumerate(N.TCP_CC_STATUSES):
        assert re.search(rf"DK_TCP_CC_{name} = {i}[,\s]", hdr), name
        assert getattr(N, f"DK_TCP_CC_{name}") == i == getattr(tcp_cc, name)
    for name, bit in N.TCP_CC_FLAGS.items():
        assert re.search(rf"#define DK_TCP_CC_{name} {bit}u\s", hdr), name
        assert getattr(tcp_cc, {"IN_RECOVERY": "IN_RECOVERY"}.get(name, name)) == bit
    assert "DK_TCP_CC_BEFORE_SEND = 0, DK_TCP_CC_AFTER_SEND = 1" in hdr
    assert (tcp_cc.BEFORE_SEND, tcp_cc.AFTER_SEND) == (0, 1)
    assert "#define DK_RX_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "dk_rx.h")).read()  # additive
    lib = N.load_library()
    for fn in ("dk_tcp_cc_ack", "dk_tcp_timers", "dk_tcp_cc_send", "dk_tcp_rto_ns", "dk_diag_tcp_cc_cbrt"):
        assert getattr(lib, fn)


def test_null_pointers_are_einval():
    lib = N.load_library()
    r, o, t = N.DkRxResults(), N.DkTcpCcAckOut(), N.DkTcpTimersOut()
    assert lib.dk_tcp_cc_ack(None, ctypes.byref(r), 0, None, None, None, None, None, 0, 0, ctypes.byref(o), None) == errno.EINVAL
    assert lib.dk_tcp_timers(None, None, None, None, None, 0, 0, None, None, ctypes.byref(t), None) == errno.EINVAL
    assert lib.dk_tcp_cc_send(None, 0, None, None, None, 0, None, 0, None, 0, None, None) == errno.EINVAL
    assert lib.dk_diag_tcp_cc_cbrt(None, None, 4, None) == errno.EINVAL
    assert lib.dk_diag_tcp_cc_cbrt(None, None, 0, None) == 0
