"""The ABI additions of the passive-open section of include/dk_tcp.h on the CPU: struct layouts against the C compiler,
constants against the header, the symbols, the pure host helpers, and the argument rules that need no device."""
import ctypes
import errno
import os
import re
import subprocess

from demikernel_amd import _native as N
from demikernel_amd import tcp_listen as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_tcp.h")


def test_listen_struct_layout_matches_ctypes(tmp_path):
    structs = {"dk_tcp_listener": N.DkTcpListener, "dk_tcp_lsn_slot": N.DkTcpLsnSlot, "dk_tcp_lsn_ready": N.DkTcpLsnReady,
               "dk_tcp_lsn_results": N.DkTcpLsnResults}
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
    for cname, dt in (("dk_tcp_listener", N.LISTENER_DTYPE), ("dk_tcp_lsn_slot", N.LSN_SLOT_DTYPE),
                      ("dk_tcp_lsn_ready", N.LSN_READY_DTYPE)):
        assert int(got[cname]) == dt.itemsize
        for fname in dt.names:
            assert int(got[f"{cname}.{fname}"]) == dt.fields[fname][1], (cname, fname)
    assert (int(got["dk_tcp_listener"]), int(got["dk_tcp_lsn_slot"]), int(got["dk_tcp_lsn_ready"])) == (64, 48, 48)


def test_listen_constants_match_header():
    hdr = open(HEADER).read()
    for i, name in enumerate(N.TCP_LSN_ACTIONS):
        assert re.search(rf"DK_TCP_LSN_{name} = {i}[,\s]", hdr), name
        assert getattr(TL, name) == i
    for i, name in enumerate(N.TCP_LSN_STATUSES):
        assert re.search(rf"DK_TCP_LSN_{name} = {i}[,\s]", hdr), name
        assert getattr(TL, name) == i
    for i, name in enumerate(N.TCP_LSN_SLOT_STATES):
        assert re.search(rf"DK_TCP_LSN_{name} = {i}[,\s]", hdr), name
        assert getattr(TL, name) == i
    assert "DK_TCP_LSN_CLOSED = 0, DK_TCP_LSN_LISTENING = 1" in hdr
    for name, val in (("NONE", "0xFFFFFFFFu"), ("NO_WSCALE", "0xFFu"), ("FALLBACK_MSS", "536u"),
                      ("MAX_LISTENERS", "65535u"), ("SYNACK_BYTES", "62u"), ("RST_BYTES", "54u")):
        assert re.search(rf"#define DK_TCP_LSN_{name} {val}\s", hdr), name
        assert getattr(N, f"DK_TCP_LSN_{name}") == int(val.rstrip("u"), 0)
    assert "#define DK_TCP_LSN_KEY_FREE (~0ull)" in hdr and "#define DK_TCP_LSN_KEY_TOMBSTONE (0xFFFFull << 48)" in hdr
    assert "#define DK_RX_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "dk_rx.h")).read()  # additive
    lib = N.load_library()
    for fn, _, _ in N.TCP_LISTEN_FUNCTIONS:
        assert getattr(lib, fn)


def test_pure_host_helpers():
    lib = N.load_library()
    k = lib.dk_tcp_listen_key(0x1234, 0x0A0B0C0D, 0xBEEF)
    assert k == TL.key(0x1234, 0x0A0B0C0D, 0xBEEF) == 0x1234_0A0B0C0D_BEEF
    assert TL.key_fields(k) == (0x1234, 0x0A0B0C0D, 0xBEEF)
    assert k not in (N.DK_TCP_LSN_KEY_FREE, N.DK_TCP_LSN_KEY_TOMBSTONE)
    for cap in (2, 64, 1 << 20):
        homes = {lib.dk_tcp_listen_home(cap, TL.key(1, 0x0100000A + (j << 8), 1000 + j)) for j in range(512)}
        assert max(homes) < cap and len(homes) >= min(cap, 512) // 2  # in range, and it spreads
        assert lib.dk_tcp_listen_home(cap, k) == lib.dk_tcp_listen_home(cap, k) == TL.home(cap, k)
    assert lib.dk_tcp_listen_backlog_fits(64, 32) == 0 and lib.dk_tcp_listen_backlog_fits(64, 33) == errno.EINVAL
    assert lib.dk_tcp_listen_backlog_fits(2, 1) == 0 and lib.dk_tcp_listen_backlog_fits(1 << 31, 1 << 40) == errno.EINVAL


def test_argument_rules_without_a_device():
    lib = N.load_library()
    h = ctypes.c_void_p()
    for cap in (0, 1, 3, 48, 1000, (1 << 20) + 1):
        assert lib.dk_tcp_listen_table_create(0, cap, ctypes.byref(h)) == errno.EINVAL and not h.value
    assert lib.dk_tcp_listen_table_create(0, 64, None) == errno.EINVAL
    r, o, lay = N.DkRxResults(), N.DkTcpLsnResults(), N.DkTcpTxLayout(64, 0)
    assert lib.dk_tcp_listen_process(None, ctypes.byref(r), 0, None, 0, 0, None, 0, None, None, 0, 0, None, 0,
                                     ctypes.byref(lay), 0, 0, 0, ctypes.byref(o), None) == errno.EINVAL
    assert lib.dk_tcp_listen_timers(None, None, 0, 0, None, 0, 0, None, 0, ctypes.byref(lay), 0, 0, 0, ctypes.byref(o),
                                    None) == errno.EINVAL
    assert lib.dk_tcp_listen_release(None, None, 0, None, 0, None, None) == errno.EINVAL
    assert lib.dk_tcp_listen_table_stats(None, None, None) == errno.EINVAL
    assert lib.dk_tcp_listen_table_read(None, None) == errno.EINVAL
    assert lib.dk_tcp_listen_table_write(None, None) == errno.EINVAL
    lib.dk_tcp_listen_table_destroy(None)
