"""The ABI of include/dk_arp.h on the CPU: struct layouts against the C compiler, constants against the header, the
symbols, and the argument rules that need no device."""
import ctypes
import errno
import os
import re
import subprocess

import demikernel_amd
from demikernel_amd import _native as N
from demikernel_amd import arp as ARP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dk_arp.h")


def test_arp_struct_layout_matches_ctypes(tmp_path):
    structs = {"dk_arp_cfg": N.DkArpCfg, "dk_arp_query": N.DkArpQuery, "dk_arp_ready": N.DkArpReady,
               "dk_arp_slot": N.DkArpSlot, "dk_arp_results": N.DkArpResults}
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
    for cname, dt in (("dk_arp_cfg", N.ARP_CFG_DTYPE), ("dk_arp_query", N.ARP_QUERY_DTYPE),
                      ("dk_arp_ready", N.ARP_READY_DTYPE), ("dk_arp_slot", N.ARP_SLOT_DTYPE)):
        assert int(got[cname]) == dt.itemsize
        for fname in dt.names:
            assert int(got[f"{cname}.{fname}"]) == dt.fields[fname][1], (cname, fname)
    assert [int(got[k]) for k in ("dk_arp_cfg", "dk_arp_query", "dk_arp_ready", "dk_arp_slot")] == [40, 32, 24, 24]
    assert int(got["dk_arp_results"]) == 8 * len(N.ARP_RESULT_FIELDS)


def test_arp_header_compiles_as_cxx(tmp_path):
    c = tmp_path / "h.cpp"
    c.write_text(f'#include "{HEADER}"\nint main() {{ return sizeof(dk_arp_query) == 32 ? 0 : 1; }}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(c)], check=True)


def test_arp_constants_match_header():
    hdr = open(HEADER).read()
    for prefix, names in (("DK_ARP_SLOT_", N.ARP_SLOT_STATES), ("DK_ARP_Q_", N.ARP_QUERY_STATES), ("DK_ARP_", N.ARP_STATUSES)):
        for i, name in enumerate(names):
            assert re.search(rf"{prefix}{name} = {i}[,\s]", hdr), name
    assert (ARP.FREE, ARP.LIVE, ARP.TOMBSTONE) == (0, 1, 2) and (ARP.IDLE, ARP.WAITING, ARP.RESOLVED, ARP.FAILED) == (0, 1, 2, 3)
    assert [getattr(ARP, s) for s in N.ARP_STATUSES] == list(range(6))
    for name, bit in N.ARP_ACTION_BITS.items():
        assert re.search(rf"#define DK_ARP_{name} {bit}u\s", hdr), name
        assert getattr(ARP, name) == bit
    assert N.ARP_ACTION_BITS == {"HIT": 1, "INSERTED": 2, "REPLY": 4, "LEARNED": 8, "DROPPED": 16}
    for name, val in (("NONE", "0xFFFFFFFFu"), ("NO_LINK", "0xFFFFFFFFu"), ("FRAME_BYTES", "42u"), ("DISABLED", "1u"),
                      ("MAX_RETRIES", "65534u"), ("SKIP", "0u")):
        assert re.search(rf"#define DK_ARP_{name} {val}\s", hdr), name
        if name != "SKIP":
            assert getattr(N, f"DK_ARP_{name}") == int(val.rstrip("u"), 0)
    assert "#define DK_RX_ABI_VERSION 4u" in open(os.path.join(ROOT, "include", "dk_rx.h")).read()  # additive
    lib = N.load_library()
    assert lib.dk_rx_abi_version() == 4
    for fn, _, _ in N.ARP_FUNCTIONS:
        assert getattr(lib, fn)
        assert re.search(rf"\b{fn}\(", hdr), fn
    assert sorted(set(re.findall(r"\b(dk_arp_\w+)\(", hdr))) == sorted(fn for fn, _, _ in N.ARP_FUNCTIONS)
    for name in ("ArpTable", "arp_process", "arp_query_start", "arp_timers", "arp_lookup", "ArpResults"):
        assert getattr(demikernel_amd, name) is getattr(ARP, name)
    assert ARP.to_device is demikernel_amd.tcp_listen.to_device
    assert "do_drop" in hdr and "include/dk_arp.h" in open(os.path.join(ROOT, "include", "dk_tcp.h")).read()
    import __graft_entry__ as G

    assert "arp_kernels.hip" in G.SOURCES and "dk_arp.h" in G.INCLUDES


def test_home_and_fits():
    lib = N.load_library()
    for cap in (2, 4, 64, 1 << 20):
        homes = {ARP.home(cap, ip) for ip in range(4 * cap)}
        assert all(0 <= h < cap for h in homes) and len(homes) > cap // 2
        assert ARP.home(cap, 0x0301A8C0) == ARP.home(cap, 0x0301A8C0)
    assert lib.dk_arp_home(0, 5) == 0
    assert ARP.fits(4, 2) and not ARP.fits(4, 3) and ARP.fits(2, 1) and not ARP.fits(2, 2)
    assert lib.dk_arp_fits(4, 3) == errno.EINVAL
    # a chain that wraps around the end of a table of 4 can be crafted
    by_home = {}
    for ip in range(1, 4000):
        by_home.setdefault(ARP.home(4, ip), []).append(ip)
    assert all(len(by_home[h]) >= 3 for h in range(4))


def test_argument_rules_without_a_device():
    """EINVAL before any GPU work: null required pointers, misaligned rows, n >= 2^31, out_bytes over the limit, and
    the table's own rules."""
    lib = N.load_library()
    E = errno.EINVAL
    h = ctypes.c_void_p()
    good = ARP.arp_cfg(1, bytes(6))
    assert lib.dk_arp_table_create(0, 4, None, ctypes.byref(h)) == E                                  # null cfg
    assert lib.dk_arp_table_create(0, 4, ctypes.byref(good), None) == E                               # null out
    for cap in (0, 1, 3, 6, 100):
        assert lib.dk_arp_table_create(0, cap, ctypes.byref(good), ctypes.byref(h)) == E              # not a power of two >= 2
    assert lib.dk_arp_table_create(0, 4, ctypes.byref(ARP.arp_cfg(1, bytes(6), cache_ttl_ns=0)), ctypes.byref(h)) == E
    assert lib.dk_arp_table_create(0, 4, ctypes.byref(ARP.arp_cfg(1, bytes(6), retry_count=65535)), ctypes.byref(h)) == E
    bad_flags = ARP.arp_cfg(1, bytes(6))
    bad_flags.flags = 2
    assert lib.dk_arp_table_create(0, 4, ctypes.byref(bad_flags), ctypes.byref(h)) == E
    assert lib.dk_arp_table_create(-1, 4, ctypes.byref(good), ctypes.byref(h)) == E                   # no such device
    assert lib.dk_arp_table_stats(None, None, None) == E and lib.dk_arp_table_read(None, None) == E
    assert lib.dk_arp_table_write(None, None) == E and lib.dk_arp_table_insert(None, None, None, 0, 0) == E
    lib.dk_arp_table_destroy(None)  # a no-op

    b, r, lay = N.DkRxBatch(), N.DkRxResults(), N.DkTcpTxLayout(64, 0)
    words = (ctypes.c_uint32 * 4)()
    w = [ctypes.addressof(words) + 4 * k for k in range(4)]
    buf = (ctypes.c_uint8 * 256)()
    a = (ctypes.addressof(buf) + 63) & ~63  # a 64-byte aligned address: never dereferenced by the checks
    t = a                                   # a table handle: the checks below fail before it is touched
    ok = N.DkArpResults(n_frames=w[0], n_ready=w[1], n_entries=w[2], status=w[3])
    B, R_, L, O = ctypes.byref(b), ctypes.byref(r), ctypes.byref(lay), ctypes.byref(ok)
    big = 0xFFFFFF00 + 1  # DK_RX_MAX_BLOB + 1
    # dk_arp_process(t, batch, rx, n, rows, nrows, links, nlinks, clock, out, out_bytes, layout, max_frames, max_ready, res, s)
    proc = lib.dk_arp_process
    assert proc(None, B, R_, 0, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E        # null table
    assert proc(t, None, R_, 0, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E        # null batch
    assert proc(t, B, None, 0, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E         # null rx
    assert proc(t, B, R_, 0, None, 0, None, 0, 0, None, 0, None, 0, 0, O, None) == E        # null layout
    assert proc(t, B, R_, 0, None, 0, None, 0, 0, None, 0, L, 0, 0, None, None) == E        # null results
    for missing in ("n_frames", "n_ready", "n_entries", "status"):
        part = N.DkArpResults(**{k: w[0] for k in ("n_frames", "n_ready", "n_entries", "status") if k != missing})
        assert proc(t, B, R_, 0, None, 0, None, 0, 0, None, 0, L, 0, 0, ctypes.byref(part), None) == E, missing
    assert proc(t, B, R_, 0, None, 0, None, 1, 0, None, 0, L, 0, 0, O, None) == E           # nlinks without links
    assert proc(t, B, R_, 0, None, 1, None, 0, 0, None, 0, L, 0, 0, O, None) == E           # nrows without rows
    assert proc(t, B, R_, 0, a + 8, 1, None, 0, 0, None, 0, L, 0, 0, O, None) == E          # misaligned rows
    assert proc(t, B, R_, 0, None, 0, None, 0, 0, None, big, L, 0, 0, O, None) == E         # out_bytes
    assert proc(t, B, R_, 1 << 31, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E     # n >= 2^31
    assert proc(t, B, R_, 0, a, 1 << 31, None, 0, 0, None, 0, L, 0, 0, O, None) == E        # nrows >= 2^31
    assert proc(t, B, R_, 1, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E           # n with null batch arrays
    fb = N.DkRxBatch(frames=a, frames_bytes=64, off=a, len=a, n=1)
    full = N.DkArpResults(n_frames=w[0], n_ready=w[1], n_entries=w[2], status=w[3], action=a, reply_frame=a)
    for missing in ("meta", "src_ip", "dst_ip"):
        part = N.DkRxResults(**{k: a for k in ("meta", "src_ip", "dst_ip") if k != missing})
        assert proc(t, ctypes.byref(fb), ctypes.byref(part), 1, None, 0, None, 0, 0, None, 0, L, 0, 0, ctypes.byref(full),
                    None) == E, missing
    rx3 = N.DkRxResults(meta=a, src_ip=a, dst_ip=a)
    assert proc(t, ctypes.byref(fb), ctypes.byref(rx3), 1, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E  # no action[]
    assert proc(t, ctypes.byref(fb), ctypes.byref(rx3), 1, None, 0, None, 0, 0, None, 64, L, 1, 0, ctypes.byref(full),
                None) == E                                                                   # max_frames without out
    assert proc(t, ctypes.byref(fb), ctypes.byref(rx3), 1, None, 0, None, 0, 0, None, 0, L, 0, 1, ctypes.byref(full),
                None) == E                                                                   # max_ready without ready
    # dk_arp_query_start(t, rows, nrows, start, nstart, links, nlinks, now, out, out_bytes, layout, max_frames, max_ready, res, s)
    start = lib.dk_arp_query_start
    assert start(None, None, 0, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E        # null table
    assert start(t, None, 0, None, 0, None, 0, 0, None, 0, None, 0, 0, O, None) == E        # null layout
    assert start(t, None, 0, None, 0, None, 0, 0, None, 0, L, 0, 0, None, None) == E        # null results
    assert start(t, None, 1, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E           # nrows without rows
    assert start(t, a + 4, 1, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E          # misaligned rows
    assert start(t, a, 1, None, 1, None, 0, 0, None, 0, L, 0, 0, O, None) == E              # null start[]
    assert start(t, a, 1, a, 1 << 31, None, 0, 0, None, 0, L, 0, 0, O, None) == E           # nstart >= 2^31
    assert start(t, a, 1, a, 1, None, 0, 0, None, big, L, 0, 0, O, None) == E               # out_bytes
    assert start(t, a, 1, a, 1, None, 0, 0, None, 64, L, 1, 0, O, None) == E                # max_frames without out
    assert start(t, a, 1, a, 1, None, 1, 0, None, 0, L, 0, 0, O, None) == E                 # nlinks without links
    # dk_arp_timers(t, rows, nrows, links, nlinks, now, out, out_bytes, layout, max_frames, max_ready, res, s)
    tim = lib.dk_arp_timers
    assert tim(None, None, 0, None, 0, 0, None, 0, L, 0, 0, O, None) == E                   # null table
    assert tim(t, None, 1, None, 0, 0, None, 0, L, 0, 0, O, None) == E                      # nrows without rows
    assert tim(t, a + 2, 1, None, 0, 0, None, 0, L, 0, 0, O, None) == E                     # misaligned rows
    assert tim(t, a, 1, None, 0, 0, None, big, L, 0, 0, O, None) == E                       # out_bytes
    assert tim(t, a, 1, None, 0, 0, None, 0, L, 0, 1, O, None) == E                         # max_ready without ready
    assert tim(t, a, 1, None, 0, 0, None, 0, None, 0, 0, O, None) == E                      # null layout
    # dk_arp_lookup(t, ips, link, n, links, nlinks, macs_out, found, s)
    look = lib.dk_arp_lookup
    assert look(None, None, None, 0, None, 0, None, None, None) == E                        # null table
    assert look(t, None, None, 1, None, 0, a, a, None) == E                                 # null ips
    assert look(t, a, None, 1, None, 0, None, a, None) == E                                 # null macs_out
    assert look(t, a, None, 1, None, 0, a, None, None) == E                                 # null found
    assert look(t, a, None, 1 << 31, None, 0, a, a, None) == E                              # n >= 2^31
    assert look(t, a, None, 1, None, 1, a, a, None) == E                                    # nlinks without links


def test_host_tables():
    rows = ARP.query_table(3, ip=[1, 2, 3], tag=7)
    assert list(rows["state"]) == [ARP.IDLE] * 3 and list(rows["link"]) == [ARP.NO_LINK] * 3 and list(rows["tag"]) == [7] * 3
    c = ARP.arp_cfg(0x0201A8C0, "12:23:45:67:89:ab", disabled=True)
    assert bytes(c.local_mac) == bytes([0x12, 0x23, 0x45, 0x67, 0x89, 0xAB]) and c.flags == ARP.DISABLED
    assert (c.cache_ttl_ns, c.request_timeout_ns, c.retry_count) == (15_000_000_000, 20_000_000_000, 5)
