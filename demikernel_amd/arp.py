"""The ARP peer on the GPU (include/dk_arp.h).

What SharedArpPeer does (layer3/arp/peer.rs) with ArpCache / HashTtlCache behind it: poll() over the ARP frames of one
RxEngine.receive_batch call (arp_process), query() up to its first await (arp_query_start), the request timeout and its
retries (arp_timers) and try_query (arp_lookup). The cache is a device table (ArpTable) that the device inserts into;
a pending query is a row of QUERY_DTYPE in device memory; a resolved row writes the MAC into links[], which the
send-side calls then take unread by the host.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N
from .rx import FrameBatch, RxResults, _check, _ptr
from .tcp_listen import _stream, to_device  # noqa: F401

CFG_DTYPE, SLOT_DTYPE, QUERY_DTYPE, READY_DTYPE = N.ARP_CFG_DTYPE, N.ARP_SLOT_DTYPE, N.ARP_QUERY_DTYPE, N.ARP_READY_DTYPE
ACTION_BITS, SLOT_STATES, QUERY_STATES, STATUSES = N.ARP_ACTION_BITS, N.ARP_SLOT_STATES, N.ARP_QUERY_STATES, N.ARP_STATUSES
SKIP, HIT, INSERTED, REPLY, LEARNED, DROPPED = 0, 1, 2, 4, 8, 16
FREE, LIVE, TOMBSTONE = range(3)
IDLE, WAITING, RESOLVED, FAILED = range(4)
OK, E_ROW, E_STATE, E_LINK, E_SLOT, NO_ROOM = range(6)
NONE, NO_LINK = N.DK_ARP_NONE, N.DK_ARP_NO_LINK
FRAME_BYTES = N.DK_ARP_FRAME_BYTES
DISABLED = N.DK_ARP_DISABLED


def mac_bytes(mac) -> bytes:
    """'aa:bb:..' or 6 bytes -> 6 bytes."""
    b = bytes(int(x, 16) for x in mac.split(":")) if isinstance(mac, str) else bytes(mac)
    assert len(b) == 6
    return b


def arp_cfg(local_ip: int, local_mac, *, cache_ttl_ns: int = 15_000_000_000, request_timeout_ns: int = 20_000_000_000,
            retry_count: int = 5, disabled: bool = False) -> N.DkArpCfg:
    """dk_arp_cfg with the reference's defaults (ArpConfig: cache ttl 15 s, request timeout 20 s, 5 retries)."""
    c = N.DkArpCfg()
    c.local_ip = local_ip
    c.local_mac[:] = list(mac_bytes(local_mac))
    c.flags = DISABLED if disabled else 0
    c.retry_count, c.cache_ttl_ns, c.request_timeout_ns = retry_count, cache_ttl_ns, request_timeout_ns
    return c


def query_table(nrows: int, **fields) -> np.ndarray:
    """Host table (QUERY_DTYPE, 32-byte items), IDLE, no link; scalars or per-row arrays override."""
    t = np.zeros(nrows, QUERY_DTYPE)
    t["link"] = NO_LINK
    for k, v in fields.items():
        t[k] = np.asarray(v).astype(QUERY_DTYPE.fields[k][0].base)
    return t


def rows_to_host(dev) -> np.ndarray:
    return dev.cpu().numpy().view(QUERY_DTYPE).copy()


def home(cap: int, ip: int) -> int:
    """The slot a key's probe walk starts at (dk_arp_home): pure host code."""
    return int(N.load_library().dk_arp_home(cap, ip))


def fits(cap: int, entries: int) -> bool:
    return N.load_library().dk_arp_fits(cap, entries) == 0


class ArpTable:
    """dk_arp_table: the peer's cache, `cap` slots (a power of two) on `device`, all FREE, with its dk_arp_cfg."""

    def __init__(self, cap: int, cfg: N.DkArpCfg, device: int = 0):
        self.lib = N.load_library()
        self.cap, self.device, self.cfg = cap, device, cfg
        h = ctypes.c_void_p()
        _check(self.lib.dk_arp_table_create(device, cap, ctypes.byref(cfg), ctypes.byref(h)), "dk_arp_table_create")
        self._t = h

    def close(self) -> None:
        if getattr(self, "_t", None):
            self.lib.dk_arp_table_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self) -> np.ndarray:
        """Every slot as a SLOT_DTYPE row (waits for the table's calls)."""
        r = np.zeros(self.cap, SLOT_DTYPE)
        _check(self.lib.dk_arp_table_read(self._t, r.ctypes.data), "dk_arp_table_read")
        return r

    def write(self, rows: np.ndarray) -> None:
        r = np.ascontiguousarray(rows, SLOT_DTYPE)
        assert len(r) == self.cap
        _check(self.lib.dk_arp_table_write(self._t, r.ctypes.data), "dk_arp_table_write")

    def insert(self, pairs, clock_ns: int) -> None:
        """The constructor's initial_values loop: (ip, mac) pairs in order, a later duplicate wins."""
        pairs = list(pairs)
        ips = np.array([p[0] for p in pairs], np.uint32)
        macs = np.frombuffer(b"".join(mac_bytes(p[1]) for p in pairs), np.uint8).copy()
        _check(self.lib.dk_arp_table_insert(self._t, ips.ctypes.data, macs.ctypes.data, len(pairs), clock_ns),
               "dk_arp_table_insert")

    def as_map(self) -> dict:
        """ip -> (mac bytes, expiration_ns) of the LIVE slots. Slot numbers are not part of the contract."""
        return {int(r["ip"]): (bytes(r["mac"]), int(r["expiration_ns"])) for r in self.rows() if r["state"] == LIVE}

    def consumed(self) -> int:
        c = ctypes.c_uint64()
        _check(self.lib.dk_arp_table_stats(self._t, None, ctypes.byref(c)), "dk_arp_table_stats")
        return c.value


class ArpResults:
    """Device outputs of one dk_arp_process / _query_start / _timers call (dk_arp_results) for n batch frames, up to
    max_frames frames and max_ready ready records, nstatus status words (one; start[] entries); every array starts as
    `fill` bytes."""

    def __init__(self, n: int, max_frames: int, max_ready: int, nstatus: int = 1, device: int = 0, fill: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.n, self.max_frames, self.max_ready, self.nstatus = n, max_frames, max_ready, nstatus
        u8 = lambda k: torch.full((max(k, 4),), fill, dtype=torch.uint8, device=dev)  # noqa: E731
        self.action, self.reply_frame = u8(n), u8(4 * n)
        self.off_out, self.len_out, self.frame_seg = u8(4 * max_frames), u8(2 * max_frames), u8(4 * max_frames)
        self.ready = u8(READY_DTYPE.itemsize * max_ready)
        self.status = u8(4 * nstatus)
        self.n_frames, self.n_ready, self.n_entries = u8(4), u8(4), u8(4)

    def c_struct(self) -> N.DkArpResults:
        return N.DkArpResults(*[_ptr(getattr(self, k)) for k in N.ARP_RESULT_FIELDS])

    def raw(self) -> dict:
        """Every array whole, as bytes (for canary comparisons)."""
        return {k: getattr(self, k).cpu().numpy().copy() for k in N.ARP_RESULT_FIELDS}

    def to_numpy(self) -> dict:
        r = self.raw()
        u32 = lambda k, m: r[k][:4 * m].view(np.uint32)  # noqa: E731
        return {"action": r["action"][:self.n], "reply_frame": u32("reply_frame", self.n),
                "off_out": u32("off_out", self.max_frames), "len_out": r["len_out"][:2 * self.max_frames].view(np.uint16),
                "frame_seg": u32("frame_seg", self.max_frames),
                "ready": r["ready"][:READY_DTYPE.itemsize * self.max_ready].view(READY_DTYPE),
                "status": u32("status", self.nstatus), "n_frames": int(u32("n_frames", 1)[0]),
                "n_ready": int(u32("n_ready", 1)[0]), "n_entries": int(u32("n_entries", 1)[0])}


def _nrows(rows) -> int:
    return 0 if rows is None else rows.numel() // QUERY_DTYPE.itemsize


def _nlinks(links) -> int:
    return 0 if links is None else links.numel() // N.TX_LINK_DTYPE.itemsize


def arp_process(table: ArpTable, batch: FrameBatch, rx: RxResults, rows, links, clock_ns: int, out, res: ArpResults, *,
                slot_stride: int, frame_lead: int = 0, n: Optional[int] = None, out_bytes=None, max_frames=None,
                max_ready=None, stream=None) -> None:
    """dk_arp_process: `batch` and `rx` are the arguments of the batch's receive_batch call, rows a uint8 device
    tensor of QUERY_DTYPE rows and links the device dk_tx_link array (both updated in place; either may be None)."""
    s = _stream(stream, table.device)
    b, r, o = batch.c_struct(), rx.c_struct(), res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(table.lib.dk_arp_process(
        table._t, ctypes.byref(b), ctypes.byref(r), rx.n if n is None else n, _ptr(rows), _nrows(rows), _ptr(links),
        _nlinks(links), clock_ns, _ptr(out), out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
        res.max_frames if max_frames is None else max_frames, res.max_ready if max_ready is None else max_ready,
        ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_arp_process")


def arp_query_start(table: ArpTable, rows, start, links, now_ns: int, out, res: ArpResults, *, slot_stride: int,
                    frame_lead: int = 0, nstart: Optional[int] = None, out_bytes=None, max_frames=None, max_ready=None,
                    stream=None) -> None:
    """dk_arp_query_start: start the int32 / uint32 device array of row indices in query-call order."""
    s = _stream(stream, table.device)
    o = res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(table.lib.dk_arp_query_start(
        table._t, _ptr(rows), _nrows(rows), _ptr(start), start.numel() if nstart is None else nstart, _ptr(links),
        _nlinks(links), now_ns, _ptr(out), out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
        res.max_frames if max_frames is None else max_frames, res.max_ready if max_ready is None else max_ready,
        ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_arp_query_start")


def arp_timers(table: ArpTable, rows, links, now_ns: int, out, res: ArpResults, *, slot_stride: int,
               frame_lead: int = 0, out_bytes=None, max_frames=None, max_ready=None, stream=None) -> None:
    """dk_arp_timers: the request timeout over every row."""
    s = _stream(stream, table.device)
    o = res.c_struct()
    lay = N.DkTcpTxLayout(slot_stride, frame_lead)
    _check(table.lib.dk_arp_timers(
        table._t, _ptr(rows), _nrows(rows), _ptr(links), _nlinks(links), now_ns, _ptr(out),
        out.numel() if out_bytes is None else out_bytes, ctypes.byref(lay),
        res.max_frames if max_frames is None else max_frames, res.max_ready if max_ready is None else max_ready,
        ctypes.byref(o), ctypes.c_void_p(s.cuda_stream)), "dk_arp_timers")


def arp_lookup(table: ArpTable, ips, links=None, link=None, stream=None, fill: int = 0):
    """dk_arp_lookup of `ips` (an iterable of addresses); link: per-address link indices (NO_LINK: none). Returns
    (found u32[n], macs u8[n, 6]) as whole canary-filled arrays cut to n (waits for the call). The addresses and link
    indices are uploaded and the two arrays made, filled and read back on `stream` (default: the current stream), the
    stream the call runs on; `links` must be ready on it. For the asynchronous calls above the same holds for
    everything the caller passes in, their result objects included: tensors made or filled on another stream need that
    stream waited for before the call."""
    import torch

    a = np.asarray(list(ips), np.uint32)
    dev = torch.device("cuda", table.device)
    s = _stream(stream, table.device)
    with torch.cuda.stream(s):
        ad = torch.from_numpy(a.view(np.int32).copy()).to(dev)
        ld = None if link is None else torch.from_numpy(np.asarray(list(link), np.uint32).view(np.int32).copy()).to(dev)
        found = torch.full((4 * max(len(a), 1),), fill, dtype=torch.uint8, device=dev)
        macs = torch.full((6 * max(len(a), 1),), fill, dtype=torch.uint8, device=dev)
        _check(table.lib.dk_arp_lookup(table._t, _ptr(ad), _ptr(ld), len(a), _ptr(links), _nlinks(links), _ptr(macs),
                                       _ptr(found), ctypes.c_void_p(s.cuda_stream)), "dk_arp_lookup")
        return found.cpu().numpy().view(np.uint32)[:len(a)], macs.cpu().numpy().reshape(-1, 6)[:len(a)]
