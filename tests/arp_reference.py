"""A plain-Python restatement of the ARP peer that include/dk_arp.h specifies, written from the reference's behaviour
(layer3/arp/peer.rs, layer3/arp/cache/mod.rs, collections/hashttlcache.rs): a literal per-frame loop over a dict with
clock, cleanup, insert and get as HashTtlCache has them, a waiter list per address, the query loop as a small state
machine, and the 42-byte builders. Nothing here is parallel and nothing knows about f0: tests/test_arp_model.py pins it
against the reference's own scripted expectations, tests/test_gpu_arp.py compares the device with it whole."""
from __future__ import annotations

import errno

import numpy as np

from demikernel_amd import _native as N

HIT, INSERTED, REPLY, LEARNED, DROPPED = 1, 2, 4, 8, 16
IDLE, WAITING, RESOLVED, FAILED = range(4)
OK, E_ROW, E_STATE, E_LINK, E_SLOT, NO_ROOM = range(6)
NONE = NO_LINK = 0xFFFFFFFF
BROADCAST = b"\xff" * 6
ZERO_MAC = bytes(6)


def ip_bytes(ip: int) -> bytes:
    return int(ip).to_bytes(4, "little")  # octet order: the first octet is the low byte


def arp_frame(op: int, eth_dst: bytes, sha: bytes, spa: int, tha: bytes, tpa: int) -> bytes:
    f = eth_dst + sha + b"\x08\x06" + b"\x00\x01\x08\x00\x06\x04" + bytes([0, op]) + sha + ip_bytes(spa) + tha + ip_bytes(tpa)
    assert len(f) == 42
    return f


def build_request(local_mac: bytes, local_ip: int, ip: int) -> bytes:
    return arp_frame(1, BROADCAST, local_mac, local_ip, BROADCAST, ip)


def build_reply(local_mac: bytes, local_ip: int, sha: bytes, spa: int) -> bytes:
    return arp_frame(2, sha, local_mac, local_ip, sha, spa)


def blob_of(frames, slot_stride, frame_lead, size, canary) -> np.ndarray:
    b = np.full(size, canary, np.uint8)
    for j, f in enumerate(frames):
        b[j * slot_stride + frame_lead: j * slot_stride + frame_lead + len(f)] = np.frombuffer(f, np.uint8)
    return b


class TtlCache:
    """HashTtlCache: values with an optional expiration; get does not test expiry, insert cleans up first."""

    def __init__(self, now: int, default_ttl):
        self.clock, self.default_ttl, self.d = now, default_ttl, {}

    def advance_clock(self, now: int):
        assert now >= self.clock
        self.clock = now

    def cleanup(self):
        self.d = {k: v for k, v in self.d.items() if v[1] is None or self.clock < v[1]}

    def insert_with_ttl(self, key, value, ttl):
        self.cleanup()
        old = self.d.get(key)
        self.d[key] = (value, None if ttl is None else self.clock + ttl)
        return None if old is None else old[0]

    def insert(self, key, value):
        return self.insert_with_ttl(key, value, self.default_ttl)

    def get(self, key):
        v = self.d.get(key)
        return None if v is None else v[0]


class Frame:
    """What dk_arp_process reads of one batch frame."""

    def __init__(self, covered: bool, op: int = 0, sha: bytes = ZERO_MAC, spa: int = 0, tpa: int = 0):
        self.covered, self.op, self.sha, self.spa, self.tpa = covered, op, bytes(sha), spa, tpa


class ArpModel:
    """The peer: cfg, the cache (None: DK_ARP_DISABLED), the query rows and links[] as the device holds them."""

    def __init__(self, local_ip: int, local_mac: bytes, *, cap: int, cache_ttl_ns: int, request_timeout_ns: int,
                 retry_count: int, disabled: bool = False, rows=None, links=None, clock: int = 0):
        self.local_ip, self.local_mac, self.cap = local_ip, bytes(local_mac), cap
        self.ttl, self.timeout, self.retries = cache_ttl_ns, request_timeout_ns, retry_count
        self.cache = None if disabled else TtlCache(clock, cache_ttl_ns)
        self.rows = np.zeros(0, N.ARP_QUERY_DTYPE) if rows is None else rows.copy()
        self.links = np.zeros(0, N.TX_LINK_DTYPE) if links is None else links.copy()

    # -- the cache -----------------------------------------------------------------------------------------------------
    def get(self, ip):
        return ZERO_MAC if self.cache is None else self.cache.get(ip)

    def cache_insert(self, ip, mac):
        if self.cache is not None:
            self.cache.insert(ip, bytes(mac))

    def insert_initial(self, pairs, clock):
        if self.cache is not None:
            self.cache.advance_clock(clock)
        for ip, mac in pairs:
            self.cache_insert(ip, mac)

    def table(self) -> dict:
        return {} if self.cache is None else {k: (v[0], v[1]) for k, v in self.cache.d.items()}

    def n_entries(self) -> int:
        return 0 if self.cache is None else len(self.cache.d)

    # -- helpers -------------------------------------------------------------------------------------------------------
    def _snapshot(self):
        return (None if self.cache is None else (self.cache.clock, dict(self.cache.d)), self.rows.copy(), self.links.copy())

    def _restore(self, snap):
        if self.cache is not None:
            self.cache.clock, self.cache.d = snap[0][0], snap[0][1]
        self.rows, self.links = snap[1], snap[2]

    def _resolve(self, r, mac):
        R = self.rows[r]
        R["state"], R["err"], R["mac"] = RESOLVED, 0, np.frombuffer(mac, np.uint8)
        if int(R["link"]) != NO_LINK and int(R["link"]) < len(self.links):
            self.links[int(R["link"])]["dst_mac"] = np.frombuffer(mac, np.uint8)

    def _ready(self, r, frame, mac, err=0):
        y = np.zeros(1, N.ARP_READY_DTYPE)[0]
        y["row"], y["tag"], y["ip"], y["frame"] = r, self.rows[r]["tag"], self.rows[r]["ip"], frame
        y["mac"], y["err"] = np.frombuffer(mac, np.uint8), err
        return y

    def _finish(self, snap, out, slot_stride, frame_lead, max_frames, out_bytes, max_ready, per_start=None):
        nf, ny = len(out["frames"]), len(out["ready"])
        out["n_frames"], out["n_ready"], out["n_entries"] = nf, ny, self.n_entries()
        slot_ok = nf == 0 or frame_lead + 42 <= slot_stride
        out["fits"] = (nf <= max_frames and nf * slot_stride <= out_bytes and ny <= max_ready and
                       out["n_entries"] <= self.cap // 2 and slot_ok)
        if per_start is None:
            out["status"] = np.array([OK if out["fits"] else NO_ROOM if slot_ok else E_SLOT], np.uint32)
        else:
            out["status"] = np.array([NO_ROOM if s == OK and not out["fits"] else s for s in per_start], np.uint32)
        if not out["fits"]:
            self._restore(snap)
        return out

    # -- SharedArpPeer::poll -------------------------------------------------------------------------------------------
    def process(self, frames, clock, *, slot_stride=64, frame_lead=0, max_frames=None, out_bytes=1 << 30, max_ready=None):
        n = len(frames)
        max_frames = n if max_frames is None else max_frames
        max_ready = len(self.rows) if max_ready is None else max_ready
        snap = self._snapshot()
        if self.cache is not None:
            self.cache.advance_clock(clock)
        waiters = {}
        for r in range(len(self.rows)):
            if int(self.rows[r]["state"]) == WAITING:
                waiters.setdefault(int(self.rows[r]["ip"]), []).append(r)
        out = {"action": np.zeros(n, np.uint8), "reply_frame": np.full(n, NONE, np.uint32), "frames": [], "frame_seg": [],
               "ready": []}

        def do_insert(i, f):
            for r in waiters.pop(f.spa, []):
                self._resolve(r, f.sha)
                out["ready"].append(self._ready(r, i, f.sha))
            self.cache_insert(f.spa, f.sha)

        for i, f in enumerate(frames):
            if not f.covered:
                continue
            act = 0
            hit = self.get(f.spa) is not None
            if hit:
                do_insert(i, f)
                act |= HIT | INSERTED
            if f.tpa != self.local_ip:
                out["action"][i] = act if hit else DROPPED
                continue
            if not hit:
                do_insert(i, f)
                act |= LEARNED | INSERTED
            if f.op == 1:
                out["reply_frame"][i] = len(out["frames"])
                out["frames"].append(build_reply(self.local_mac, self.local_ip, f.sha, f.spa))
                out["frame_seg"].append(i)
                act |= REPLY
            else:
                self.cache_insert(f.spa, f.sha)
            out["action"][i] = act
        return self._finish(snap, out, slot_stride, frame_lead, max_frames, out_bytes, max_ready)

    # -- query() up to its first await ---------------------------------------------------------------------------------
    def start(self, start, now, *, slot_stride=64, frame_lead=0, max_frames=None, out_bytes=1 << 30, max_ready=None):
        max_frames = len(start) if max_frames is None else max_frames
        max_ready = len(start) if max_ready is None else max_ready
        snap = self._snapshot()
        out = {"frames": [], "frame_seg": [], "ready": []}
        status, seen = [], set()
        for k, r in enumerate(start):
            if r >= len(self.rows):
                status.append(E_ROW)
                continue
            R = self.rows[r]
            if int(snap[1][r]["state"]) != IDLE or r in seen:
                status.append(E_STATE)
                continue
            seen.add(r)
            if int(R["link"]) != NO_LINK and int(R["link"]) >= len(self.links):
                status.append(E_LINK)
            elif frame_lead + 42 > slot_stride:
                status.append(E_SLOT)
            else:
                status.append(OK)
                mac = self.get(int(R["ip"]))
                if mac is not None:
                    self._resolve(r, mac)
                    out["ready"].append(self._ready(r, NONE, mac))
                else:
                    out["frames"].append(build_request(self.local_mac, self.local_ip, int(R["ip"])))
                    out["frame_seg"].append(k)
                    R["state"], R["err"], R["sent"], R["deadline_ns"] = WAITING, 0, 1, now + self.timeout
        return self._finish(snap, out, slot_stride, frame_lead, max_frames, out_bytes, max_ready, per_start=status)

    # -- the conditional_yield_with_timeout expiry ---------------------------------------------------------------------
    def timers(self, now, *, slot_stride=64, frame_lead=0, max_frames=64, out_bytes=1 << 30, max_ready=64):
        snap = self._snapshot()
        out = {"frames": [], "frame_seg": [], "ready": []}
        for r in range(len(self.rows)):
            R = self.rows[r]
            if int(R["state"]) != WAITING or int(R["deadline_ns"]) > now:
                continue
            if int(R["sent"]) < self.retries + 1:
                out["frames"].append(build_request(self.local_mac, self.local_ip, int(R["ip"])))
                out["frame_seg"].append(r)
                R["sent"] = int(R["sent"]) + 1
                mac = self.get(int(R["ip"]))
                if mac is not None:
                    self._resolve(r, mac)
                    out["ready"].append(self._ready(r, NONE, mac))
                else:
                    R["deadline_ns"] = now + self.timeout
            else:
                R["state"], R["err"] = FAILED, errno.ETIMEDOUT
                out["ready"].append(self._ready(r, NONE, ZERO_MAC, errno.ETIMEDOUT))
        return self._finish(snap, out, slot_stride, frame_lead, max_frames, out_bytes, max_ready)

    # -- try_query -----------------------------------------------------------------------------------------------------
    def lookup(self, ips, link=None):
        found, macs = [], []
        for i, ip in enumerate(ips):
            mac = self.get(int(ip))
            found.append(int(mac is not None))
            macs.append(mac or ZERO_MAC)
            if mac is not None and link is not None and link[i] < len(self.links):
                self.links[link[i]]["dst_mac"] = np.frombuffer(mac, np.uint8)
        return np.array(found, np.uint32), np.frombuffer(b"".join(macs), np.uint8).reshape(-1, 6)
