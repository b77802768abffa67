"""TEST INFRASTRUCTURE ONLY: a go-back-N sender, a lossy network, a lazy application and a byte-stream checker for the
TCP receive path, in plain Python / numpy.

Connection c's byte at stream offset p is `stream_bytes(c, p)`, a fixed hash of (c, p), so any delivered or stored view
can be checked against the stream without keeping what was sent. Each round the sender resends every open connection's
stream from the receiver's RCV.NXT, cut afresh with an MSS drawn for the round, as real frames (tests/frames.py) with
several header layouts; during the lossy phase the network drops, duplicates and locally reorders whole frames; after
each call the application reads part of what is unread (Receiver::pop, ctrlblk.rs:113-129: reader_next moves) and the
caller rewrites the out-of-order store's batch-index refs to handles 0x80000000 | global frame number (the carry
protocol of INTEGRATION.md).

`StreamChecker` has no oracle inside: it is fed one call's outputs, the table after it and the frame bytes, and asserts
  S1  per connection the delivered views (EOF and empty buffers aside) are the stream's next bytes: no gap, no repeat,
      no foreign byte, read from the blob at off[frame] + view.off
  S2  RCV.NXT - IRS (wrapping) = bytes delivered so far (+ 1 once closed by FIN); RCV.NXT never moves backwards
  S3  every store entry k < ooo_count is non-empty and holds the stream's bytes at ooo_start[k] - IRS; ooo_count <= 16;
      entries past the count are zero
  S4  every processed frame's view lies inside the payload the builder gave that frame
  S5  (finish) every connection that was not reset delivered its whole stream, is CLOSED, RCV.NXT = the sender's final
      SND.NXT, within the call cap.
`trace(case)` runs a case once through the oracle chain (OraclePeer.process -> tcp_process) and records every call, so
the CPU tests and every GPU walk replay the same batches against the same recorded reference.
"""
from __future__ import annotations

import functools
import struct
from dataclasses import dataclass, field

import numpy as np

import frames as F
from demikernel_amd import _native as N
from demikernel_amd import synth

M32 = 0xFFFFFFFF
HANDLE = 0x80000000
EOF = N.DK_TCP_REF_EOF
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
CALL_CAP = 64
OOO_MAX = N.DK_TCP_OOO_MAX
TS_OPTION = bytes([1, 1, 8, 10]) + b"\x00\x00\x00\x01\x00\x00\x00\x02"  # NOP NOP TS: payload at 66
IHL6, IHL15 = bytes([1, 1, 1, 0]), bytes([1] * 39 + [0])


def stream_bytes(c, p) -> np.ndarray:
    """The stream of connection(s) c at offset(s) p (arrays broadcast): a 32-bit integer hash, not periodic in p."""
    x = (np.asarray(p, np.uint64) + np.asarray(c, np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & np.uint64(M32)
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    return (x & np.uint64(0xFF)).astype(np.uint8)


@dataclass(frozen=True)
class Case:
    name: str
    nconns: int
    stream: int
    buffer: int
    mss: tuple
    flight: int            # a flight is 1 .. flight segments
    lossy: int             # rounds of the lossy phase
    loss: float = 0.1
    dup: float = 0.1
    span: int = 8          # local reordering: a frame moves up to this many places
    stall: int = -1        # this connection's reader stalls until its window is zero, then resumes
    strays: bool = False
    listener: bool = False  # one more row, the Passive flow's: not a connection (DK_TCP_NONE)
    seed: int = 1


CASES = {c.name: c for c in [
    Case("one_long", 1, 60000, 8192, (64, 16, 7), 1500, 14, loss=0.01, dup=0.02, span=6, seed=11),
    Case("few_windowed", 7, 20000, 2000, (33, 100), 300, 18, loss=0.05, dup=0.05, seed=12),
    Case("many_reordered", 40, 1500, 65536, (8, 64), 60, 16, loss=0.1, dup=0.3, span=40, seed=13),
    Case("tiny_window", 3, 6000, 300, (1, 5, 64), 400, 14, loss=0.3, dup=0.1, span=5, stall=1, seed=14),
    Case("wide_254", 254, 400, 512, (8, 40), 7, 10, loss=0.15, dup=0.1, span=300, listener=True, seed=15),
    Case("wide_300", 300, 400, 512, (8, 40), 7, 10, loss=0.15, dup=0.1, span=300, listener=True, seed=16),
    Case("strays", 7, 20000, 2000, (33, 100), 300, 18, loss=0.05, dup=0.05, strays=True, seed=17),
]}
# Built on the GPU by dk_tcp_tx_segment (tests/test_gpu_tcp_streams.py): flight = the send window in segments.
DEVICE_CASE = Case("device_sender", 6, 4000, 2000, (37, 64, 100), 40, 8, loss=0.1, dup=0.1, span=12, seed=18)
RESET_AT = {1: 6, 4: 12}  # strays: connection -> the round from which an RST at RCV.NXT is sent until it lands


def initial_table(case: Case):
    """(flows, table, irs): the receiving peer's Active flows and its connection table at the start. The strays case
    has two more rows, one DK_TCP_NONE and one DK_TCP_CLOSED, whose frames the engine must leave alone; the wide cases
    have the listener's row."""
    rows = case.nconns + (2 if case.strays else 0)
    flows = synth.make_flows(rows, passive=case.listener, seed=case.seed)
    rows = len(flows)
    rng = np.random.default_rng(case.seed)
    irs = rng.integers(0, 1 << 32, rows, dtype=np.uint64)
    near = np.arange(rows) % 3 == 0  # these wrap 2^32 inside the first calls
    irs[near] = (1 << 32) - 1 - rng.integers(0, min(case.stream, 200), rows, dtype=np.uint64)[near]
    irs = irs.astype(np.uint32)
    t = np.zeros(rows, N.CONN_DTYPE)
    t["state"] = N.DK_TCP_ESTABLISHED
    t["receive_next"] = t["reader_next"] = irs
    t["buffer_size"] = case.buffer
    t["send_next"] = 1000 + np.arange(rows)
    t["state"][case.nconns:] = N.DK_TCP_NONE
    if case.strays:
        t["state"][case.nconns + 1] = N.DK_TCP_CLOSED
    return flows, t, irs


@dataclass
class Call:
    """One receive call: the batch (descriptors into `blob`; duplicates repeat a descriptor), each descriptor's global
    frame number and payload as built, the table it started from, the oracle's outputs and table after it (before the
    handle rewrite), and what the application read afterwards."""
    blob: np.ndarray
    off: np.ndarray
    lens: np.ndarray
    gidx: np.ndarray
    pay_off: np.ndarray
    pay_len: np.ndarray
    conn: np.ndarray
    lossy: bool
    start: np.ndarray = None
    exp: dict = None
    exp_table: np.ndarray = None
    reads: np.ndarray = None


@dataclass
class Trace:
    case: Case
    flows: np.ndarray
    table0: np.ndarray
    irs: np.ndarray
    calls: list = field(default_factory=list)
    final_snd_nxt: np.ndarray = None
    final_table: np.ndarray = None
    exempt: tuple = ()
    done: bool = False


# ---------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------
class FrameStore:
    """Every distinct frame of a case, built once: bytes, global frame number, payload offset and length."""

    def __init__(self, flows, table0, irs):
        self.flows, self.irs, self.snd = flows, irs, table0["send_next"]
        self.frames, self.pay, self.index = [], [], {}

    def _add(self, key, frame: bytes, pay_off: int, pay_len: int) -> int:
        g = len(self.frames)
        self.frames.append(frame)
        self.pay.append((pay_off, pay_len))
        self.index[key] = g
        return g

    def segment(self, c: int, p: int, ln: int, fin: bool, kind: str = "data") -> int:
        """Connection c's stream bytes [p, p + ln) (+ FIN) as a frame. kind: data; syn (a SYN copy: the SYN takes the
        sequence number before the data, ctrlblk.rs:474-476, :512-516); noack; unsent (acknowledges beyond SND.NXT);
        ack (no data); rst; badsum (TCP checksum wrong: never reaches TCP)."""
        key = (c, p, ln, fin, kind)
        g = self.index.get(key)
        if g is not None:
            return g
        fl = self.flows[c]
        payload = stream_bytes(c, np.arange(p, p + ln)).tobytes() if kind not in ("ack", "rst") else b""
        seq, ack = (int(self.irs[c]) + p) & M32, int(self.snd[c])
        flags = ACK | (PSH if payload else 0) | (FIN if fin else 0)
        kw = {}
        if kind == "syn":
            seq, flags = (seq - 1) & M32, flags | SYN
        elif kind == "noack":
            flags &= ~ACK
        elif kind == "unsent":
            ack = (ack + 5) & M32
        elif kind == "rst":
            flags = RST | ACK
        elif kind == "badsum":
            kw["checksum"] = 0x1234
        v = (c + p + ln) % 5  # header layout: payload at 54 / 66 / 58 / 54 / 54 or 94
        options = TS_OPTION if v == 1 else b""
        ip_options = IHL6 if v == 2 else IHL15 if v == 4 and (p // 7) % 3 == 0 else b""
        short = 54 + len(options) + len(ip_options) + len(payload)
        frame = F.tcp_frame(payload, src=int(fl["remote_ip"]), dst=int(fl["local_ip"]), sport=int(fl["remote_port"]),
                            dport=int(fl["local_port"]), options=options, ip_options=ip_options,
                            pad=max(0, synth.ETH_MIN_FRAME - short),  # Ethernet padding behind the IP length
                            tcp_kw=dict(seq=seq, ack=ack, flags=flags, **kw))
        return self._add(key, frame, 54 + len(options) + len(ip_options), len(payload))

    def udp(self, k: int) -> int:
        key = ("udp", k)
        if key in self.index:
            return self.index[key]
        return self._add(key, F.udp_frame(struct.pack("!I", k) * 5, dst=synth.BOB_IPV4, dport=9), 42, 20)

    def pack(self, g: np.ndarray):
        """A call's blob: its distinct frames in slots at 0 and 2 mod 16, and (off, len) per descriptor of g."""
        uniq, inv = np.unique(g, return_inverse=True)
        offs, pos = np.zeros(len(uniq), np.uint32), 0
        for k, u in enumerate(uniq):
            pos = (pos + 15) // 16 * 16 + (2 if u & 1 else 0)
            offs[k] = pos
            pos += len(self.frames[u])
        blob = np.zeros(max(pos, 1), np.uint8)
        for k, u in enumerate(uniq):
            f = self.frames[u]
            blob[offs[k]:offs[k] + len(f)] = np.frombuffer(f, np.uint8)
        lens = np.array([len(self.frames[u]) for u in uniq], np.uint16)
        pay = np.array([self.pay[u] for u in uniq], np.uint32).reshape(-1, 2)
        return blob, offs[inv], lens[inv], pay[inv, 0], pay[inv, 1]


# ---------------------------------------------------------------------------------------------------------------------
# sender, network, application
# ---------------------------------------------------------------------------------------------------------------------
def cut_flight(start: int, length: int, mss: int, nseg: int, fin_on_data: bool) -> list:
    """Go-back-N from stream offset `start`: up to nseg segments (p, len, fin) of at most mss bytes; the stream ends in
    FIN, on the last data segment or as a FIN-only segment."""
    segs, p = [], start
    while len(segs) < nseg:
        if p < length:
            ln = min(mss, length - p)
            fin = p + ln == length and fin_on_data
            segs.append((p, ln, fin))
            p += ln
            if fin:
                break
        else:
            segs.append((length, 0, True))
            break
    return segs


def network(conn: np.ndarray, rank: np.ndarray, lossy: bool, case: Case, rng) -> np.ndarray:
    """The order in which the sender's frames (connection, position in its flight) arrive: connections interleaved,
    each in order; in the lossy phase frames are dropped, duplicated and moved up to case.span places."""
    idx = np.lexsort((conn, rank))
    if not lossy:
        return idx
    pos = np.arange(len(idx), dtype=np.float64)
    keep = rng.random(len(idx)) >= case.loss
    idx, pos = idx[keep], pos[keep]
    d = rng.random(len(idx)) < case.dup  # a duplicate is the same frame again: a repeated descriptor, not a copy
    idx, pos = np.concatenate([idx, idx[d]]), np.concatenate([pos, pos[d] + 1])
    return idx[np.argsort(pos + rng.random(len(idx)) * case.span, kind="stable")]


def carry_refs(table: np.ndarray, gidx: np.ndarray) -> None:
    """The ref carry protocol: every store entry whose ref is an index of this batch becomes 0x80000000 | global frame
    number; entries already carrying a handle are left alone."""
    k = np.arange(OOO_MAX)[None, :] < table["ooo_count"][:, None]
    ref = table["ooo"]["ref"]
    mine = k & (ref < HANDLE)
    ref[mine] = HANDLE | gidx[ref[mine]]


def after_call(table: np.ndarray, call: Call) -> None:
    """What the caller does to its table between two calls: the handle rewrite, then the application's reads."""
    carry_refs(table, call.gidx)
    table["reader_next"] += call.reads


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
class StreamChecker:
    def __init__(self, irs: np.ndarray, length: int, table0: np.ndarray):
        self.irs, self.length = irs.astype(np.uint32), length
        self.rcv_nxt = table0["receive_next"].copy()
        self.delivered = np.zeros(len(irs), np.int64)
        self.fin = np.zeros(len(irs), bool)
        self.carry = np.zeros(0, np.uint8)   # the bytes of every frame a handle was made for
        self.carry_at = {}                   # global frame number -> (offset in carry, length)
        self.via_handle = 0                  # deliveries resolved through a carried handle
        self.calls = 0

    def _resolve(self, ref, voff, vlen, nblob, off, lens, what):
        """Byte positions (in blob ++ carry) of views given as batch indices or carried handles; checks they lie in
        their frames."""
        base = np.zeros(len(ref), np.int64)
        h = ref >= HANDLE
        b = ~h
        assert (ref[b] < len(off)).all(), f"{what}: ref {ref[b][ref[b] >= len(off)][:4]} is no frame of this batch"
        assert (voff[b].astype(np.int64) + vlen[b] <= lens[ref[b]]).all(), f"{what}: view past its frame's end"
        base[b] = off[ref[b]].astype(np.int64) + voff[b]
        for k in np.nonzero(h)[0]:
            g = int(ref[k]) & ~HANDLE
            assert g in self.carry_at, f"{what}: handle of frame {g} was never carried"
            o, ln = self.carry_at[g]
            assert int(voff[k]) + int(vlen[k]) <= ln, f"{what}: view past its carried frame's end"
            base[k] = nblob + o + int(voff[k])
        return base

    def _same_bytes(self, src, base, vlen, conn, pos, what):
        """src[base[k] .. + vlen[k]) == stream(conn[k], pos[k] ..) for every k."""
        vlen = vlen.astype(np.int64)
        assert (pos >= 0).all() and (pos + vlen <= self.length).all(), \
            f"{what}: bytes outside the stream at {np.nonzero((pos < 0) | (pos + vlen > self.length))[0][:4]}"
        within = np.arange(vlen.sum()) - np.repeat(np.cumsum(vlen) - vlen, vlen)
        got = src[np.repeat(base, vlen) + within]
        exp = stream_bytes(np.repeat(conn, vlen), np.repeat(pos, vlen) + within)
        if not np.array_equal(got, exp):
            k = np.repeat(np.arange(len(vlen)), vlen)[np.nonzero(got != exp)[0][0]]
            raise AssertionError(f"{what}: view {k} of connection {conn[k]} does not hold the stream's bytes at "
                                 f"{pos[k]}")

    def feed(self, out: dict, table: np.ndarray, blob, off, lens, gidx, pay_off, pay_len) -> None:
        """One call: `out` = action, view, deliv, deliv_start, deliv_count; `table` after the call, before the handle
        rewrite; the batch's frame bytes and descriptors; each descriptor's global frame number and built payload."""
        ctx = f"call {self.calls}"
        self.calls += 1
        n, nc = len(off), len(table)
        blob = np.asarray(blob, np.uint8)
        src = np.concatenate([blob, self.carry])
        # S4
        proc = np.nonzero(out["action"] != N.A["SKIP"])[0]
        v = out["view"][proc]
        assert (v["ref"] == proc).all(), f"{ctx} S4: a processed frame's view names another frame"
        lo, hi = pay_off[proc].astype(np.int64), pay_off[proc].astype(np.int64) + pay_len[proc]
        bad = (v["off"] < lo) | (v["off"].astype(np.int64) + v["len"] > hi)
        assert not bad.any(), f"{ctx} S4: views outside the payload at frames {proc[bad][:4]}"
        # S1
        cnt = out["deliv_count"].astype(np.int64)
        conn = np.repeat(np.arange(nc), cnt)
        slot = (np.repeat(out["deliv_start"].astype(np.int64), cnt) + np.arange(cnt.sum()) -
                np.repeat(np.cumsum(cnt) - cnt, cnt))
        d = out["deliv"][slot]
        eof = d["ref"] == EOF
        last = np.zeros(len(d), bool)
        last[np.cumsum(cnt)[cnt > 0] - 1] = True
        assert not (eof & ~last).any(), f"{ctx} S1: an EOF buffer is not the last delivery"
        assert not (eof & self.fin[conn]).any(), f"{ctx} S1: a second EOF"
        assert not (self.fin[conn] & ~eof).any(), f"{ctx} S1: delivery after EOF"
        data = ~eof & (d["len"] > 0)
        dc, dv = conn[data], d[data]
        ln = dv["len"].astype(np.int64)
        run = np.cumsum(ln) - ln  # bytes before each delivery in this call; minus those of earlier connections
        firstrun = np.zeros(nc, np.int64)
        if len(dc):
            firstk = np.unique(dc, return_index=True)
            firstrun[firstk[0]] = run[firstk[1]]
        pos = self.delivered[dc] + run - firstrun[dc]
        base = self._resolve(dv["ref"], dv["off"], dv["len"], len(blob), off, lens, f"{ctx} S1")
        self._same_bytes(src, base, dv["len"], dc, pos, f"{ctx} S1")
        self.via_handle += int((dv["ref"] >= HANDLE).sum())
        np.add.at(self.delivered, dc, ln)
        self.fin[conn[eof]] = True
        # S2
        adv = (table["receive_next"] - self.rcv_nxt).astype(np.int32)
        assert (adv >= 0).all(), f"{ctx} S2: RCV.NXT moved backwards on {np.nonzero(adv < 0)[0][:4]}"
        self.rcv_nxt = table["receive_next"].copy()
        want = (self.delivered + self.fin) & M32
        got = (table["receive_next"] - self.irs).astype(np.uint32)
        assert (got == want).all(), (f"{ctx} S2: RCV.NXT - IRS {got[got != want][:4]} != delivered (+ FIN) "
                                     f"{want[got != want][:4]} on {np.nonzero(got != want)[0][:4]}")
        assert not (self.fin & (table["state"] != N.DK_TCP_CLOSED)).any(), f"{ctx} S2: EOF delivered, not CLOSED"
        # S3
        cntk = table["ooo_count"]
        assert (cntk <= OOO_MAX).all(), f"{ctx} S3: ooo_count above {OOO_MAX}"
        live = np.arange(OOO_MAX)[None, :] < cntk[:, None]
        e = table["ooo"]
        dead = ~live
        assert not (table["ooo_start"][dead].any() or e["ref"][dead].any() or e["off"][dead].any() or
                    e["len"][dead].any()), f"{ctx} S3: entries past the count are not zero"
        sc = np.nonzero(live)[0]
        sv, ss = e[live], table["ooo_start"][live]
        assert (sv["len"] > 0).all(), f"{ctx} S3: an empty store entry"
        spos = (ss - self.irs[sc]).astype(np.uint32).astype(np.int64)
        sbase = self._resolve(sv["ref"], sv["off"], sv["len"], len(blob), off, lens, f"{ctx} S3")
        self._same_bytes(src, sbase, sv["len"], sc, spos, f"{ctx} S3")
        # the frames the caller is about to make handles for
        new = np.unique(sv["ref"][sv["ref"] < HANDLE])
        for i in new:
            g = int(gidx[i])
            if g not in self.carry_at:
                self.carry_at[g] = (len(self.carry), int(lens[i]))
                self.carry = np.concatenate([self.carry, blob[int(off[i]):int(off[i]) + int(lens[i])]])

    def finish(self, table: np.ndarray, final_snd_nxt: np.ndarray, exempt=(), cap: int = CALL_CAP) -> None:
        """S5."""
        assert self.calls <= cap, f"S5: {self.calls} calls, the cap is {cap}"
        for c in range(len(table)):
            if c in exempt:
                continue
            assert self.delivered[c] == self.length and self.fin[c], \
                f"S5: connection {c} delivered {self.delivered[c]} of {self.length} bytes, EOF {self.fin[c]}"
            assert table["state"][c] == N.DK_TCP_CLOSED and table["receive_next"][c] == final_snd_nxt[c], \
                f"S5: connection {c} state {table['state'][c]} RCV.NXT {table['receive_next'][c]} != {final_snd_nxt[c]}"


# ---------------------------------------------------------------------------------------------------------------------
# a case, run once through the oracle chain
# ---------------------------------------------------------------------------------------------------------------------
def reads_after(table, case: Case, lossy: bool, st: dict, rng) -> np.ndarray:
    """What the application reads after a call: a random part of the unread bytes in the lossy phase, everything in
    the lossless phase; the stalled reader nothing until one call has started with a zero window."""
    unread = (table["receive_next"] - table["reader_next"]).astype(np.uint32)
    reads =(rng.random(len(table)) * (unread.astype(np.float64) + 1)).astype(np.uint32) if lossy else unread.copy()
    reads = np.minimum(reads, unread)
    s = case.stall
    if s >= 0 and not st.get("resumed"):
        reads[s] = 0
        if unread[s] == table["buffer_size"][s]:
            if st.get("zero_seen"):
                reads[s], st["resumed"] = unread[s], True
            st["zero_seen"] = True
    return reads


@functools.lru_cache(maxsize=None)
def trace(name: str) -> Trace:
    from oracle import oracle as O
    from oracle.oracle import OraclePeer

    case = CASES[name]
    flows, table, irs = initial_table(case)
    tr = Trace(case, flows, table.copy(), irs)
    store = FrameStore(flows, table, irs)
    peer = OraclePeer(synth.ipv4(synth.BOB_IPV4))
    peer.set_flows(flows)
    rng = np.random.default_rng(case.seed + 1000)
    L, st = case.stream, {}
    inert = tuple(range(case.nconns, len(table)))
    for rnd in range(CALL_CAP + 8):
        opened = [c for c in range(case.nconns) if table["state"][c] == N.DK_TCP_ESTABLISHED]
        if not opened:
            tr.done = True
            break
        lossy = rnd < case.lossy
        g, conn, rank = [], [], []

        def put(c, k, gi):
            g.append(gi), conn.append(c), rank.append(k)

        for c in opened:
            start = (int(table["receive_next"][c]) - int(irs[c])) & M32
            segs = cut_flight(start, L, int(rng.choice(case.mss)), int(rng.integers(1, case.flight + 1)),
                              bool(rng.random() < 0.5))
            for k, (p, ln, fin) in enumerate(segs):
                put(c, k, store.segment(c, p, ln, fin))
                if case.strays and rng.random() < 0.04:
                    kind = ("syn", "noack", "unsent", "ack", "badsum", "udp")[int(rng.integers(0, 6))]
                    put(c, k, store.udp(int(rng.integers(0, 8))) if kind == "udp" else
                        store.segment(c, p, 0 if kind == "ack" else ln, False, kind))
            if case.strays and c in RESET_AT and rnd >= RESET_AT[c]:
                k = int(rng.integers(0, len(segs)))  # mid-flight, behind segment k at the sequence number that ends at
                put(c, k, store.segment(c, segs[k][0] + segs[k][1], 0, False, "rst"))
        if case.strays:
            for c in inert:  # rows that are no connection / a closed one: their frames are left alone
                for k, (p, ln, fin) in enumerate(cut_flight(0, L, 50, 3, True)):
                    put(c, k, store.segment(c, p, ln, fin))
        g, conn, rank = np.array(g), np.array(conn), np.array(rank)
        idx = network(conn, rank, lossy, case, rng)
        if len(idx) == 0:
            idx = np.array([0])
        blob, off, lens, pay_off, pay_len = store.pack(g[idx])
        call = Call(blob, off, lens, g[idx].astype(np.uint32), pay_off, pay_len, conn[idx], lossy, start=table.copy())
        rx = peer.process(blob, off, lens)
        call.exp = O.tcp_process(table, rx)
        call.exp_table = table.copy()
        call.reads = reads_after(table, case, lossy, st, rng)
        after_call(table, call)
        tr.calls.append(call)
    tr.final_snd_nxt = (irs.astype(np.uint64) + L + 1).astype(np.uint32)
    tr.exempt = tuple(c for c in RESET_AT if case.strays) + inert
    tr.final_table = table
    return tr


def check_trace(tr: Trace, outputs=None) -> StreamChecker:
    """StreamChecker over a whole trace: the recorded oracle outputs, or `outputs(k, call) -> (out, table, blob)`."""
    chk = StreamChecker(tr.irs, tr.case.stream, tr.table0)
    for k, call in enumerate(tr.calls):
        out, table, blob = (call.exp, call.exp_table, call.blob) if outputs is None else outputs(k, call)
        chk.feed(out, table, blob, call.off, call.lens, call.gidx, call.pay_off, call.pay_len)
    return chk


def guards(tr: Trace) -> dict:
    """Coverage of a trace, from the oracle's run: calls x connections (established, with a frame in the call) that
    start with a non-empty store, a store front behind RCV.NXT, a pending FIN, unread bytes, a zero window; the action
    histogram; whether an IRS wrapped."""
    g = dict(store=0, stale=0, fin_pending=0, unread=0, zero_window=0, segments=0, calls=len(tr.calls),
             actions=np.zeros(len(N.TCP_ACTIONS), np.int64))
    for call in tr.calls:
        t = call.start
        act = (t["state"] == N.DK_TCP_ESTABLISHED) & (np.bincount(call.conn, minlength=len(t)) > 0)
        unread = (t["receive_next"] - t["reader_next"]).astype(np.uint32)
        front = (t["ooo_start"][:, 0] - t["receive_next"]).astype(np.int32)
        g["store"] += int((act & (t["ooo_count"] > 0)).sum())
        g["stale"] += int((act & (t["ooo_count"] > 0) & (front < 0)).sum())
        g["fin_pending"] += int((act & (t["fin_pending"] != 0)).sum())
        g["unread"] += int((act & (unread > 0)).sum())
        g["zero_window"] += int((act & (unread == t["buffer_size"])).sum())
        g["segments"] += len(call.off)
        g["actions"] += np.bincount(call.exp["action"], minlength=len(N.TCP_ACTIONS))
    ft = tr.final_table
    g["wrapped"] = int(((ft["receive_next"] < tr.irs) & (ft["state"] != N.DK_TCP_NONE))[:tr.case.nconns].sum())
    return g
