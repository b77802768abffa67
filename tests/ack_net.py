"""TEST INFRASTRUCTURE ONLY: a whole transfer over a lossy network seen from the sender, in plain Python / numpy: the
send side of tests/stream_net.py. A closed loop that runs entirely on the host and is recorded once per case; the CPU
tests and every form of dk_tcp_ack_process on the GPU replay the recording.

Sender A pushes connection c's stream (stream_net.stream_bytes) and an end-of-send marker. Each round
tx_segment_reference.segment cuts what the send window (whatever the peer last advertised) lets out, `append_frames`
(UnackedQueue.append_frames in numpy) queues the frames, and after the network and the peer the ACKs that come back
go through A's receive side (OraclePeer.process -> tcp_process) and tcp_ack_reference.ack_process.

What stays with the host (sender.rs:320-403, restated): a virtual clock in nanoseconds; a timer per connection at
rtx_base_ns + rto. When it fires the front entry is resent as it stands (retransmit(): from its moved `off` if it was
trimmed, the marker as a FIN, sequence number SND.UNA), its tx_time becomes NONE, rto = min(2 rto, 60) is written into
the table (RtoCalculator::back_off) and rtx_base_ns = now. The harness's own policy, not the reference's congestion
control: a call that reports dup_acks[c] >= 3 is followed by one immediate retransmission of the front (tx_time NONE,
the timer left alone). When a round has nothing to send the clock jumps to the earliest deadline.

The network, during the first `lossy` rounds, drops, duplicates and locally reorders data frames and ACK frames, and
splits some data frames in two (tests/frames.py), so that the peer acknowledges the middle of a queue entry; now and
then it adds an ACK beyond SND.NXT. In the fin_lost case every connection's first FIN is dropped in any round.

Peer B is a plain host model: it parses A's frames, keeps the bytes it has (a mask over the stream: the reassembly
intervals are its runs) and answers every arriving frame with one ACK: the cumulative ack number and a window drawn
from [MSS, flight x MSS] in units of 1 << snd_wscale, never zero (there is no persist timer). In the peer_data cases
every ACK carries 0..8 bytes of B's own stream, resent each round from A's RCV.NXT on: seq advances, wl1 moves, A's
receive side returns DELIVERED, STORED and DUPLICATE, and reordered ACKs exercise the window-update rule.

`AckChecker` has no reference inside. It is fed each call's outputs, the tables and the pool after the call, and the
host's own log (the state the call started from, the frames it built, its sends and retransmissions), and asserts
  T1  SND.UNA never moves backwards: after a call it is the highest ack number in (SND.UNA, SND.NXT] among the call's
      processed frames, or its old value; SND.NXT is left alone. (wl1, wl2, snd_wnd) are untouched, or those of the
      first processed frame that carries ack == wl2, which is above the old SND.UNA; wl1 never moves backwards
  T2  the live entries are contiguous in the source blob, the front's off is the stream offset of SND.UNA, sum of len
      (+ 1 for the marker, which is last) == SND.NXT - SND.UNA, the queue's end did not move, and no pool entry but
      the new front changed
  T3  bytes_acked == SND.UNA's advance == the sum of acked[] over the call's new ACKs (0 < acked < 2^31), new_acks and
      dup_acks count them and the zeros, new_acks + dup_acks <= processed frames, acked == 0 on every other frame;
      over all calls bytes_acked sums to SND.UNA - ISN
  T4  (Karn) every live tx_time is the time the log has for that entry's first send, and NONE once the entry was
      retransmitted or trimmed; samples == the entries the call touched (popped or trimmed) whose time was not NONE
  T5  0.1 <= rto <= 60; after a call with a new ACK rtx_armed == (q_count != 0) and rtx_base_ns is the front's
      tx_time, now where that is NONE, 0 when empty; without a new ACK the connection's rows are untouched; without a
      sample srtt / rttvar / rto keep their bits, with one rto == clamp(srtt + max(0.001, 4 rttvar)) and srtt lies
      between the smallest and the largest sample the log allowed so far (a weighted mean of them, 1e-12 for rounding)
  T6  (finish) SND.UNA == SND.NXT == ISN + stream + 1, queues empty, timers disarmed, B has exactly the stream and
      the FIN, within CALL_CAP calls.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

import frames as F
import stream_net as SN
import tcp_ack_reference as R
import tx_segment_reference as M
from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_ack import TCP_HEADERS, ack_conn_table

M32 = 0xFFFFFFFF
NONE = N.DK_TCP_TX_TIME_NONE
FIN, PSH, ACK = 0x01, 0x08, 0x10
HANDLE = SN.HANDLE
CALL_CAP = 128  # a condition: every case's all-host run finishes within it (tests/test_ack_net.py)
SEC = 10**9
PEER_STREAM = 1000  # B's own stream on connection c is stream_bytes(PEER_STREAM + c, .)


@dataclass(frozen=True)
class Case:
    name: str
    nconns: int
    stream: int
    mss: tuple             # connection c cuts with mss[c % len]; from round mss_switch on with the next one
    flight: tuple          # B's windows are lo .. hi segments of the connection's MSS
    lossy: int             # rounds of the lossy phase
    loss: float = 0.1
    dup: float = 0.1
    span: int = 8          # local reordering of data frames
    ack_span: int = 8      # and of ACK frames
    split: float = 0.1     # data frames cut in two, lossy phase
    peer_data: bool = False
    listener: bool = False
    fin_lost: bool = False
    mss_switch: int = -1
    seed: int = 1


CASES = {c.name: c for c in [
    Case("one_long", 1, 60000, (7, 16), (1100, 1600), 6, loss=0.01, dup=0.02, span=6, ack_span=6, split=0.1,
         mss_switch=5, seed=30),
    Case("few", 7, 20000, (33, 100), (1, 40), 12, loss=0.05, dup=0.05, peer_data=True, seed=22),
    Case("many", 40, 1500, (8, 64), (1, 6), 14, loss=0.1, dup=0.15, span=40, ack_span=40, seed=23),
    Case("wide_300", 300, 400, (8, 40), (1, 7), 8, loss=0.15, dup=0.1, span=300, ack_span=300, listener=True,
         seed=24),
    Case("fin_lost", 3, 2000, (64,), (1, 4), 10, loss=0.1, dup=0.1, span=5, ack_span=5, fin_lost=True, seed=25),
    Case("piggy", 5, 5000, (100,), (1, 10), 12, loss=0.1, dup=0.1, ack_span=12, peer_data=True, seed=26),
]}


# ---------------------------------------------------------------------------------------------------------------------
# the recording
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Round:
    """One round as the host saw it. Before the sends: mss (the whole column of the TX table), the connections whose
    front entry is retransmitted (tx_time := NONE), the rto and rtx_base_ns values the timer wrote. The sends: the
    push list and what tx_segment_reference.segment made of it (frames, results, the TX table after), at t_send. The
    ACK call (None when no ACK frame arrived): the batch, the harness's own description of each frame (connection,
    seq, ack, raw window), now, the tables and the pool the call started from, and the recorded results."""
    mss: np.ndarray
    rtx: np.ndarray
    rto_set: tuple
    base_set: tuple
    t_send: int
    push: tuple = None
    seg: dict = None
    sends: tuple = None      # (conn, off, len) of the entries appended
    rtx_keys: list = field(default_factory=list)  # (conn, end offset, is marker) of the entries retransmitted
    ack: SimpleNamespace = None
    lossy: bool = False


@dataclass
class Trace:
    case: Case
    flows: np.ndarray
    rx0: np.ndarray
    tx0: np.ndarray
    ak0: np.ndarray
    isn: np.ndarray
    irs: np.ndarray
    src: np.ndarray
    links: np.ndarray
    cap: int                 # queue entries per connection
    stride: int
    max_frames: int
    rounds: list = field(default_factory=list)
    done: bool = False
    peer_got: list = None    # B's bytes per connection
    peer_fin: np.ndarray = None
    final: dict = None
    stats: dict = field(default_factory=dict)

    @property
    def calls(self):
        return [r for r in self.rounds if r.ack is not None]


def mss_of(case: Case, rnd: int, rows: int) -> np.ndarray:
    k = np.arange(rows) + (1 if 0 <= case.mss_switch <= rnd else 0)
    return np.asarray(case.mss, np.uint32)[k % len(case.mss)]


def initial(case: Case) -> Trace:
    """A's socket table, its three connection tables, the source blob (connection c's stream at c * stream)."""
    flows = synth.make_flows(case.nconns, passive=case.listener, seed=case.seed)
    rows, nc, L = len(flows), case.nconns, case.stream
    rng = np.random.default_rng(case.seed)
    isn, irs = (rng.integers(0, 1 << 32, rows, dtype=np.uint64) for _ in range(2))
    near = np.arange(rows) % 3 == 0  # these wrap 2^32 inside the first calls
    isn[near] = (1 << 32) - 1 - rng.integers(0, 200, rows, dtype=np.uint64)[near]
    irs[near] = (1 << 32) - 1 - rng.integers(0, 200, rows, dtype=np.uint64)[near]
    isn, irs = isn.astype(np.uint32), irs.astype(np.uint32)
    peer = flows.copy()  # conns_toward builds the send sides of a table's remote ends: A is the remote end of B's
    peer["local_ip"], peer["remote_ip"] = flows["remote_ip"], flows["local_ip"]
    peer["local_port"], peer["remote_port"] = flows["remote_port"], flows["local_port"]
    mss0 = mss_of(case, 0, rows)
    wsmax = min(14, int(np.log2(max(case.flight[1] * min(case.mss) // 4, 1))))  # the unit: a quarter of the flight
    ws = (wsmax - np.arange(rows)) % (wsmax + 1)
    tx = M.conns_toward(peer, seed=case.seed, snd_nxt=isn, rcv_nxt=irs, rcv_wnd_hdr=65535, mss=mss0, link=0,
                        snd_wnd=quantize(mss0.astype(np.int64) * case.flight[0], mss0, ws) << ws)
    ak = ack_conn_table(rows, wl1=irs, wl2=isn, snd_wscale=ws)
    rx = conn_table(rows, receive_next=irs, send_next=isn, buffer_size=1 << 20)
    for t in (tx, rx):
        t["state"][nc:] = N.DK_TCP_NONE
    src = SN.stream_bytes(np.repeat(np.arange(nc), L), np.tile(np.arange(L), nc))
    # twice the largest window in segments: a window that opens by a few bytes lets a short frame out
    cap = 2 * (case.flight[1] * max(case.mss) // min(case.mss) + (1 << wsmax) // min(case.mss)) + 8
    stride = (TCP_HEADERS + max(case.mss) + 63) // 64 * 64
    return Trace(case, flows, rx, tx, ak, isn, irs, src, np.ascontiguousarray(M.links_table()), cap, stride,
                 max_frames=nc * cap)


def quantize(want, mss, ws):
    """The raw header window for `want` bytes at scale ws: at least one MSS, never zero."""
    mss, ws = np.asarray(mss, np.int64), np.asarray(ws, np.int64)
    raw = (np.maximum(np.asarray(want, np.int64), mss) + (1 << ws) - 1) >> ws
    assert (raw >= 1).all() and (raw <= 0xFFFF).all()
    return raw


def append_frames(ak: np.ndarray, pool: dict, cap: int, conn, off, lens, now: int) -> None:
    """UnackedQueue.append_frames on host arrays, in place: every connection's live entries move to the start of its
    region (the rest of the region zero), the frames follow, a disarmed timer is armed at `now`."""
    nc = len(ak)
    nq = nc * cap
    qf, qc = ak["q_first"].astype(np.int64), ak["q_count"].astype(np.int64)
    j = np.arange(cap)[None, :]
    live = j < qc[:, None]
    at = np.minimum(qf[:, None] + j, max(nq - 1, 0))
    for k in pool:
        pool[k][:] = np.where(live, pool[k][at], 0).reshape(-1)
    conn = np.asarray(conn, np.int64)
    cnt = np.bincount(conn, minlength=nc)
    start = np.cumsum(cnt) - cnt  # a connection's frames are consecutive
    assert (np.diff(conn) >= 0).all() and (qc + cnt <= cap).all(), "a connection's entries exceed its capacity"
    pos = conn * cap + qc[conn] + (np.arange(len(conn)) - start[conn])
    pool["off"][pos], pool["len"][pos], pool["tx_time"][pos] = off, lens, now
    ak["q_first"], ak["q_count"] = np.arange(nc) * cap, qc + cnt
    arm = (ak["rtx_armed"] == 0) & (cnt > 0)
    ak["rtx_armed"][arm] = 1
    ak["rtx_base_ns"][arm] = now


def sent_entries(push, seg) -> tuple:
    """(conn, off, len) of the queue entries for the frames a segment call wrote, as append_frames derives them from
    the call's results: the frame's payload bytes in the source blob."""
    pc, po, _ = push
    buf = seg["frame_buf"].astype(np.int64)
    flen = seg["len_out"].astype(np.int64) - TCP_HEADERS
    before = np.cumsum(flen) - flen
    within = before - before[seg["first_frame"].astype(np.int64)[buf]] if len(buf) else before
    return np.asarray(pc, np.int64)[buf], (np.asarray(po, np.int64)[buf] + within) & M32, flen


def carry_refs(rx: np.ndarray, base: int) -> None:
    """INTEGRATION.md's carry protocol on A's receive table: store entries that name a frame of the batch just
    processed become handles."""
    k = np.arange(SN.OOO_MAX)[None, :] < rx["ooo_count"][:, None]
    ref = rx["ooo"]["ref"]
    mine = k & (ref < HANDLE)
    ref[mine] = HANDLE | ((base + ref[mine]) & 0x7FFFFFFF)


class Peer:
    """B."""

    def __init__(self, tr: Trace, rng):
        c = tr.case
        self.tr, self.rng, self.L = tr, rng, c.stream
        self.got = [np.zeros(c.stream, np.uint8) for _ in range(c.nconns)]
        self.have = [np.zeros(c.stream, bool) for _ in range(c.nconns)]
        self.rcv = np.zeros(c.nconns, np.int64)      # stream bytes in order (+ 1 once the FIN is)
        self.fin = np.zeros(c.nconns, bool)
        self.sent = np.zeros(c.nconns, np.int64)     # B's own stream position

    def receive(self, c: int, frame: bytes) -> None:
        tot = int.from_bytes(frame[16:18], "big")
        seq, flags = int.from_bytes(frame[38:42], "big"), frame[47]
        pay = np.frombuffer(frame[TCP_HEADERS:14 + tot], np.uint8)
        p = (seq - int(self.tr.isn[c])) & M32
        assert p + len(pay) <= self.L, "A sent bytes beyond its stream"
        self.got[c][p:p + len(pay)] = pay
        self.have[c][p:p + len(pay)] = True
        if flags & FIN:
            assert p + len(pay) == self.L, "FIN before the stream's end"
            self.fin[c] = True
        r = int(min(self.rcv[c], self.L))
        while r < self.L:
            gap = np.flatnonzero(~self.have[c][r:r + 2048])
            if len(gap):
                r += int(gap[0])
                break
            r = min(r + 2048, self.L)
        self.rcv[c] = r + (1 if r == self.L and self.fin[c] else 0)

    def ack(self, c: int, mss: int) -> tuple:
        """(frame, seq, ack, raw window) of the ACK B sends now."""
        tr, case = self.tr, self.tr.case
        ws = int(tr.ak0["snd_wscale"][c])
        raw = int(quantize(mss * int(self.rng.integers(case.flight[0], case.flight[1] + 1)), mss, ws))
        k = int(self.rng.integers(0, 9)) if case.peer_data else 0
        pay = SN.stream_bytes(PEER_STREAM + c, np.arange(self.sent[c], self.sent[c] + k)).tobytes()
        seq, ack = (int(tr.irs[c]) + int(self.sent[c])) & M32, (int(tr.isn[c]) + int(self.rcv[c])) & M32
        self.sent[c] += k
        return self.frame(c, seq, ack, raw, pay), seq, ack, raw

    def frame(self, c, seq, ack, raw, pay=b"") -> bytes:
        fl = self.tr.flows[c]
        return F.tcp_frame(pay, src=int(fl["remote_ip"]), dst=int(fl["local_ip"]), sport=int(fl["remote_port"]),
                           dport=int(fl["local_port"]),
                           tcp_kw=dict(seq=seq, ack=ack, flags=ACK | (PSH if pay else 0), window=raw))


def resend(tr: Trace, tx: np.ndarray, c: int, off: int, ln: int) -> bytes:
    """retransmit() (sender.rs:375-403): the front entry as it stands, at SND.UNA, PSH on data, FIN for the marker."""
    fl, T = tr.flows[c], tx[c]
    return F.tcp_frame(tr.src[off:off + ln].tobytes(), src=int(fl["local_ip"]), dst=int(fl["remote_ip"]),
                       sport=int(fl["local_port"]), dport=int(fl["remote_port"]),
                       tcp_kw=dict(seq=int(T["snd_una"]), ack=int(T["rcv_nxt"]), flags=ACK | (PSH if ln else FIN),
                                   window=int(T["rcv_wnd_hdr"])))


def halves(frame: bytes, k: int) -> list:
    """A data frame cut in two after k payload bytes: both with the headers tests/frames.py writes."""
    tot = int.from_bytes(frame[16:18], "big")
    pay, seq = frame[TCP_HEADERS:14 + tot], int.from_bytes(frame[38:42], "big")
    kw = dict(src=int.from_bytes(frame[26:30], "little"), dst=int.from_bytes(frame[30:34], "little"),
              sport=int.from_bytes(frame[34:36], "big"), dport=int.from_bytes(frame[36:38], "big"))
    tk = dict(ack=int.from_bytes(frame[42:46], "big"), window=int.from_bytes(frame[48:50], "big"))
    return [F.tcp_frame(pay[:k], tcp_kw=dict(seq=seq, flags=ACK, **tk), **kw),
            F.tcp_frame(pay[k:], tcp_kw=dict(seq=(seq + k) & M32, flags=frame[47], **tk), **kw)]


def deadline(ak, c) -> int:
    return int(ak["rtx_base_ns"][c]) + int(round(float(ak["rto"][c]) * SEC))


@functools.lru_cache(maxsize=None)
def trace(name: str) -> Trace:
    """The case's closed loop, run once on the host and recorded round by round. A round trip takes 0.2 .. 80 ms of
    the virtual clock, one in ten 1 .. 6 s (samples beyond 2^32 ns, timers that fire with the ACKs on their way)."""
    from oracle import oracle as O
    from oracle.oracle import OraclePeer

    case = CASES[name]
    tr = initial(case)
    nc, L, rows, cap = case.nconns, case.stream, len(tr.flows), tr.cap
    rng = np.random.default_rng(case.seed + 1000)
    rx, tx, ak = tr.rx0.copy(), tr.tx0.copy(), tr.ak0.copy()
    pool = {"off": np.zeros(rows * cap, np.uint32), "len": np.zeros(rows * cap, np.uint32),
            "tx_time": np.zeros(rows * cap, np.uint64)}
    a_side = OraclePeer(synth.ipv4(synth.BOB_IPV4))
    a_side.set_flows(tr.flows)
    peer = Peer(tr, rng)
    out_blob = np.zeros(tr.max_frames * tr.stride, np.uint8)
    pushed, fin_out = np.zeros(nc, np.int64), np.zeros(nc, bool)
    fast = np.zeros(nc, bool)            # the last call reported three duplicate ACKs
    fin_dropped = np.zeros(nc, bool)
    now, frames_seen = SEC, 0
    st = tr.stats = dict(timer_rtx=0, fast_rtx=0, fin_rtx=0, unsent=0, jumps=0, splits=0)
    final = ((tr.isn[:nc].astype(np.int64) + L + 1) & M32).astype(np.uint32)
    for rnd in range(4 * CALL_CAP):
        if (tx["snd_una"][:nc] == final).all():
            tr.done = True
            break
        lossy = rnd < case.lossy
        mss = mss_of(case, rnd, rows)
        tx["mss"] = mss
        # ---- the host's timers and retransmissions -----------------------------------------------------------------
        data, dconn = [], []             # this round's frames toward B
        rtx, rto_c, rto_v, base_c, keys = [], [], [], [], []

        def retransmit(c):
            e = int(ak["q_first"][c])
            off, ln = int(pool["off"][e]), int(pool["len"][e])
            data.append(resend(tr, tx, c, off, ln)), dconn.append(c)
            pool["tx_time"][e] = NONE
            rtx.append(c), keys.append((c, off + ln, ln == 0))
            st["fin_rtx"] += ln == 0

        def timers():
            for c in range(nc):
                if ak["rtx_armed"][c] and ak["q_count"][c] and deadline(ak, c) <= now:
                    retransmit(c)
                    ak["rto"][c] = min(2.0 * float(ak["rto"][c]), 60.0)
                    ak["rtx_base_ns"][c] = now
                    rto_c.append(c), rto_v.append(float(ak["rto"][c])), base_c.append(c)
                    st["timer_rtx"] += 1
                    fast[c] = False

        timers()
        for c in np.nonzero(fast)[0]:
            if ak["q_count"][c]:
                retransmit(int(c))
                st["fast_rtx"] += 1
        fast[:] = False
        # ---- what the window lets out ------------------------------------------------------------------------------
        pc, po, pl = [], [], []
        for c in range(nc):
            if pushed[c] < L:
                pc.append(c), po.append(c * L + pushed[c]), pl.append(L - pushed[c])
            if not fin_out[c]:
                pc.append(c), po.append(c * L + L), pl.append(0)  # the end-of-send marker
        seg = None
        if pc:
            seg = M.segment(tr.src, pc, po, pl, tx, tr.links, out_blob, slot_stride=tr.stride, frame_lead=0,
                            max_frames=tr.max_frames)
            n = len(seg["off_out"])
            assert (seg["status"] != M.NO_ROOM).all() and (seg["status"] != M.E_CONN).all(), seg["status"]
            if n == 0:
                seg = None
        if seg is None and not data:  # nothing to send: wait for the earliest timer
            armed = [deadline(ak, c) for c in range(nc) if ak["rtx_armed"][c] and ak["q_count"][c]]
            assert armed, "the transfer is stuck with no timer armed"
            now = max(now, min(armed))
            st["jumps"] += 1
            timers()
            assert data
        r = Round(mss=mss.copy(), rtx=np.array(rtx, np.int64), rto_set=(np.array(rto_c, np.int64), np.array(rto_v)),
                  base_set=(np.array(base_c, np.int64), now), t_send=now, rtx_keys=keys, lossy=lossy)
        if seg is not None:
            n = len(seg["off_out"])
            tx = seg["tx_conns"]
            for b, c in enumerate(pc):
                if pl[b]:
                    pushed[c] += int(seg["sent"][b])
                elif seg["status"][b] == M.SENT:
                    fin_out[c] = True
            r.push = (np.array(pc, np.uint32), np.array(po, np.uint32), np.array(pl, np.uint32))
            r.seg = {k: seg[k] for k in ("off_out", "len_out", "frame_buf", "first_frame", "sent", "status")}
            r.seg["out"], r.seg["tx_conns"] = seg["out"][:n * tr.stride].copy(), tx.copy()
            r.sends = sent_entries(r.push, seg)
            append_frames(ak, pool, cap, *r.sends, now)
            for f in range(n):
                o = int(seg["off_out"][f])
                data.append(seg["out"][o:o + int(seg["len_out"][f])].tobytes()), dconn.append(int(r.sends[0][f]))
        tr.rounds.append(r)
        # ---- the network toward B, B, the network back ------------------------------------------------------------
        if lossy:  # some data frames arrive as two
            d2, c2 = [], []
            for f, c in zip(data, dconn):
                ln = int.from_bytes(f[16:18], "big") - 40
                if ln >= 2 and rng.random() < case.split:
                    d2 += halves(f, int(rng.integers(1, ln)))
                    c2 += [c, c]
                    st["splits"] += 1
                else:
                    d2.append(f), c2.append(c)
            data, dconn = d2, c2
        dconn = np.array(dconn, np.int64)
        order = np.argsort(dconn, kind="stable")
        rank = np.empty(len(dconn), np.int64)
        rank[order] = np.arange(len(dconn)) - np.searchsorted(dconn[order], dconn[order])
        idx = SN.network(dconn, rank, lossy, SimpleNamespace(loss=case.loss, dup=case.dup, span=case.span), rng)
        acks, aconn, aseq, aack, awin = [], [], [], [], []
        for i in idx:
            c, f = int(dconn[i]), data[i]
            if case.fin_lost and f[47] & FIN and not fin_dropped[c]:
                fin_dropped[c] = True
                continue
            peer.receive(c, f)
            fr, s, a, w = peer.ack(c, int(mss[c]))
            acks.append(fr), aconn.append(c), aseq.append(s), aack.append(a), awin.append(w)
            if lossy and rng.random() < 0.03:  # an ACK for bytes A has not sent
                a = (int(tx["snd_nxt"][c]) + 1 + int(rng.integers(0, 50))) & M32
                acks.append(peer.frame(c, s, a, w)), aconn.append(c), aseq.append(s), aack.append(a), awin.append(w)
                st["unsent"] += 1
        aconn = np.array(aconn, np.int64)
        order = np.argsort(aconn, kind="stable")
        rank = np.empty(len(aconn), np.int64)
        rank[order] = np.arange(len(aconn)) - np.searchsorted(aconn[order], aconn[order])
        idx = SN.network(aconn, rank, lossy, SimpleNamespace(loss=case.loss, dup=case.dup, span=case.ack_span), rng)
        # ---- A: the ACKs ------------------------------------------------------------------------------------------
        rtt = rng.integers(2 * 10**5, 8 * 10**7) if rng.random() >= 0.1 else rng.integers(SEC, 6 * SEC)
        now += int(rtt)
        if len(idx):
            blob, off, lens = F.pack([acks[i] for i in idx])
            a = SimpleNamespace(blob=blob, off=off, lens=lens, conn=aconn[idx], seq=np.array(aseq, np.uint32)[idx],
                                ackn=np.array(aack, np.uint32)[idx], win=np.array(awin, np.uint32)[idx], now=now,
                                base=frames_seen)
            rx["send_next"] = tx["snd_nxt"]  # sync_send_next
            a.start = dict(rx=rx.copy(), tx=tx.copy(), ak=ak.copy(), pool={k: v.copy() for k, v in pool.items()})
            h = a_side.process(blob, off, lens)
            a.rx_out = O.tcp_process(rx, h)
            a.h = {k: h[k] for k in ("flow_id", "tcp_seq", "tcp_ack", "tcp_win")}
            a.exp = R.ack_process(h["flow_id"], a.rx_out["action"], h["tcp_seq"], h["tcp_ack"], h["tcp_win"], rx, tx,
                                  ak, pool, now)
            a.rx_after = rx.copy()  # before the handle rewrite
            tx, ak, pool = a.exp["tx_conns"].copy(), a.exp["ack_conns"].copy(), {k: v.copy() for k, v in
                                                                                 a.exp["pool"].items()}
            carry_refs(rx, frames_seen)
            frames_seen += len(idx)
            fast[:] = a.exp["dup_acks"][:nc] >= 3
            r.ack = a
        if case.peer_data:
            peer.sent[:] = (rx["receive_next"][:nc] - tr.irs[:nc]).astype(np.uint32)
        now += int(rng.integers(10**5, 5 * 10**6))
    tr.peer_got, tr.peer_fin = peer.got, peer.fin
    tr.final = dict(rx=rx, tx=tx, ak=ak, pool=pool)
    return tr


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
def clamp_rto(srtt: float, rttvar: float) -> float:
    return min(max(srtt + max(0.001, 4.0 * rttvar), 0.1), 60.0)


def same_row(a, b, c) -> bool:
    return a[c].tobytes() == b[c].tobytes()


class AckChecker:
    def __init__(self, tr: Trace):
        self.tr, self.nc, self.L = tr, tr.case.nconns, tr.case.stream
        self.isn = tr.isn.astype(np.int64)
        self.una = tr.tx0["snd_una"].copy()
        self.acked_total = np.zeros(len(tr.tx0), np.int64)
        self.first = {}                      # (conn, end offset, is marker) -> (off, time) of the first send
        self.resent = set()
        self.ends = [{self.L + 1} for _ in range(self.nc)]  # stream offsets at which a frame A cut ends
        self.lo = np.full(len(tr.tx0), np.inf)
        self.hi = np.full(len(tr.tx0), -np.inf)
        self.calls = 0
        self.seen = dict(inside=0, trimmed=0, trimmed_again=0, old=0, new=0, dup=0, samples=0)

    def host(self, r: Round) -> None:
        """The host's log of a round: what it retransmitted and what it sent."""
        self.resent.update(r.rtx_keys)
        if r.sends is not None:
            for c, off, ln in zip(*r.sends):
                self.first[(int(c), int(off + ln), bool(ln == 0))] = (int(off), r.t_send)
                self.ends[int(c)].add(int(off + ln) - int(c) * self.L)

    def feed(self, a, action, out: dict, tx, ak, pool) -> None:
        """One ACK call: a = the round's ack record (the batch as the harness built it, now, the state the call
        started from); action = dk_tcp_rx_process's; out = the ACK pass's outputs; tx, ak, pool after it."""
        ctx = f"call {self.calls}"
        self.calls += 1
        s_tx, s_ak, s_pool = a.start["tx"], a.start["ak"], a.start["pool"]
        proc = np.isin(action, R.PROCESSED)
        acked = out["acked"]
        assert not acked[~proc].any(), f"{ctx} T3: acked set on a frame that was not ACK-processed"
        changed = np.zeros(len(pool["off"]), bool)
        for k in pool:
            changed |= pool[k] != s_pool[k]
        for c in range(len(tx)):
            w = f"{ctx} connection {c}"
            if c >= self.nc:  # the listener's row
                assert out["status"][c] == R.E_STATE and same_row(tx, s_tx, c) and same_row(ak, s_ak, c), \
                    f"{w}: not left alone"
                continue
            assert out["status"][c] == R.OK, f"{w}: status {out['status'][c]}"
            i = np.nonzero(proc & (a.conn == c))[0]
            una0, nxt = int(s_tx["snd_una"][c]), int(s_tx["snd_nxt"][c])
            una1, ws = int(tx["snd_una"][c]), int(s_ak["snd_wscale"][c])
            flight = (nxt - una0) & M32
            # T1
            assert una0 == int(self.una[c]) and int(tx["snd_nxt"][c]) == nxt, f"{w} T1: SND.NXT or SND.UNA rewritten"
            offs = (a.ackn[i].astype(np.int64) - una0) & M32
            ok = offs[(offs > 0) & (offs <= flight)]
            adv = int(ok.max()) if len(ok) else 0
            got = (una1 - una0) & M32
            assert got < 1 << 31, f"{w} T1: SND.UNA moved backwards"
            assert got == adv, f"{w} T1: SND.UNA moved by {got}, the highest ack in (SND.UNA, SND.NXT] is {adv} ahead"
            self.una[c] = una1
            wl = (int(ak["wl1"][c]), int(ak["wl2"][c]), int(tx["snd_wnd"][c]))
            wl0 = (int(s_ak["wl1"][c]), int(s_ak["wl2"][c]), int(s_tx["snd_wnd"][c]))
            if wl[:2] == wl0[:2]:
                assert wl[2] == wl0[2], f"{w} T1: the window changed without a window update"
            else:
                assert ((wl[0] - wl0[0]) & M32) < 1 << 31, f"{w} T1: wl1 moved backwards"
                j = i[a.ackn[i] == wl[1]]
                assert len(j) and 0 < ((wl[1] - una0) & M32) <= flight, f"{w} T1: wl2 is no new ACK of this call"
                j = int(j[0])  # only the first frame with this ack number can have been a new ACK
                assert (int(a.seq[j]), (int(a.win[j]) << ws) & M32) == (wl[0], wl[2]), \
                    f"{w} T1: the window update is not that of the new ACK {wl[1]}"
            # T3
            new = (acked[i] > 0) & (acked[i] < 1 << 31)
            assert int(out["bytes_acked"][c]) == got == int(acked[i][new].astype(np.int64).sum()), \
                f"{w} T3: bytes_acked {out['bytes_acked'][c]}, SND.UNA moved {got}, new ACKs sum {acked[i][new].sum()}"
            counts = (int(out["new_acks"][c]), int(out["dup_acks"][c]))
            assert counts == (int(new.sum()), int((acked[i] == 0).sum())), \
                f"{w} T3: new_acks / dup_acks {counts} do not count acked[]"
            assert int(out["new_acks"][c]) + int(out["dup_acks"][c]) <= len(i), f"{w} T3: more ACKs than frames"
            self.acked_total[c] += got
            self.seen["new"] += int(new.sum())
            self.seen["dup"] += int(out["dup_acks"][c])
            self.seen["old"] += int((acked[i] >= 1 << 31).sum())
            self.seen["inside"] += sum(int(p) not in self.ends[c]
                                       for p in (a.ackn[i][new].astype(np.int64) - self.isn[c]) & M32)
            # T2
            qf0, qc0, qf1, qc1 = (int(t[k][c]) for t in (s_ak, ak) for k in ("q_first", "q_count"))
            assert qf1 >= qf0 and qf1 + qc1 == qf0 + qc0, f"{w} T2: queue [{qf1}, +{qc1}) from [{qf0}, +{qc0})"
            off, ln = (pool[k][qf1:qf1 + qc1].astype(np.int64) for k in ("off", "len"))
            tt = pool["tx_time"][qf1:qf1 + qc1]
            pos = (una1 - int(self.isn[c])) & M32
            marker = int(qc1 > 0 and ln[-1] == 0)
            assert (ln[:qc1 - marker] > 0).all(), f"{w} T2: an empty entry or a marker inside the queue"
            assert int(ln.sum()) + marker == (nxt - una1) & M32, \
                f"{w} T2: the queue holds {int(ln.sum())} + {marker}, in flight {(nxt - una1) & M32}"
            if qc1:
                assert off[0] == c * self.L + pos, f"{w} T2: the front is at {off[0]}, SND.UNA at {c * self.L + pos}"
                assert (off[:-1] + ln[:-1] == off[1:]).all(), f"{w} T2: the live entries are not contiguous"
            ch = changed[c * self.tr.cap:(c + 1) * self.tr.cap].copy()
            trimmed = bool(qc1) and bool(ch[qf1 - c * self.tr.cap])
            if qc1:
                ch[qf1 - c * self.tr.cap] = False
            assert not ch.any(), f"{w} T2: pool entries {np.nonzero(ch)[0][:4] + c * self.tr.cap} changed"
            # T4
            for e in range(qc1):
                key = (c, int(off[e] + ln[e]), bool(ln[e] == 0))
                assert key in self.first, f"{w} T4: entry {qf1 + e} was never sent"
                off1, t1 = self.first[key]
                want = NONE if key in self.resent or off1 != off[e] else t1
                assert int(tt[e]) == want, f"{w} T4: entry {qf1 + e} holds {int(tt[e])}, the log says {want}"
            touched = s_pool["tx_time"][qf0:qf1 + trimmed]
            timed = touched[touched != NONE]
            assert int(out["samples"][c]) == len(timed), \
                f"{w} T4: {out['samples'][c]} samples, {len(timed)} touched entries had a time"
            self.seen["trimmed"] += trimmed
            if qf1 > qf0 or trimmed:
                o0 = s_pool["off"][qf0:qf1 + trimmed].astype(np.int64)
                e0 = o0 + s_pool["len"][qf0:qf1 + trimmed]
                mk = s_pool["len"][qf0:qf1 + trimmed] == 0
                self.seen["trimmed_again"] += sum(self.first[(c, int(e), bool(m))][0] != int(o)
                                                  for o, e, m in zip(o0, e0, mk))
            self.seen["samples"] += len(timed)
            # T5
            rto = float(ak["rto"][c])
            assert 0.1 <= rto <= 60.0, f"{w} T5: rto {rto}"
            if int(out["new_acks"][c]) == 0:
                assert same_row(tx, s_tx, c) and same_row(ak, s_ak, c) and not trimmed, \
                    f"{w} T5: changed without a new ACK"
                continue
            front = int(tt[0]) if qc1 else 0
            want = (int(qc1 != 0), (front if front != NONE else a.now) if qc1 else 0)
            assert (int(ak["rtx_armed"][c]), int(ak["rtx_base_ns"][c])) == want, \
                f"{w} T5: timer {ak['rtx_armed'][c]} at {ak['rtx_base_ns'][c]}, the queue says {want}"
            est = [ak[k][c].tobytes() for k in ("srtt", "rttvar", "rto", "received_sample")]
            if not len(timed):
                assert est == [s_ak[k][c].tobytes() for k in ("srtt", "rttvar", "rto", "received_sample")], \
                    f"{w} T5: the RTO state changed without a sample"
                continue
            d = np.where(timed <= np.uint64(a.now), np.uint64(a.now) - timed, 0).astype(np.float64) / 1e9
            self.lo[c], self.hi[c] = min(self.lo[c], d.min()), max(self.hi[c], d.max())
            srtt = float(ak["srtt"][c])
            assert ak["received_sample"][c] == 1 and rto == clamp_rto(srtt, float(ak["rttvar"][c])), \
                f"{w} T5: rto {rto} is not that of srtt {srtt} and rttvar {ak['rttvar'][c]}"
            assert self.lo[c] * (1 - 1e-12) <= srtt <= self.hi[c] * (1 + 1e-12), \
                f"{w} T5: srtt {srtt} outside the samples [{self.lo[c]}, {self.hi[c]}]"

    def finish(self, tx, ak, peer_got, peer_fin, cap: int = CALL_CAP) -> None:
        """T6."""
        assert self.calls <= cap, f"T6: {self.calls} calls, the cap is {cap}"
        nc = self.nc
        final = ((self.isn[:nc] + self.L + 1) & M32).astype(np.uint32)
        assert (tx["snd_una"][:nc] == final).all() and (tx["snd_nxt"][:nc] == final).all(), \
            f"T6: SND.UNA {tx['snd_una'][:nc]} SND.NXT {tx['snd_nxt'][:nc]}, the streams end at {final}"
        assert (self.acked_total[:nc] == self.L + 1).all(), f"T3: bytes_acked sums to {self.acked_total[:nc]}"
        assert not ak["q_count"][:nc].any() and not ak["rtx_armed"][:nc].any(), "T6: a queue or a timer is left"
        for c in range(nc):
            want = SN.stream_bytes(c, np.arange(self.L))
            assert peer_fin[c] and np.array_equal(peer_got[c], want), f"T6: B did not get connection {c}'s stream"


def check_trace(tr: Trace, outputs=None) -> AckChecker:
    """AckChecker over a whole trace: the recorded results, or `outputs(k, round) -> (action, out, tx, ak, pool)`."""
    chk = AckChecker(tr)
    k = 0
    for r in tr.rounds:
        chk.host(r)
        if r.ack is None:
            continue
        e = r.ack.exp
        got = (r.ack.rx_out["action"], e, e["tx_conns"], e["ack_conns"], e["pool"]) if outputs is None else \
            outputs(k, r)
        chk.feed(r.ack, *got)
        k += 1
    return chk
