"""TEST INFRASTRUCTURE ONLY: batches for the dk_tcp_ack_process tests. Every connection gets a script: its send side
(SND.UNA / SND.NXT, the window-update pair, an unacknowledged queue that covers the flight) and the segments its peer
sends in arrival order (data, pure ACKs, out-of-order data, retransmissions, strays beyond the window, segments without
the ACK bit or acknowledging unsent data, a FIN or an RST mid-stream), whose ack numbers follow one of the ACK streams
below. The scripts are merged into one batch in random order (each connection's own order kept) with UDP frames
between, and built into frames with demikernel_amd.synth, so the actions the ACK pass filters on are the engine's own.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_ack import ack_conn_table
from demikernel_amd.tcp_tx import tx_conn_table

M32 = 0xFFFFFFFF
NONE = N.DK_TCP_TX_TIME_NONE
NOW = 50 * 10**9
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
ACK_STREAMS = ("rising", "rising_dups", "reordered", "all_una", "all_nxt")
SEG_COUNTS = (0, 1, 63, 64, 65, 129)
QUEUE_COUNTS = (0, 1, 63, 64, 65, 200)


@dataclass
class Script:
    m: int                      # segments
    stream: str = "rising"      # ACK stream
    qn: int = 8                 # queue entries (without the marker)
    marker: bool = False        # an end-of-send marker closes the queue
    end: str = "whole"          # where the last ACK lands: "whole" queue, entry "boundary", "inside" an entry
    mixed: bool = True          # drops and out-of-order segments between the processed ones
    close: str = ""             # "fin" / "rst" in the middle of the stream
    una: int | None = None      # SND.UNA (random unless given)
    rn: int | None = None       # the peer's stream position = our RCV.NXT (random unless given)
    wl1_off: int = -5           # wl1 = rn + wl1_off
    wl2_off: int = -3           # wl2 = una + wl2_off
    wscale: int = 0
    extra_flight: int = 0       # sequence space in flight that no queue entry covers (a dry queue)
    bad: dict = field(default_factory=dict)  # "tx__state" etc.: a field overwritten in the tables
    tx_times: list | None = None  # the queue entries' transmit times, given (qn = their number; no marker's)
    rto: tuple | None = None    # the RTO state the call starts from: (srtt, rttvar, rto, received_sample)

    def __post_init__(self):
        if self.tx_times is not None:
            self.qn = len(self.tx_times)


def offsets(rng, s: Script, lens: np.ndarray) -> np.ndarray:
    """The m ack numbers as offsets from SND.UNA."""
    flight = int(lens.sum()) + int(s.marker) + s.extra_flight
    bounds = np.concatenate([[0], np.cumsum(lens)])
    if s.m == 0:
        return np.zeros(0, np.int64)
    if s.stream == "all_una":
        return np.zeros(s.m, np.int64)
    if s.stream == "all_nxt":
        return np.full(s.m, flight, np.int64)
    top = flight
    if s.end == "boundary" and len(lens) > 1:
        top = int(bounds[len(lens) // 2])
    elif s.end == "inside" and len(lens):
        k = len(lens) // 2
        top = int(bounds[k]) + max(int(lens[k]) // 2, 1) if lens[k] > 1 else int(bounds[k + 1])
    pick = np.where(rng.random(s.m) < 0.5, bounds[rng.integers(0, len(bounds), s.m)], rng.integers(0, top + 1, s.m))
    o = np.sort(np.minimum(pick, top))
    o[-1] = top
    if s.stream == "rising_dups":
        for i in np.nonzero(rng.random(s.m) < 0.2)[0]:
            if i:
                o[i] = o[i - 1] if rng.random() < 0.5 else o[rng.integers(0, i)]
    return o.astype(np.int64)


def build(scripts: list[Script], seed: int = 1, udp_every: int = 9, now: int = NOW):
    """-> dict: flows, blob/off/lens (the frames), rx/tx/ak tables, pool arrays, now (the call's clock, below NONE)."""
    assert 3 * 10**9 <= now < NONE
    rng = np.random.default_rng(seed)
    nc = len(scripts)
    flows = np.concatenate([synth.make_flows(nc, seed=seed), synth.make_flows(2, kind="udp")])
    nrows = nc + 1  # the Passive listener's row follows the connections (DK_TCP_NONE)
    rx, tx, ak = conn_table(nrows), tx_conn_table(nrows), ack_conn_table(nrows)
    rx["state"][nc:] = N.DK_TCP_NONE
    tx["state"][nc:] = N.DK_TCP_NONE
    pool = {"off": [], "len": [], "tx_time": []}
    per = []
    for c, s in enumerate(scripts):
        una = int(rng.integers(0, 1 << 32)) if s.una is None else s.una & M32
        rn = int(rng.integers(0, 1 << 32)) if s.rn is None else s.rn & M32
        lens = rng.integers(1, 1461, s.qn)
        txt = np.uint64(now) - rng.integers(10**5, 3 * 10**9, s.qn).astype(np.uint64)
        r = rng.random(s.qn)
        txt[r < 0.3] = NONE  # retransmitted entries, interleaved
        # a transmit time ahead of now: the difference saturates at 0
        txt[(r >= 0.3) & (r < 0.4)] = min(now + 12345, NONE - 1)
        if s.tx_times is not None:
            txt = np.array(s.tx_times, np.uint64)
        qlens, qtx = list(lens), list(txt)
        if s.marker:
            qlens.append(0), qtx.append(now - 777)
        # some slack in front of every queue, so q_first is not a multiple of anything
        pad = int(rng.integers(0, 3))
        pool["off"] += [0] * pad + list(rng.integers(0, 1 << 20, len(qlens)))
        pool["len"] += [7] * pad + qlens
        pool["tx_time"] += [1] * pad + qtx
        ak["q_first"][c], ak["q_count"][c] = len(pool["off"]) - len(qlens), len(qlens)
        flight = int(lens.sum()) + int(s.marker) + s.extra_flight
        nxt = (una + flight) & M32
        tx["snd_una"][c], tx["snd_nxt"][c], tx["snd_wnd"][c] = una, nxt, 4321
        rx["receive_next"][c] = rx["reader_next"][c] = rn
        rx["send_next"][c] = nxt
        ak["wl1"][c], ak["wl2"][c], ak["snd_wscale"][c] = (rn + s.wl1_off) & M32, (una + s.wl2_off) & M32, s.wscale
        if s.rto is not None:
            ak["srtt"][c], ak["rttvar"][c], ak["rto"][c], ak["received_sample"][c] = s.rto
        # the segments
        o = offsets(rng, s, lens)
        if s.stream == "reordered":  # swap neighbours' acks; the seqs below get their own disorder from "stored"
            for i in range(0, s.m - 1, 2):
                if rng.random() < 0.5:
                    o[i], o[i + 1] = o[i + 1], o[i]
        pos, segs, held = 0, [], None  # pos: the peer's stream offset; held: the hole before a stored piece
        close_at = s.m // 2 if s.close else -1
        for k in range(s.m):
            kind = "data"
            if s.mixed or s.stream == "reordered":
                kind = rng.choice(["data", "ack", "stored", "dup", "oow", "noack", "unsent"],
                                  p=[0.4, 0.25, 0.1, 0.08, 0.07, 0.05, 0.05])
            ackn, flags, seq, ln = (una + int(o[k])) & M32, PSH | ACK, pos, int(rng.integers(1, 9))
            if k == close_at:
                kind, ln = "close", 0
                flags = (FIN | ACK) if s.close == "fin" else (RST | ACK)
            if kind == "ack":
                flags, ln = ACK, 0
            elif kind == "stored":  # ln bytes, ln bytes ahead of the stream; the next data segment fills the hole
                if held is not None or pos > 60000:
                    kind = "data"
                else:
                    held, seq = ln, pos + ln
            elif kind == "dup":
                seq, ln = pos - 600, 100
            elif kind == "oow":
                seq = pos + 70000
            elif kind == "noack":
                flags = PSH
            elif kind == "unsent":
                ackn = (nxt + 1 + int(rng.integers(0, 1000))) & M32
            if kind == "data":
                if held is not None:
                    ln, pos, held = held, pos + 2 * held, None
                else:
                    pos += ln
            segs.append((c, (rn + seq) & M32, ackn, flags, ln, int(rng.integers(0, 65536))))
        for k, v in s.bad.items():
            t, f = k.split("__")
            {"tx": tx, "rx": rx, "ak": ak}[t][f][c] = v
        per.append(segs)
    # merge: a random interleave that keeps each connection's order, UDP frames between
    order = np.repeat(np.arange(nc), [len(p) for p in per])
    rng.shuffle(order)
    nxt_i = [0] * nc
    rows = []
    for j, c in enumerate(order):
        rows.append(per[c][nxt_i[c]])
        nxt_i[c] += 1
        if udp_every and j % udp_every == udp_every - 1:
            rows.append(None)
    n = len(rows)
    tr = synth.traffic(n, 40, flows, seed=seed)
    for i, row in enumerate(rows):
        if row is None:
            f = nc + 1 + (i & 1)
            tr.proto[i], tr.flow[i], tr.ip_len[i] = 17, f, 28 + 5
            tr.src_ip[i], tr.sport[i], tr.dport[i] = synth.ipv4("10.1.2.3"), 999, flows["local_port"][f]
            continue
        c, seq, ackn, flags, ln, win = row
        tr.proto[i], tr.flow[i], tr.ip_len[i] = 6, c, 40 + ln
        tr.src_ip[i], tr.sport[i], tr.dport[i] = flows["remote_ip"][c], flows["remote_port"][c], flows["local_port"][c]
        tr.seq[i], tr.ack[i], tr.flags[i], tr.window[i] = seq, ackn, flags, win
    tr.frame_len = np.maximum(tr.ip_len.astype(np.int64) + 14, synth.ETH_MIN_FRAME).astype(np.uint16)
    blob, off, lens = synth.build_numpy(tr, seed=seed) if n else (np.zeros(1, np.uint8), np.zeros(0, np.uint32),
                                                                   np.zeros(0, np.uint16))
    pool = {"off": np.array(pool["off"], np.uint32), "len": np.array(pool["len"], np.uint32),
            "tx_time": np.array(pool["tx_time"], np.uint64)}
    return {"flows": flows, "blob": blob, "off": off, "lens": lens, "rx": rx, "tx": tx, "ak": ak, "pool": pool,
            "now": now, "n": n, "nconns": nrows}


# RTT samples d = now - tx_time in nanoseconds, in queue order: around one second (where Duration::as_secs_f64 splits
# whole seconds from nanoseconds), around 2^32 ns (4.29 s: what 32-bit arithmetic on d loses), around the RTO's upper
# clamp of 60 s, above 2^53 (the whole seconds no longer fit f64 once multiplied out), at 2^63 (the sign bit of an
# int64 difference) and the largest there is.
EXTREME_D = (0, 1, 999999999, 10**9, 10**9 + 1, 2**32 - 1, 2**32, 2**32 + 1, 599 * 10**8, 60 * 10**9, 100 * 10**9,
             2**53 + 1, 2**63, 2**64 - 2)
EXTREME_NOWS = (2**64 - 2, 2**63)
BACKED_OFF = (0.2, 0.01, 8.0, 1)  # an RTO state after samples and one host back-off (rto is not srtt + 4 rttvar)


def extreme_times(now: int, ds=EXTREME_D, ahead: bool = True) -> list:
    """Transmit times that give the samples `ds` (those that fit below `now`) in order, a NONE entry after every
    third and, where `now` leaves room above it, entries with tx_time > now (no sample of theirs is negative: it
    saturates at 0). At now = 2^64 - 2 the only value above now is NONE itself."""
    out = []
    for k, d in enumerate(d for d in ds if d <= now):
        out.append(now - d)
        if k % 3 == 2:
            out.append(NONE)
        if ahead and k % 4 == 1 and now + 1 < NONE:
            out.append((now + 1, NONE - 1)[k // 4 % 2])
    return out


def extremes(now: int):
    """One batch at clock `now`: the RTT / RTO extremes, one connection per line. Every ACK stream is all_nxt or rising
    without drops between, so every entry is popped and the samples taken are exactly the entries with a time."""
    cyc = lambda k: [now - EXTREME_D[(7 * i) % len(EXTREME_D)] for i in range(k)  # noqa: E731
                     if EXTREME_D[(7 * i) % len(EXTREME_D)] <= now]
    scripts = [
        Script(m=9, mixed=False, tx_times=extreme_times(now)),
        # the same list from entry 65 on and 200 more behind: the wave form folds 64 entries a step
        Script(m=12, mixed=False, marker=True, tx_times=cyc(130)[:65] + extreme_times(now) + cyc(400)[:200]),
        Script(m=5, mixed=False, stream="all_nxt", tx_times=[now - d for d in (0, 1, 500, 1000, 999, 1000, 7, 1000)]),
        Script(m=5, mixed=False, tx_times=[now - d for d in (60 * 10**9, 100 * 10**9, 2**53 + 1, 2**63, 60 * 10**9)]),
        Script(m=4, mixed=False, stream="all_nxt", tx_times=[NONE, now - (2**32 - 1), NONE]),
        Script(m=6, mixed=False, rto=BACKED_OFF, tx_times=[NONE] * 5),
        Script(m=6, mixed=False, rto=BACKED_OFF, tx_times=[NONE, now - 3 * 10**8, NONE]),
        # srtt the smallest subnormal: 0.875 * srtt + 0 rounds back to it, a flush to zero would not
        Script(m=6, mixed=False, rto=(5e-324, 1e300, 1.0, 1), tx_times=[now] * 3),
        Script(m=6, mixed=False, rto=(5e-324, 1e300, 1.0, 1), tx_times=[now - d for d in (0, 0, 1, 10**9, 0)]),
    ]
    case = build(scripts, seed=123, now=now)
    case["scripts"] = scripts
    return case


def check_extremes(case: dict, exp: dict) -> None:
    """What the lines of extremes() are there for, asserted on a result (the reference's, which the device's equals
    bit for bit)."""
    a, now = exp["ack_conns"], case["now"]
    nc = len(case["scripts"])
    assert (exp["status"][:nc] == 0).all() and (a["q_count"][:nc] == 0).all(), exp["status"]
    for c, s in enumerate(case["scripts"]):  # the samples taken are known: every entry with a time, and the marker
        assert exp["samples"][c] == sum(t != NONE for t in s.tx_times) + int(s.marker), (c, exp["samples"][c])
    assert a["rto"][2] == 0.1 and 4.0 * a["rttvar"][2] < 0.001
    assert a["rto"][3] == 60.0 and a["srtt"][3] > 60.0
    assert exp["samples"][4] == 1 and a["received_sample"][4] == 1
    assert a["srtt"][4] == 4.0 + 294967295 / 1e9 and a["rttvar"][4] == a["srtt"][4] / 2.0
    before = case["ak"]
    assert exp["new_acks"][5] > 0 and exp["samples"][5] == 0 and a["rto"][5] == 8.0
    for k in ("srtt", "rttvar", "rto"):
        assert a[k][5].tobytes() == before[k][5].tobytes(), k
    assert a["srtt"][6] == 0.875 * 0.2 + 0.125 * 0.3 and a["rttvar"][6] == 0.75 * 0.01 + 0.25 * abs(0.2 - 0.3)
    assert a["rto"][6] == a["srtt"][6] + 4.0 * a["rttvar"][6] != 8.0
    assert a["srtt"][7] == 5e-324 and a["rttvar"][7] == 0.75 * (0.75 * (0.75 * 1e300)) and a["rto"][7] == 60.0
    assert a["rto"][8] == 60.0 and 0.1 < a["srtt"][8] < 0.2
    if now == 2**64 - 2:  # the last sample is 18,446,744,073 s + 0.709551614: an eighth of it is in srtt
        assert a["srtt"][0] > (2**64 - 2) // 10**9 / 8 and a["rto"][0] == 60.0


def host_actions(case: dict) -> dict:
    """The batch through the CPU restatement of the receive chain: what dk_rx_process and dk_tcp_rx_process hand to
    the ACK pass (flow_id, tcp_seq, tcp_ack, tcp_win, action)."""
    from oracle import oracle as O

    peer = O.OraclePeer(synth.ipv4(synth.BOB_IPV4))
    peer.set_flows(case["flows"])
    rx = peer.process(case["blob"], case["off"], case["lens"])
    rx["action"] = O.tcp_process(case["rx"].copy(), rx)["action"]
    return rx


def shapes(nconns: int, big: bool = True) -> list[Script]:
    """`nconns` scripts that cycle through the segment counts, the queue sizes, the ACK streams and the ends; with
    `big`, connection 0 gets 4,097 segments."""
    out = []
    ends = ("whole", "boundary", "inside")
    for c in range(nconns):
        m = SEG_COUNTS[c % len(SEG_COUNTS)]
        qn = QUEUE_COUNTS[(c // 2) % len(QUEUE_COUNTS)]
        out.append(Script(m=m, stream=ACK_STREAMS[(c // 3) % len(ACK_STREAMS)], qn=qn, marker=c % 4 == 1,
                          end=ends[(c // 5) % 3], mixed=c % 3 != 2, close=("fin", "", "", "rst", "", "", "")[c % 7],
                          wscale=c % 15))
    if big and out:
        out[0] = Script(m=4097, stream="rising_dups", qn=200, marker=True, end="whole", mixed=True)
    return out
