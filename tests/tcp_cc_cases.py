"""TEST INFRASTRUCTURE ONLY: batches for the dk_tcp_cc_ack tests, as dk_rx result arrays (uploaded as
tests/test_gpu_tcp.py does). Every connection gets a script of ACKs in arrival order that walks cubic.rs's branches: new
ACKs, four duplicates in a row, a partial and a full acknowledgement, an old ACK, an ACK of unsent data (visited by
congestion control, and the only ACK above `recover` inside one batch), with frames between that must not be visited:
entirely old segments (DUPLICATE), segments without the ACK bit, frames of no connection. The rows start in different
phases (fresh, congestion avoidance on either side of w_max, fast recovery, after a timeout)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import tx_segment_reference as M
from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_ack import ack_conn_table
from demikernel_amd.tcp_ackemit import dack_conn_table
from demikernel_amd.tcp_cc import CUBIC, FAST_CONVERGENCE, IN_RECOVERY, LAST_WAS_RTO, cc_conn_table

M32 = 0xFFFFFFFF
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
NOW = 77 * 10**9 + 123456789
NONE = N.DK_TCP_TX_TIME_NONE
PROGRAM = ("new", "new", "dup", "dup", "dup", "dup", "small", "new", "unsent", "new", "old", "new", "dup", "big", "dup",
           "dup", "dup", "small", "unsent", "new", "old", "dup", "dup", "dup", "dup")  # an old ACK moves prev_ack alone
PHASES = ("fresh", "avoidance", "recovery", "after_rto", "above_w_max")


@dataclass
class Script:
    m: int                      # visited segments
    phase: str = "fresh"
    mss: int = 1460
    rto: float = 0.3
    una: int | None = None
    fillers: bool = True        # unvisited frames between
    fin: bool = False           # the last visited segment is a FIN (what follows it is never processed)
    cubic: bool = True
    bad: dict = field(default_factory=dict)  # "tx__state" etc.: a field overwritten in the tables


def build(scripts: list[Script], seed: int = 1, now: int = NOW) -> dict:
    """-> dict: rx (dk_rx result arrays), table (CONN_DTYPE), tx, ak, cc, dack, pool, n, nconns, now. One more row
    than scripts: the last is DK_TCP_NONE."""
    rng = np.random.default_rng(seed)
    nc = len(scripts)
    nrows = nc + 1
    flows = synth.make_flows(nrows, seed=seed, passive=False)
    snd = rng.integers(0, 1 << 32, nrows, dtype=np.uint64)
    table = conn_table(nrows, send_next=snd, buffer_size=1 << 24)
    tx = M.conns_toward(flows, seed=seed, snd_nxt=snd, local_ip=flows["local_ip"], remote_ip=flows["remote_ip"],
                        ports=flows["local_port"].astype(np.uint32) | flows["remote_port"].astype(np.uint32) << 16)
    table["state"][nc:] = N.DK_TCP_NONE
    tx["state"][nc:] = N.DK_TCP_NONE
    tx["rcv_wscale"] = 10  # the 16 MiB buffer fits the 16-bit header window
    ak = ack_conn_table(nrows)
    cc = cc_conn_table(nrows, mss=1460, now_ns=now)
    dack = dack_conn_table(nrows)
    pool = {"off": np.zeros(nrows, np.uint32), "len": np.zeros(nrows, np.uint32), "tx_time": np.full(nrows, NONE, np.uint64)}
    per = []
    for c, s in enumerate(scripts):
        mss = s.mss
        flight = 300 * max(mss, 1) + 17
        nxt = int(snd[c])
        una = (nxt - flight) & M32 if s.una is None else s.una & M32
        nxt = (una + flight) & M32
        rn = int(rng.integers(0, 1 << 32))
        tx["snd_una"][c], tx["snd_nxt"][c], tx["mss"][c], tx["cwnd"][c] = una, nxt, mss, 0x12345678
        table["send_next"][c], table["receive_next"][c], table["reader_next"][c] = nxt, rn, rn
        ak["rto"][c], ak["wl1"][c], ak["wl2"][c] = s.rto, (rn - 5) & M32, (una - 3) & M32
        ak["q_first"][c], ak["q_count"][c], pool["len"][c] = c, 1, flight  # one entry covers the flight
        row = cc_conn_table(1, mss=max(mss, 1), seq_no=una, now_ns=now - 10**9, cubic=s.cubic)[0]
        if s.phase == "avoidance":      # cwnd below w_max: the region where w_est or the cubic increment decide
            row["cwnd"], row["ssthresh"], row["w_max"], row["ca_start_ns"] = 10 * mss, 2 * mss, 14 * mss, now - 1_500_000_000
        elif s.phase == "above_w_max":  # no fast convergence, a long epoch
            row["flags"] = int(row["flags"]) & (M32 ^ FAST_CONVERGENCE)
            row["cwnd"], row["ssthresh"], row["w_max"], row["ca_start_ns"] = 20 * mss, 5 * mss, 10 * mss, now - 10 * 10**9
        elif s.phase == "recovery":
            row["flags"] |= IN_RECOVERY
            row["cwnd"], row["ssthresh"], row["w_max"] = 8 * mss, 6 * mss, 11 * mss
            row["recover"], row["prev_ack"] = (una + flight // 2) & M32, una
        elif s.phase == "after_rto":
            row["flags"] |= LAST_WAS_RTO
            row["cwnd"], row["ssthresh"], row["w_max"], row["rpif"] = mss, 0, 9 * mss, 2
            row["ca_start_ns"] = now + 5  # ahead of the clock: t saturates at 0
        if not s.cubic:  # the algorithm None: whatever the row holds stays
            row = np.array(tuple(int(v) for v in rng.integers(0, 1 << 31, 13)), N.CC_CONN_DTYPE)
            row["flags"] = int(row["flags"]) & (M32 ^ CUBIC)
        cc[c] = row
        # the script: (kind of segment, ack number)
        cur, pos, segs, k, visited = 0, 0, [], int(rng.integers(0, len(PROGRAM))), 0
        while visited < s.m:
            if s.fillers and rng.random() < 0.3:
                kind = ("dupseg", "noack", "none")[int(rng.integers(0, 3))]
                ackn = (una + int(rng.integers(0, flight))) & M32
                if kind == "dupseg":
                    segs.append(((rn + pos - 600) & M32, ackn, PSH | ACK, 100))
                elif kind == "noack":
                    segs.append(((rn + pos) & M32, ackn, PSH, 0))
                else:
                    segs.append(None)
                continue
            op = PROGRAM[k % len(PROGRAM)]
            k += 1
            if op == "new":
                cur = min(cur + int(rng.integers(1, 2 * max(mss, 1) + 2)), flight)
            elif op == "small":
                cur = min(cur + int(rng.integers(1, max(mss, 2))), flight)
            elif op == "big":
                cur = min(cur + 5 * max(mss, 1) + 3, flight)
            ackn = (una + cur) & M32
            if op == "old":
                ackn = (una + cur - int(rng.integers(1, 5000))) & M32
            elif op == "unsent":
                ackn = (nxt + 1 + int(rng.integers(0, 1000))) & M32
            visited += 1
            shape = int(rng.integers(0, 4))
            if s.fin and visited == s.m:
                segs.append(((rn + pos) & M32, ackn, FIN | ACK, 0))
                segs.append(((rn + pos + 1) & M32, (una + cur) & M32, ACK, 0))  # behind the close: UNPROCESSED
            elif shape == 0:
                segs.append(((rn + pos) & M32, ackn, ACK, 0))            # a pure ACK
            elif shape == 1:
                segs.append(((rn + pos + 5000) & M32, ackn, PSH | ACK, 4))  # out of order: STORED, then STORE_DUP
            else:
                ln = int(rng.integers(1, 9))
                segs.append(((rn + pos) & M32, ackn, PSH | ACK, ln))
                pos += ln if op != "unsent" else 0  # the data of a segment that acknowledges unsent data is dropped
        for key, v in s.bad.items():
            t, f = key.split("__")
            {"tx": tx, "rx": table, "ak": ak}[t][f][c] = v
        per.append(segs)
    order = np.repeat(np.arange(nc), [len(p) for p in per])
    rng.shuffle(order)
    nxt_i = [0] * nc
    rows = []
    for c in order:
        seg = per[c][nxt_i[c]]
        rows.append(None if seg is None else (c,) + seg)
        nxt_i[c] += 1
    n = len(rows)
    rx = {k: np.zeros(n, np.uint32) for k in ("meta", "flow_id", "tcp_seq", "tcp_ack", "payload")}
    for i, row in enumerate(rows):
        if row is None:  # a UDP datagram, a segment of no socket, or one for the row that is no connection
            which = i % 3
            rx["meta"][i] = (N.V["OK_UDP"] | 17 << 8) if which == 0 else (N.V["OK_TCP"] | 6 << 8 | ACK << 16 | 0x50 << 24)
            rx["flow_id"][i] = (0, N.DK_FLOW_NONE, nc)[which]
            rx["tcp_seq"][i], rx["tcp_ack"][i], rx["payload"][i] = i, 7 * i, 54 | 5 << 16
            continue
        c, seq, ackn, flags, ln = row
        rx["meta"][i] = N.V["OK_TCP"] | 6 << 8 | flags << 16 | 0x50 << 24
        rx["flow_id"][i], rx["tcp_seq"][i], rx["tcp_ack"][i], rx["payload"][i] = c, seq, ackn, 54 | ln << 16
    return {"rx": rx, "table": table, "tx": tx, "ak": ak, "cc": cc, "dack": dack, "pool": pool, "n": n,
            "nconns": nrows, "now": now, "flows": flows, "scripts": scripts}


def segs_by_conn(flow_id, action, ack, nconns: int) -> list:
    """Per connection, in arrival order: (frame index, action, ack) of the frames dk_tcp_rx_process gave an action."""
    out = [[] for _ in range(nconns)]
    for i in np.nonzero(np.asarray(action) != N.A["SKIP"])[0]:
        if flow_id[i] < nconns:
            out[int(flow_id[i])].append((int(i), int(action[i]), int(ack[i])))
    return out


def host_actions(case: dict) -> np.ndarray:
    """The batch through the CPU restatement of dk_tcp_rx_process: the actions the device gives."""
    from oracle import oracle as O

    return O.tcp_process(case["table"].copy(), case["rx"])["action"]


VISITS = (1, 7, 8, 63, 64, 65, 200)


def walk_case(seed: int = 11) -> dict:
    """Connections of 1, 7, 8, 63, 64, 65 and 200 visited segments in every starting phase, an MSS of 1 and of 9,000, an
    rto of 0 (rtt = 0: the divisions by zero and the casts of what they give), a FIN, a None row, and one failing
    connection per status (E_RTO three ways)."""
    s = []
    for j, m in enumerate(VISITS):
        for p, phase in enumerate(PHASES):
            if m == 200 and p > 1:
                continue
            s.append(Script(m=m, phase=phase, mss=(1460, 536, 9000, 1460, 100)[(j + p) % 5],
                            rto=(0.3, 0.1, 1.0, 60.0, 0.2500000001)[(j + 2 * p) % 5], una=(-3000) & M32 if (j + p) % 6 == 0 else None))
    s += [Script(m=40, phase="avoidance", mss=1), Script(m=40, phase="avoidance", rto=0.0),
          Script(m=30, phase="recovery", fin=True), Script(m=20, cubic=False),
          Script(m=9, bad={"tx__state": N.DK_TCP_CLOSED}), Script(m=9, bad={"rx__send_next": 1234}),
          Script(m=9, mss=0), Script(m=9, rto=float("nan")), Script(m=9, rto=-0.5), Script(m=9, rto=1.0000001e9),
          Script(m=9, phase="avoidance", mss=0, bad={"rx__send_next": 99}),     # E_SND_NXT before E_MSS
          Script(m=9, cubic=False, mss=0, rto=float("nan"))]                    # None: neither mss nor rto matters
    return build(s, seed=seed)
