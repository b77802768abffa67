"""Case builder for the close tests: a table of closing connections, the segments their peers send them, and the
batches the tests need. A segment is (connection, flags, ack, seq), or None for traffic of no closing connection; a
batch of them becomes dk_rx result arrays (rx_arrays, uploaded as tests/test_gpu_tcp.py uploads them) or real
Ethernet / IPv4 / TCP frames (frame_of, on tests/frames.py) for the tests that go through the receive engine."""
from __future__ import annotations

import itertools

import numpy as np

import frames as F
import tcp_close_reference as R
import tx_segment_reference as M
from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd import tcp_close as TCL
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_ackemit import dack_conn_table

M32 = R.M32
FIN, SYN, RST, PSH, ACK = R.FIN, R.SYN, R.RST, R.PSH, R.ACK
LINKS = M.links_table()
NOW = 9_000_000_000
KINDS = ("none", "A", "U", "F", "AF", "UF")
LIVE = R.LIVE


def table(states, seed: int = 1, snd_nxt=None, rcv_nxt=None, **tx_fields) -> dict:
    """One connection per entry of `states` (the closer row's state), every table the calls take: rows, rx (CONN_DTYPE:
    CLOSED where the row is live, ESTABLISHED elsewhere), tx, dack (armed at random), flows."""
    rng = np.random.default_rng(seed)
    nc = len(states)
    flows = synth.make_flows(nc, seed=seed, passive=False)
    snd = rng.integers(0, 1 << 32, nc, dtype=np.uint64) if snd_nxt is None else np.asarray(snd_nxt, np.uint64)
    rn = rng.integers(0, 1 << 32, nc, dtype=np.uint64) if rcv_nxt is None else np.asarray(rcv_nxt, np.uint64)
    rx = conn_table(nc, send_next=snd, receive_next=rn)
    rx["reader_next"] = (rn - rng.integers(0, 2000, nc, dtype=np.uint64)) & M32
    rx["buffer_size"] = 60000
    st = np.asarray(states)
    rx["state"] = np.where(np.isin(st, LIVE), N.DK_TCP_CLOSED, N.DK_TCP_ESTABLISHED)
    # the ACKs go from the local end of each flow to its remote end
    tx = M.conns_toward(flows, seed=seed, snd_nxt=snd, local_ip=flows["local_ip"], remote_ip=flows["remote_ip"],
                        ports=flows["local_port"].astype(np.uint32) | flows["remote_port"].astype(np.uint32) << 16)
    for k, v in tx_fields.items():
        tx[k] = v
    rows = TCL.closer_table(nc, state=st, linger_ns=rng.integers(1, 1 << 40, nc, dtype=np.uint64),
                            deadline_ns=rng.integers(1, 1 << 50, nc, dtype=np.uint64))
    dack = dack_conn_table(nc, delay_ns=rng.integers(1, 1 << 40, nc, dtype=np.uint64),
                           deadline_ns=rng.integers(1, 1 << 50, nc, dtype=np.uint64), armed=rng.integers(0, 2, nc))
    return {"rows": rows, "rx": rx, "tx": tx, "dack": dack, "flows": flows, "nconns": nc}


def seg(t: dict, c: int, kind: str, k: int = 0, seq: int | None = None):
    """A segment of `kind` for connection c: A acknowledges snd_nxt - k, U snd_nxt + 1 + k."""
    nxt = int(t["tx"]["snd_nxt"][c])
    flags = (FIN if "F" in kind else 0) | (ACK if "A" in kind or "U" in kind else 0)
    if kind == "none":
        flags = PSH
    ack = (nxt - k) & M32 if "A" in kind else (nxt + 1 + k) & M32 if "U" in kind else (nxt + 5) & M32
    return (c, flags, ack, (int(t["rx"]["receive_next"][c]) + 3 * k) & M32 if seq is None else seq)


def rx_arrays(segs, nconns: int) -> dict:
    """The dk_rx result arrays of a batch of segments. None: a UDP datagram, a TCP segment of no socket, or one whose
    flow id lies beyond the tables, in turn."""
    n = len(segs)
    rx = {k: np.zeros(n, np.uint32) for k in ("meta", "flow_id", "tcp_seq", "tcp_ack", "payload")}
    for i, s in enumerate(segs):
        if s is None:
            which = i % 3
            rx["meta"][i] = (N.V["OK_UDP"] | 17 << 8) if which == 0 else (N.V["TCP_NOSOCK"] | 6 << 8 | (ACK | FIN) << 16 | 0x50 << 24) \
                if which == 1 else (6 << 8 | (ACK | FIN) << 16 | 0x50 << 24)
            rx["flow_id"][i] = (0, N.DK_FLOW_NONE, nconns + i % 5)[which]
            rx["tcp_seq"][i], rx["tcp_ack"][i], rx["payload"][i] = i, 7 * i, 54 | 5 << 16
            continue
        c, flags, ack, seq = s
        rx["meta"][i] = 6 << 8 | flags << 16 | 0x50 << 24
        rx["flow_id"][i], rx["tcp_seq"][i], rx["tcp_ack"][i], rx["payload"][i] = c, seq, ack, 54
    return rx


def frame_of(t: dict, s) -> bytes:
    """The segment as a frame from the remote end of connection c's flow to its local end."""
    c, flags, ack, seq = s
    f = t["flows"][c]
    return F.tcp_frame(src=int(f["remote_ip"]), dst=int(f["local_ip"]), sport=int(f["remote_port"]),
                       dport=int(f["local_port"]), tcp_kw=dict(seq=seq, ack=ack, flags=flags, window=65535))


def interleave(scripts, pad_every: int = 0):
    """Round-robin over the scripts: a row's frames are never adjacent (with two rows or more)."""
    out = []
    for j in range(max((len(s) for s in scripts), default=0)):
        for s in scripts:
            if j < len(s):
                out.append(s[j])
                if pad_every and len(out) % pad_every == 0:
                    out.append(None)
    return out


def exhaustive():
    """Every sequence of 1 to 4 frames over the six kinds from each of the four live states, one row each: 6,216 rows,
    23,640 frames, as one batch."""
    seqs = [q for m in range(1, 5) for q in itertools.product(KINDS, repeat=m)]
    states = [s for s in LIVE for _ in seqs]
    t = table(states, seed=11)
    scripts = [[seg(t, c, kind, k) for k, kind in enumerate(seqs[c % len(seqs)])] for c in range(len(states))]
    return t, interleave(scripts)


def long_row(t: dict, c: int, m: int, decide_at: int | None, kind: str = "AF", idle: str = "none"):
    """m frames for row c: `idle` frames that change nothing, and the deciding `kind` at index decide_at."""
    return [seg(t, c, kind if k == decide_at else idle, k % 7) for k in range(m)]
