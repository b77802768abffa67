"""TEST INFRASTRUCTURE ONLY: batches for the dk_tcp_ack_emit tests, as dk_rx result arrays (no frames: the GPU tests
upload them as tests/test_gpu_tcp.py does). Every connection gets a script of segments in arrival order that reaches
every row of dk_tcp.h's ACK table: in-order data, pure ACKs, out-of-order data and the segment that fills the hole,
retransmissions that overlap RCV.NXT, an old SYN that is trimmed off, entirely old segments and segments beyond the
window (with and without RST: the key kernel classifies them early, apart from the walked ones), in-window SYNs,
segments without the ACK bit or acknowledging unsent data, and a FIN or an RST part of the way through, after which
the rest is never processed. The scripts are merged into one batch in random order (each connection's own order kept)
with frames of no connection between."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from demikernel_amd import _native as N
from demikernel_amd import synth
from demikernel_amd.tcp import conn_table
from demikernel_amd.tcp_ackemit import dack_conn_table

M32 = 0xFFFFFFFF
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
KINDS = ("data", "ack", "stored", "dup", "oow", "duprst", "oowrst", "noack", "unsent", "syn", "retrans", "synold")
MIXED = (0.36, 0.2, 0.08, 0.06, 0.06, 0.02, 0.02, 0.03, 0.03, 0.03, 0.08, 0.03)
PLAIN = (1.0,) + (0.0,) * 11


@dataclass
class Script:
    m: int                   # segments
    mix: tuple = MIXED       # probabilities of KINDS
    close: str = ""          # "fin" / "rst" at segment m // 2
    rn: int | None = None    # RCV.NXT at the start (random unless given)
    unread: int = 0          # bytes the application has not read yet
    bufsz: int = 60000
    wscale: int = 0
    armed: int | None = None  # random unless given
    big: bool = False        # data segments of up to 1,400 bytes (to fill a window)


def build(scripts: list[Script], seed: int = 1, skip_every: int = 9, total: int | None = None) -> dict:
    """-> dict: rx (the dk_rx result arrays), table (CONN_DTYPE, before the batch), tx (TX_CONN_DTYPE), dack, n, nconns.
    One more row than scripts: the last is DK_TCP_NONE. total: pad with frames of no connection to exactly this many."""
    import tx_segment_reference as M

    rng = np.random.default_rng(seed)
    nc = len(scripts)
    nrows = nc + 1
    flows = synth.make_flows(nrows, seed=seed, passive=False)
    snd = rng.integers(0, 1 << 32, nrows, dtype=np.uint64)
    table = conn_table(nrows, send_next=snd)
    # the ACKs go from the local end of each flow to its remote end
    tx = M.conns_toward(flows, seed=seed, snd_nxt=snd, local_ip=flows["local_ip"], remote_ip=flows["remote_ip"],
                        ports=flows["local_port"].astype(np.uint32) | flows["remote_port"].astype(np.uint32) << 16)
    table["state"][nc:] = N.DK_TCP_NONE
    tx["state"][nc:] = N.DK_TCP_NONE
    dack = dack_conn_table(nrows, delay_ns=rng.integers(1, 1 << 40, nrows, dtype=np.uint64),
                           deadline_ns=rng.integers(1, 1 << 50, nrows, dtype=np.uint64))
    per = []
    for c, s in enumerate(scripts):
        rn = int(rng.integers(0, 1 << 32)) if s.rn is None else s.rn & M32
        table["receive_next"][c], table["reader_next"][c] = rn, (rn - s.unread) & M32
        table["buffer_size"][c], tx["rcv_wscale"][c] = s.bufsz, s.wscale
        dack["armed"][c] = int(rng.integers(0, 2)) if s.armed is None else s.armed
        wend = s.bufsz - s.unread  # offset of the window's end from rn
        nxt = int(snd[c])
        pos, held, segs = 0, None, []
        kinds = rng.choice(len(KINDS), s.m, p=s.mix)
        for k in range(s.m):
            kind = KINDS[kinds[k]]
            seq, ln, flags, ackn = pos, int(rng.integers(1, 1401 if s.big else 9)), PSH | ACK, nxt
            if s.close and k == s.m // 2:
                kind = "close"
                flags, ln = ((FIN | ACK), int(rng.integers(0, 4))) if s.close == "fin" else ((RST | ACK), 0)
            if kind == "ack":
                flags, ln = ACK, 0
            elif kind == "stored":  # ln bytes, ln bytes ahead of the stream; the next data segment fills the hole
                if held is not None:  # the stored segment again: inside stored data
                    seq, ln = pos + held, held
                elif pos + 3 * ln >= wend:
                    kind = "data"
                else:
                    held, seq = ln, pos + ln
            elif kind in ("dup", "duprst"):
                seq, ln = pos - 600, 100
                flags |= RST if kind == "duprst" else 0
            elif kind in ("oow", "oowrst"):
                seq = wend + int(rng.integers(0, 5000))
                flags |= RST if kind == "oowrst" else 0
            elif kind == "noack":
                flags = PSH
            elif kind == "unsent":
                ackn = (nxt + 1 + int(rng.integers(0, 1000))) & M32
            elif kind == "syn":
                flags, ln = SYN | ACK, 0
            elif kind == "retrans":  # three old bytes in front
                if pos < 3 or held is not None:
                    kind = "data"
                else:
                    seq, ln = pos - 3, ln + 3
                    pos += ln - 3
            elif kind == "synold":  # an old SYN in front of new bytes: trimmed off, it took one sequence number
                if pos < 1 or held is not None:
                    kind = "data"
                else:
                    seq, flags = pos - 1, SYN | ACK | PSH
                    pos += ln
            if kind == "data":
                if held is not None:
                    ln, pos, held = held, pos + 2 * held, None
                else:
                    pos += ln
            elif kind == "close" and s.close == "fin":
                pos += ln
            segs.append(((rn + seq) & M32, ackn, flags, ln))
        per.append(segs)
    order = np.repeat(np.arange(nc), [len(p) for p in per])
    rng.shuffle(order)
    nxt_i = [0] * nc
    rows = []
    for j, c in enumerate(order):
        rows.append((c,) + per[c][nxt_i[c]])
        nxt_i[c] += 1
        if skip_every and j % skip_every == skip_every - 1:
            rows.append(None)
    if total is not None:
        assert len(rows) <= total, (len(rows), total)
        rows += [None] * (total - len(rows))
    n = len(rows)
    rx = {k: np.zeros(n, np.uint32) for k in ("meta", "flow_id", "tcp_seq", "tcp_ack", "payload")}
    for i, row in enumerate(rows):
        if row is None:  # a UDP datagram, a segment of no socket, or one for the row that is no connection
            which = i % 3
            rx["meta"][i] = (N.V["OK_UDP"] | 17 << 8) if which == 0 else (6 << 8 | ACK << 16 | 0x50 << 24)
            rx["flow_id"][i] = (0, N.DK_FLOW_NONE, nc)[which]
            rx["tcp_seq"][i], rx["payload"][i] = i, 54 | 5 << 16
            continue
        c, seq, ackn, flags, ln = row
        rx["meta"][i] = 6 << 8 | flags << 16 | 0x50 << 24
        rx["flow_id"][i], rx["tcp_seq"][i], rx["tcp_ack"][i], rx["payload"][i] = c, seq, ackn, 54 | ln << 16
    return {"rx": rx, "table": table, "tx": tx, "dack": dack, "n": n, "nconns": nrows, "flows": flows}


def uniform(nconns: int, m: int, seed: int = 0, **kw) -> dict:
    """nconns connections of m segments each; every third closes half way (FIN, RST in turn), every fifth starts with
    unread bytes, every seventh at a window scale of 14, one in four across 2^32."""
    s = []
    for c in range(nconns):
        ws = 14 if c % 7 == 3 else 0
        s.append(Script(m=m, close=("", "", "fin", "", "", "rst")[c % 6] if m >= 4 else "",
                        rn=(1 << 32) - 5 * (c + 1) if c % 4 == 1 else None, unread=1000 if c % 5 == 2 else 0,
                        bufsz=(1 << 29) if ws else 60000, wscale=ws))
    return build(s, seed=1000 * nconns + m + seed, **kw)
