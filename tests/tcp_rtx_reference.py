"""TEST INFRASTRUCTURE ONLY: a plain-Python / numpy restatement of dk_tcp_retransmit (include/dk_tcp.h) for the tests to
compare against byte for byte.

    Sender::retransmit                                 layer4/tcp/established/sender.rs:375-403
    background_retransmitter, the timeout branch       sender.rs:347-364
    RtoCalculator::back_off / update_rto's clamp       rto.rs:70-84

One connection at a time, in connection order: the checks in the header's order, the frame from the front entry of the
unacknowledged queue as it stands, the state writes, and the call's all-or-nothing capacity rule. Header bytes come
from tests/tx_reference.py with the descriptor dk_tcp_tx_segment's restatement (tests/tx_segment_reference.py) uses.
"""
from __future__ import annotations

import numpy as np

import tx_reference as R
import tx_segment_reference as M

(NOT_FIRED, SENT, IDLE, E_FIRE, E_STATE, E_QUEUE, E_RANGE, E_SLOT, E_LINK, E_WINDOW, NO_ROOM) = range(11)
FIRE_NONE, FIRE_TIMEOUT, FIRE_FAST = range(3)
NO_FRAME = 0xFFFFFFFF
NONE = 0xFFFFFFFFFFFFFFFF  # DK_TCP_TX_TIME_NONE
FIN, PSH, ACK = M.FIN, M.PSH, M.ACK


def back_off(rto: float) -> float:
    """RtoCalculator::back_off: update_rto(rto * 2.0), whose clamp is to [0.1, 60.0]."""
    r = float(rto) * 2.0
    if r < 0.1:
        r = 0.1
    if r > 60.0:
        r = 60.0
    return r


def retransmit(src: np.ndarray, fire, tx_conns: np.ndarray, ack_conns: np.ndarray, pool: dict, now_ns: int,
               links: np.ndarray, out: np.ndarray, *, slot_stride: int, frame_lead: int = 0, max_frames: int,
               rx_conns=None, flags: int = 0, src_bytes=None, out_bytes=None) -> dict:
    """dk_tcp_retransmit over host arrays. pool: {"off", "len", "tx_time"}. Returns copies of `out`, `ack_conns` and the
    pool after the call, the result arrays (per-frame arrays hold the frames written: none when the call ran out of
    room) and `desc`, the planned frames as (connection, off, len, seq, ack, tcp flags, window)."""
    out = np.array(out, np.uint8, copy=True)
    ak = np.array(ack_conns, copy=True)
    pool = {k: np.array(v, copy=True) for k, v in pool.items()}
    tx = tx_conns
    fire = np.asarray(fire, np.uint8)
    nc, nq = len(fire), len(pool["off"])
    sb = src.size if src_bytes is None else src_bytes
    ob = out.size if out_bytes is None else out_bytes
    status = np.zeros(nc, np.uint32)
    frame = np.full(nc, NO_FRAME, np.uint32)
    desc = []
    for c in range(nc):
        f = int(fire[c])
        if f == FIRE_NONE:
            continue
        if f > FIRE_FAST:
            status[c] = E_FIRE
            continue
        T, A = tx[c], ak[c]
        qf, qc = int(A["q_first"]), int(A["q_count"])
        ack, win = int(T["rcv_nxt"]), int(T["rcv_wnd_hdr"])
        if rx_conns is not None:
            ack, win = int(rx_conns[c]["receive_next"]), M.header_window(rx_conns[c], int(T["rcv_wscale"]))
        if int(T["state"]) != M.ESTABLISHED:
            status[c] = E_STATE
        elif qf + qc > nq:
            status[c] = E_QUEUE
        elif int(T["link"]) >= len(links):
            status[c] = E_LINK
        elif win is None:
            status[c] = E_WINDOW
        elif qc == 0 or (f == FIRE_TIMEOUT and not int(A["rtx_armed"])):
            status[c] = IDLE
        else:
            off, ln = int(pool["off"][qf]), int(pool["len"][qf])
            if off + ln > sb:
                status[c] = E_RANGE
            elif ln > M.MAX_MSS or frame_lead + 54 + ln > slot_stride:
                status[c] = E_SLOT
            else:
                status[c] = SENT
                desc.append((c, off, ln, int(T["snd_una"]), ack, ACK | (PSH if ln else FIN), win))
    need = len(desc)
    fits = need <= max_frames and need * slot_stride <= ob
    n = need if fits else 0
    off_out, len_out, frame_conn = np.zeros(n, np.uint32), np.zeros(n, np.uint16), np.zeros(n, np.uint32)
    if not fits:
        status[status == SENT] = NO_ROOM
    else:
        for k, (c, off, ln, seq, ack, fl, win) in enumerate(desc):
            T = tx[c]
            payload = src[off:off + ln].tobytes()
            link = links[int(T["link"])]
            h = R.headers(payload, 6, int(T["local_ip"]), int(T["remote_ip"]), int(T["ports"]),
                          meta=6 << 8 | fl << 16 | 5 << 28, seq=seq, ack=ack, winurg=win, ipw=int(T["ip_word"]),
                          dst_mac=bytes(link["dst_mac"]), src_mac=bytes(link["src_mac"]), flags=flags)
            a = k * slot_stride + frame_lead
            out[a:a + 54 + ln] = np.frombuffer(h + payload, np.uint8)
            off_out[k], len_out[k], frame_conn[k], frame[c] = a, 54 + ln, c, k
            pool["tx_time"][int(ak["q_first"][c])] = NONE  # Karn
            if int(fire[c]) == FIRE_TIMEOUT:
                ak["rto"][c] = back_off(ak["rto"][c])
                ak["rtx_base_ns"][c] = now_ns
                ak["rtx_armed"][c] = 1
    return dict(out=out, ack_conns=ak, pool=pool, status=status, frame=frame, n_frames=need, off_out=off_out,
                len_out=len_out, frame_conn=frame_conn, desc=desc)
