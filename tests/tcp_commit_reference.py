"""TEST INFRASTRUCTURE ONLY: a plain numpy restatement of dk_tcp_tx_commit and dk_tcp_rtx_piggyback (include/dk_tcp.h),
for the tests to compare against byte for byte: the "post-send operations" of Sender::send_segment (sender.rs:195-206)
and of ControlBlock::emit (ctrlblk.rs:761). One connection at a time, one frame at a time, the running sum of a
buffer's payload bytes kept literally (not the kernels' closed form).

One freedom the header leaves is pinned here so that whole regions can be compared: entries of a region outside its
new live range are unspecified after a successful commit, so `live_mask` says which pool entries a comparison may look
at: everything of untouched regions, the live range of committed ones.
"""
from __future__ import annotations

import numpy as np

OK, E_QUEUE, E_FULL = range(3)
SENT, PARTIAL = 0, 1
RTX_SENT = 1
HEADERS = 54
M32 = 0xFFFFFFFF
NONE = 0xFFFFFFFFFFFFFFFF


def tx_commit(conn, off, res: dict, ack_conns: np.ndarray, pool: dict, q_cap: int, now: int, dack=None) -> dict:
    """conn, off: the push list's arrays. res: the dk_tcp_tx_segment call's status, first_frame, frame_count [nbufs] and
    len_out [the frames written]. Returns copies: ack_conns, pool, dack (None when not given), and status, appended,
    k (the frames per connection)."""
    ak = np.array(ack_conns, copy=True)
    pool = {k: np.array(v, copy=True) for k, v in pool.items()}
    dack = None if dack is None else np.array(dack, copy=True)
    nc = len(ak)
    assert nc * q_cap <= len(pool["off"]) and now != NONE
    conn = np.asarray(conn, np.int64)
    status, appended, kk = (np.zeros(nc, np.uint32) for _ in range(3))
    for c in range(nc):
        entries = []  # (off, len) per frame, in frame order
        for b in np.nonzero(conn == c)[0]:
            if int(res["status"][b]) not in (SENT, PARTIAL):
                continue
            within = 0
            for f in range(int(res["first_frame"][b]), int(res["first_frame"][b]) + int(res["frame_count"][b])):
                ln = (int(res["len_out"][f]) - HEADERS) & M32
                entries.append(((int(off[b]) + within) & M32, ln))
                within += ln
        k = kk[c] = len(entries)
        if k == 0:
            continue
        if dack is not None:
            dack["armed"][c] = 0
        qf, qc = int(ak["q_first"][c]), int(ak["q_count"][c])
        r0, r1 = c * q_cap, (c + 1) * q_cap
        if qc > q_cap or (qc > 0 and not (r0 <= qf and qf + qc <= r1)):
            status[c] = E_QUEUE
            continue
        if qc + k > q_cap:
            status[c] = E_FULL
            continue
        if qc == 0:
            first = r0
        elif qf + qc + k <= r1:
            first = qf
        else:
            first = r0
            for name in pool:
                pool[name][r0:r0 + qc] = pool[name][qf:qf + qc].copy()
        at = first + qc
        pool["off"][at:at + k] = [e[0] for e in entries]
        pool["len"][at:at + k] = [e[1] for e in entries]
        pool["tx_time"][at:at + k] = now
        ak["q_first"][c], ak["q_count"][c] = first, qc + k
        if ak["rtx_armed"][c] == 0:
            ak["rtx_armed"][c], ak["rtx_base_ns"][c] = 1, now
        appended[c] = k
    return dict(ack_conns=ak, pool=pool, dack=dack, status=status, appended=appended, k=kk)


def live_mask(exp: dict, q_cap: int, nq: int) -> np.ndarray:
    """The pool entries whose values the contract fixes after the commit `exp` describes."""
    m = np.ones(nq, bool)
    ak = exp["ack_conns"]
    for c in np.nonzero(exp["appended"])[0]:
        m[c * q_cap:(c + 1) * q_cap] = False
        qf, qc = int(ak["q_first"][c]), int(ak["q_count"][c])
        m[qf:qf + qc] = True
    return m


def rtx_piggyback(rtx_status, dack: np.ndarray) -> np.ndarray:
    d = np.array(dack, copy=True)
    d["armed"][np.asarray(rtx_status)[:len(d)] == RTX_SENT] = 0
    return d
