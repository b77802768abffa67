"""Plain-Python restatement of CUBIC as the reference states it, for dk_tcp_cc_ack, dk_tcp_timers and dk_tcp_cc_send
(include/dk_tcp.h). Line numbers are tcp/established/congestion_control/cubic.rs's unless another file is named.

Arithmetic: u32 wraps (& M32), f32 is numpy.float32 with one operation per statement (each rounded once), Rust's
`as u32` is f32_as_u32, Duration::from_secs_f64 is rto_ns (exact, with fractions), and K's cube root is cbrt_f32: the
correctly rounded f32 cube root, found by comparing the cubes of midpoints as rationals.
"""
from __future__ import annotations

import collections
import math
import struct
from fractions import Fraction

import numpy as np

from demikernel_amd import _native as N

M32 = 0xFFFFFFFF
f32 = np.float32
CUBIC, FAST_CONVERGENCE, IN_RECOVERY, LAST_WAS_RTO, RETRANSMIT_NOW = 1, 2, 4, 8, 16
OK, E_STATE, E_SND_NXT, E_MSS, E_RTO = range(5)
RTX_NONE, RTX_TIMEOUT, RTX_FAST = range(3)
BEFORE_SEND, AFTER_SEND = 0, 1
BETA, C = f32(0.7), f32(0.4)          # :108-110
DUP_ACK_THRESHOLD = 3                  # :111
VISITED = tuple(N.A[k] for k in ("DELIVERED", "STORED", "STORE_DUP", "NO_DATA", "FIN", "ACK_UNSENT"))
ACK_UNSENT = N.A["ACK_UNSENT"]
NS = 10**9
HITS = collections.Counter()  # the branches taken, by name: the tests assert that their cases reach them


def seq_gt(a: int, b: int) -> bool:
    """SeqNumber's `>` (sequence_number.rs:76-101): the sign of the wrapping difference."""
    d = (a - b) & M32
    return 0 < d < 0x80000000


def f32_as_u32(x) -> int:
    """Rust's `f32 as u32`: NaN and negatives 0, saturating at u32::MAX, else truncation."""
    x = float(x)
    if math.isnan(x) or x <= 0.0:
        return 0
    return M32 if x >= 4294967296.0 else int(x)


def as_secs_f32(ns: int):
    """Duration::as_secs_f32: secs as f32 + nanos as f32 / 1e9f."""
    with np.errstate(all="ignore"):
        return f32(f32(ns // NS) + f32(f32(ns % NS) / f32(1e9)))


def rto_valid(rto: float) -> bool:
    return 0.0 <= rto <= 1e9  # False for NaN


def rto_ns(rto: float) -> int:
    """Duration::from_secs_f64(rto).as_nanos(): rto * 10^9 rounded to nearest, ties to even, exactly."""
    assert rto_valid(rto)
    x = Fraction(rto) * NS
    q, r = divmod(x.numerator, x.denominator)
    twice = 2 * r
    if twice > x.denominator or (twice == x.denominator and q & 1):
        q += 1
    return q


def _next_f32(y, up: bool):
    b = struct.unpack("<I", struct.pack("<f", float(y)))[0]
    return f32(struct.unpack("<f", struct.pack("<I", b + 1 if up else b - 1))[0])


def cbrt_f32(x):
    """The correctly rounded f32 cube root of a finite f32 x >= 0: from an estimate, step to the f32 y whose
    neighbouring midpoints lo < hi satisfy lo^3 <= x <= hi^3 as rationals (a tie cannot occur: a midpoint's cube has
    more than 24 significant bits)."""
    x = f32(x)
    if not x > 0 or np.isinf(x):
        return x
    X = Fraction(float(x))
    y = f32(float(x) ** (1.0 / 3.0))
    for _ in range(8):
        lo = (Fraction(float(y)) + Fraction(float(_next_f32(y, False)))) / 2
        hi = (Fraction(float(y)) + Fraction(float(_next_f32(y, True)))) / 2
        if lo ** 3 > X:
            y = _next_f32(y, False)
        elif hi ** 3 < X:
            y = _next_f32(y, True)
        else:
            assert lo ** 3 != X and hi ** 3 != X
            return y
    raise AssertionError("cbrt_f32 did not settle")


class Cubic:
    """struct Cubic (:37-59) over one CC_CONN_DTYPE row; mss from the TX table."""

    U32 = N.CC_CONN_U32
    U64 = N.CC_CONN_U64

    def __init__(self, row, mss: int, cbrt=cbrt_f32):
        for k in self.U32 + self.U64:
            setattr(self, k, int(row[k]))
        self.mss, self.cbrt = int(mss), cbrt

    def store(self, row) -> None:
        for k in self.U32 + self.U64:
            row[k] = getattr(self, k)

    def has(self, f: int) -> bool:
        return bool(self.flags & f)

    def set(self, f: int, on: bool) -> None:
        self.flags = self.flags | f if on else self.flags & ~f

    def fast_convergence_(self) -> None:  # :113-123
        if self.cwnd // self.mss < self.w_max // self.mss:
            HITS["fast_convergence_shrinks"] += 1
            a = f32(f32(self.cwnd) * f32(f32(1.0) + BETA))
            self.w_max = f32_as_u32(f32(a / f32(2.0)))
        else:
            self.w_max = self.cwnd

    def on_dup_ack_received(self, send_next: int, ack: int) -> None:  # :125-165
        self.dup_acks = (self.dup_acks + 1) & M32
        if self.dup_acks < DUP_ACK_THRESHOLD:
            HITS["limited_transmit"] += 1
            self.ltci = (self.ltci + self.mss) & M32
        diff = (ack - self.prev_ack) & M32
        covers = seq_gt((ack - 1) & M32, self.recover)                      # :141
        dropped = self.cwnd > self.mss and diff <= (4 * self.mss) & M32     # :142
        if self.dup_acks == DUP_ACK_THRESHOLD and (covers or dropped):
            HITS["enter_" + ("both" if covers and dropped else "covers" if covers else "dropped")] += 1
            self.set(IN_RECOVERY, True)
            self.recover = send_next
            reduced = f32_as_u32(f32(f32(self.cwnd) * BETA))
            if self.has(FAST_CONVERGENCE):
                self.fast_convergence_()
            else:
                self.w_max = self.cwnd
            self.ssthresh = max(reduced, (2 * self.mss) & M32)
            self.cwnd = reduced
            self.set(RETRANSMIT_NOW, True)
        elif self.dup_acks > DUP_ACK_THRESHOLD or self.has(IN_RECOVERY):
            HITS["inflate"] += 1
            self.cwnd = (self.cwnd + self.mss) & M32

    def on_ack_received_fast_recovery(self, una: int, send_next: int, ack: int, now: int) -> None:  # :167-192
        outstanding, acked = (send_next - una) & M32, (ack - una) & M32
        if seq_gt(ack, self.recover):
            HITS["full_ack"] += 1
            self.cwnd = min(self.ssthresh, (max(outstanding, self.mss) + self.mss) & M32)
            self.ca_start_ns = now
            self.set(LAST_WAS_RTO, False)
            self.set(IN_RECOVERY, False)
        else:
            self.set(RETRANSMIT_NOW, True)
            if acked >= self.mss:
                HITS["partial_ge_mss"] += 1
                self.cwnd = (self.cwnd - acked + self.mss) & M32
            else:
                HITS["partial_lt_mss"] += 1
                self.cwnd = (self.cwnd - acked) & M32

    def k(self, w):  # :194-202
        if self.has(LAST_WAS_RTO):
            HITS["k_zero"] += 1
            return f32(0.0)
        a = f32(w * f32(f32(1.0) - BETA))
        return self.cbrt(f32(a / C))

    @staticmethod
    def w_cubic(w, t, k):  # :204-208; powi(3) = (d * d) * d
        d = f32(t - k)
        d3 = f32(f32(d * d) * d)
        return f32(f32(C * d3) + w)

    @staticmethod
    def w_est(w, t, rtt):  # :210-215
        coef = f32(f32(f32(3.0) * f32(f32(1.0) - BETA)) / f32(f32(1.0) + BETA))
        return f32(f32(w * BETA) + f32(f32(coef * t) / rtt))

    def on_ack_received_ss_ca(self, rtt, una: int, ack: int, now: int) -> None:  # :217-246
        acked = (ack - una) & M32
        if self.cwnd < self.ssthresh:
            HITS["slow_start"] += 1
            self.cwnd = (self.cwnd + min(acked, self.mss)) & M32
            return
        with np.errstate(all="ignore"):
            t = as_secs_f32(max(now - self.ca_start_ns, 0))
            mss_f = f32(self.mss)
            w = f32(f32(self.w_max) / mss_f)
            k, est = self.k(w), self.w_est(w, t, rtt)
            if self.w_cubic(w, t, k) < est:
                HITS["ca_w_est"] += 1
                self.cwnd = f32_as_u32(f32(est * mss_f))
            else:
                HITS["ca_cubic"] += 1
                ncwnd = f32(f32(self.cwnd) / mss_f)
                over = f32(self.w_cubic(w, f32(t + rtt), k) - ncwnd)
                inc = f32(f32(over / ncwnd) * mss_f)
                self.cwnd = (self.cwnd + f32_as_u32(inc)) & M32

    def on_ack_received(self, rtt, una: int, send_next: int, ack: int, now: int) -> None:  # :307-328
        if (ack - una) & M32 == 0:
            self.on_dup_ack_received(send_next, ack)
            self.rpif = max(self.rpif - 1, 0)
        else:
            self.dup_acks = 0
            if self.has(IN_RECOVERY):
                self.on_ack_received_fast_recovery(una, send_next, ack, now)
            else:
                self.on_ack_received_ss_ca(rtt, una, ack, now)
            self.prev_ack = ack

    def on_rto(self, una: int) -> None:  # :248-278, :330-334
        old = self.cwnd
        if self.has(FAST_CONVERGENCE):
            self.fast_convergence_()
        else:
            self.w_max = old
        self.cwnd = self.mss
        if self.rpif == 0:
            self.ssthresh = max(f32_as_u32(f32(f32(old) * BETA)), (2 * self.mss) & M32)
        self.rpif = (self.rpif + 1) & M32
        self.set(LAST_WAS_RTO, True)
        self.recover = una
        self.set(IN_RECOVERY, False)

    def on_cwnd_check_before_send(self, now: int) -> None:  # :290-298
        if max(now - self.last_send_ns, 0) > self.rtt_at_last_send_ns:
            self.cwnd = min(self.initial_cwnd, self.cwnd)
            self.ltci = 0

    def on_send(self, rto_nanos: int, in_flight: int, now: int) -> None:  # :300-305
        self.last_send_ns = now
        self.rtt_at_last_send_ns = rto_nanos
        self.ltci = max(self.ltci - in_flight, 0)


def next_una(una: int, ack: int, action: int) -> int:
    """Sender::process_ack's move of SND.UNA, dk_tcp_ack_process's rule."""
    return ack if action != ACK_UNSENT and 0 < (ack - una) & M32 < 0x80000000 else una


def cc_ack(segs, rx, tx, ak, cc, now: int, n: int, cbrt=cbrt_f32, per_segment_rto=None) -> dict:
    """dk_tcp_cc_ack. segs[c] = [(frame index, action, ack)] of connection c in arrival order (every frame of the
    connection; the unvisited actions are skipped here). tx and cc are updated in place. per_segment_rto(c, i) ->
    seconds gives the reference's per-segment reading instead of the table's one value."""
    nconns = len(cc)
    out = {"status": np.zeros(nconns, np.uint32), "new_acks": np.zeros(nconns, np.uint32),
           "dup_acks": np.zeros(nconns, np.uint32), "cwnd_after": np.zeros(n, np.uint32)}
    for c in range(nconns):
        mss, rto, flags = int(tx["mss"][c]), float(ak["rto"][c]), int(cc["flags"][c])
        if tx["state"][c] != N.DK_TCP_ESTABLISHED:
            out["status"][c] = E_STATE
        elif rx["send_next"][c] != tx["snd_nxt"][c]:
            out["status"][c] = E_SND_NXT
        elif not flags & CUBIC:
            pass
        elif mss == 0:
            out["status"][c] = E_MSS
        elif not rto_valid(rto):
            out["status"][c] = E_RTO
        if out["status"][c] != OK or not flags & CUBIC:
            continue
        k = Cubic(cc[c], mss, cbrt)
        rtt = as_secs_f32(rto_ns(rto))
        una, nxt = int(tx["snd_una"][c]), int(tx["snd_nxt"][c])
        for i, action, ack in segs[c]:
            if action not in VISITED:
                continue
            ack = int(ack)
            out["dup_acks" if ack == una else "new_acks"][c] += 1
            r = rtt if per_segment_rto is None else as_secs_f32(rto_ns(per_segment_rto(c, i)))
            k.on_ack_received(r, una, nxt, ack, now)  # ctrlblk.rs:629
            out["cwnd_after"][i] = k.cwnd
            una = next_una(una, ack, action)
        k.store(cc[c])
        tx["cwnd"][c] = (k.cwnd + k.ltci) & M32
    return out


def timers(tx, ak, cc, now: int, dack=None) -> dict:
    """dk_tcp_timers. tx and cc are updated in place."""
    nconns = len(cc)
    out = {"status": np.zeros(nconns, np.uint32), "rtx_fire": np.zeros(nconns, np.uint8)}
    for c in range(nconns):
        mss, rto, flags = int(tx["mss"][c]), float(ak["rto"][c]), int(cc["flags"][c])
        cubic = bool(flags & CUBIC)
        if tx["state"][c] != N.DK_TCP_ESTABLISHED:
            out["status"][c] = E_STATE
        elif cubic and mss == 0:
            out["status"][c] = E_MSS
        elif not rto_valid(rto):
            out["status"][c] = E_RTO
        if out["status"][c] != OK:
            continue
        deadline = min(int(ak["rtx_base_ns"][c]) + rto_ns(rto), (1 << 64) - 1)
        fire = RTX_NONE
        if cubic and flags & RETRANSMIT_NOW:          # sender.rs:327-335
            fire = RTX_FAST
        elif ak["rtx_armed"][c] and now >= deadline:  # sender.rs:345-353, runtime/timer.rs:215
            fire = RTX_TIMEOUT
        out["rtx_fire"][c] = fire
        if cubic:
            k = Cubic(cc[c], mss)
            if fire == RTX_FAST:
                k.set(RETRANSMIT_NOW, False)          # :346-351
            elif fire == RTX_TIMEOUT:
                k.on_rto(int(tx["snd_una"][c]))
            k.store(cc[c])
            tx["cwnd"][c] = (k.cwnd + k.ltci) & M32
    out["n_fast"] = int((out["rtx_fire"] == RTX_FAST).sum())
    out["n_timeout"] = int((out["rtx_fire"] == RTX_TIMEOUT).sum())
    if dack is not None:
        out["ack_fire"] = ((dack["armed"] != 0) & (dack["deadline_ns"] <= np.uint64(now))).astype(np.uint8)
    out["n_ack"] = int(out["ack_fire"].sum()) if dack is not None else 0
    return out


def cc_send_before(tx, cc, now: int) -> np.ndarray:
    """dk_tcp_cc_send(DK_TCP_CC_BEFORE_SEND)."""
    status = np.zeros(len(cc), np.uint32)
    for c in range(len(cc)):
        if tx["state"][c] != N.DK_TCP_ESTABLISHED:
            status[c] = E_STATE
        elif cc["flags"][c] & CUBIC:
            k = Cubic(cc[c], int(tx["mss"][c]))
            k.on_cwnd_check_before_send(now)
            k.store(cc[c])
            tx["cwnd"][c] = (k.cwnd + k.ltci) & M32
    return status


def cc_send_after(tx, ak, cc, now: int, frames) -> np.ndarray:
    """dk_tcp_cc_send(DK_TCP_CC_AFTER_SEND). tx is the table after the dk_tcp_tx_segment call; frames[c] = the sequence
    space each frame of connection c consumed in that call, in order (empty: no frame, nothing changes). on_send is
    given SND.NXT - SND.UNA as it stood before the frame (sender.rs:177, ahead of :193)."""
    status = np.zeros(len(cc), np.uint32)
    for c in range(len(cc)):
        if tx["state"][c] != N.DK_TCP_ESTABLISHED:
            status[c] = E_STATE
            continue
        if not cc["flags"][c] & CUBIC or not len(frames[c]):
            continue
        rto = float(ak["rto"][c])
        if not rto_valid(rto):
            status[c] = E_RTO
            continue
        k = Cubic(cc[c], int(tx["mss"][c]))
        flight = (int(tx["snd_nxt"][c]) - sum(frames[c]) - int(tx["snd_una"][c])) & M32
        for consumed in frames[c]:
            k.on_send(rto_ns(rto), flight, now)
            flight = (flight + consumed) & M32
        k.store(cc[c])
        tx["cwnd"][c] = (k.cwnd + k.ltci) & M32
    return status
