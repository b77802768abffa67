"""tests/tcp_cc_reference.py pinned on the CPU: one hand-written case per branch of cubic.rs, with the expected numbers
worked out in the comments, and the library's host helper dk_tcp_rto_ns against exact rational arithmetic. No GPU work.
Unless a case says otherwise: mss = 1,000, fast convergence on, the clock at NOW."""
import collections
import math
from fractions import Fraction

import numpy as np

import tcp_ack_reference as RA
import tcp_cc_cases as C
import tcp_cc_reference as R
from demikernel_amd import _native as N
from demikernel_amd.tcp_cc import cc_conn_table, rto_ns

NOW = 50 * 10**9
UNA, NXT = 100_000, 120_000
SEC = 10**9


def cubic(mss=1000, **over) -> R.Cubic:
    row = cc_conn_table(1, mss=mss, seq_no=UNA, now_ns=NOW)[0]
    k = R.Cubic(row, mss)
    for name, v in over.items():
        setattr(k, name, v)
    return k


def ack(k: R.Cubic, ackn: int, una=UNA, nxt=NXT, rto=1.0, now=NOW):
    k.on_ack_received(R.as_secs_f32(R.rto_ns(rto)), una, nxt, ackn, now)
    return k


def test_new_starts_as_cubic_new():
    t = cc_conn_table(4, mss=[1095, 1096, 2190, 2191], seq_no=[1, 2, 3, 0xFFFFFFFF])
    assert t["cwnd"].tolist() == [4 * 1095, 3 * 1096, 3 * 2190, 2 * 2191] == t["initial_cwnd"].tolist()
    assert (t["ssthresh"] == 0xFFFFFFFF).all() and (t["w_max"] == 0).all() and (t["rtt_at_last_send_ns"] == SEC).all()
    assert t["recover"].tolist() == t["prev_ack"].tolist() == [1, 2, 3, 0xFFFFFFFF]
    assert (t["flags"] == (R.CUBIC | R.FAST_CONVERGENCE)).all()
    assert cc_conn_table(1, mss=1460, cubic=False).tobytes() == bytes(64)  # the algorithm None


def test_slow_start_adds_min_of_bytes_and_mss():
    k = cubic()  # cwnd 4,000 < ssthresh u32::MAX
    assert ack(k, UNA + 300).cwnd == 4300           # 300 bytes acknowledged
    assert ack(k, UNA + 2800, una=UNA + 300).cwnd == 5300  # 2,500 bytes: capped at one mss
    assert k.prev_ack == UNA + 2800 and k.dup_acks == 0


def test_congestion_avoidance_below_w_est():
    # w_max = 8 mss, so K = cbrt(8 * 0.3 / 0.4) = cbrt(6) = 1.817; t = 1 s, rtt = 0.1 s:
    # w_cubic = 0.4 (1 - 1.817)^3 + 8 = 7.78; w_est = 8 * 0.7 + (3 * 0.3 / 1.7) * 1 / 0.1 = 5.6 + 5.294 = 10.894
    # w_cubic < w_est: cwnd = 10.894 * 1,000 = 10,894 (10,894.1: far from an integer boundary)
    k = cubic(cwnd=9000, ssthresh=2000, w_max=8000, ca_start_ns=NOW - SEC)
    assert ack(k, UNA + 1, rto=0.1).cwnd == 10894


def test_congestion_avoidance_cubic_increment():
    # w_max = 36 mss: K = cbrt(36 * 0.3 / 0.4) = cbrt(27) = 3; t = 5 s, rtt = 1 s:
    # w_cubic(5) = 0.4 * 2^3 + 36 = 39.2, w_est = 25.2 + 0.529 * 5 = 27.85: not below, so the cubic increment:
    # w_cubic(t + rtt = 6) = 0.4 * 27 + 36 = 46.8; cwnd = 41 mss: (46.8 - 41) / 41 * 1,000 = 141.46 -> 141
    k = cubic(cwnd=41000, ssthresh=2000, w_max=36000, ca_start_ns=NOW - 5 * SEC)
    assert ack(k, UNA + 1).cwnd == 41141
    # a target below cwnd gives a negative increment, which the cast turns into 0: cwnd = 50 mss, (46.8 - 50) / 50 < 0
    k = cubic(cwnd=50000, ssthresh=2000, w_max=36000, ca_start_ns=NOW - 5 * SEC)
    assert ack(k, UNA + 1).cwnd == 50000


def test_k_is_zero_after_an_rto():
    # last_congestion_was_rto: K = 0. w_max = 8 mss, t = 2 s, rtt = 1 s: w_cubic(2) = 0.4 * 8 + 8 = 11.2, w_est = 5.6 +
    # 0.529 * 2 = 6.66; w_cubic(3) = 0.4 * 27 + 8 = 18.8; cwnd = 9 mss: (18.8 - 9) / 9 * 1,000 = 1,088.9 -> 1,088
    k = cubic(cwnd=9000, ssthresh=2000, w_max=8000, ca_start_ns=NOW - 2 * SEC, flags=R.CUBIC | R.LAST_WAS_RTO)
    assert ack(k, UNA + 1).cwnd == 10088
    # without the flag K = 1.817: w_cubic(3) = 0.4 * 1.183^3 + 8 = 8.66: (8.66 - 9) / 9 < 0, no increment
    k = cubic(cwnd=9000, ssthresh=2000, w_max=8000, ca_start_ns=NOW - 2 * SEC)
    assert ack(k, UNA + 1).cwnd == 9000


def test_duplicate_acks_one_to_four():
    k = cubic(cwnd=10000, rpif=2)
    ack(k, UNA)   # 1st: limited transmit, one mss
    assert (k.dup_acks, k.ltci, k.cwnd, k.rpif) == (1, 1000, 10000, 1)
    ack(k, UNA)   # 2nd: another
    assert (k.dup_acks, k.ltci, k.cwnd, k.rpif) == (2, 2000, 10000, 0)
    ack(k, UNA)   # 3rd: fast retransmit. cwnd = 10,000 * 0.7f = 6,999.9999 in f32 arithmetic = 7,000.0 once rounded
    assert (k.dup_acks, k.ltci, k.cwnd, k.ssthresh, k.w_max, k.recover, k.rpif) == (3, 2000, 7000, 7000, 10000, NXT, 0)
    assert k.has(R.IN_RECOVERY) and k.has(R.RETRANSMIT_NOW)
    ack(k, UNA)   # 4th: inflation by one mss
    assert (k.dup_acks, k.ltci, k.cwnd) == (4, 2000, 8000)
    # ssthresh never falls below 2 mss: cwnd 2,000 -> 1,400, ssthresh 2,000
    k = cubic(cwnd=2000, dup_acks=2)
    ack(k, UNA)
    assert (k.cwnd, k.ssthresh) == (1400, 2000)


def test_recovery_entry_by_each_heuristic_alone_and_by_neither():
    # `ack - 1 > recover` alone: prev_ack 5,000 behind (more than 4 mss), recover below the ACK
    k = ack(cubic(cwnd=10000, dup_acks=2, prev_ack=UNA - 5000, recover=UNA - 10), UNA)
    assert k.has(R.IN_RECOVERY) and k.cwnd == 7000
    # the "retransmitted packet dropped" heuristic alone: recover ahead of the ACK, prev_ack within 4 mss, cwnd > mss
    k = ack(cubic(cwnd=10000, dup_acks=2, prev_ack=UNA - 4000, recover=UNA + 100), UNA)
    assert k.has(R.IN_RECOVERY) and k.cwnd == 7000
    # ... and not with cwnd == mss
    k = ack(cubic(cwnd=1000, dup_acks=2, prev_ack=UNA - 4000, recover=UNA + 100), UNA)
    assert not k.has(R.IN_RECOVERY) and k.cwnd == 1000
    # neither: the third duplicate changes nothing, the fourth inflates (count > threshold)
    k = ack(cubic(cwnd=10000, dup_acks=2, prev_ack=UNA - 4001, recover=UNA + 100), UNA)
    assert not k.has(R.IN_RECOVERY) and not k.has(R.RETRANSMIT_NOW) and (k.cwnd, k.dup_acks, k.ltci) == (10000, 3, 0)
    assert ack(k, UNA).cwnd == 11000
    # `ack - 1 > recover` is strict: recover == ack - 1 does not cover
    k = ack(cubic(cwnd=10000, dup_acks=2, prev_ack=UNA - 5000, recover=UNA - 1), UNA)
    assert not k.has(R.IN_RECOVERY)


def test_partial_and_full_acknowledgement():
    rec = dict(flags=R.CUBIC | R.IN_RECOVERY | R.LAST_WAS_RTO, recover=UNA + 10000, cwnd=9000, ssthresh=7000, dup_acks=5)
    k = ack(cubic(**rec), UNA + 1500)       # partial, at least one mss: cwnd - 1,500 + 1,000
    assert k.cwnd == 8500 and k.has(R.RETRANSMIT_NOW) and k.has(R.IN_RECOVERY) and k.dup_acks == 0
    k = ack(cubic(**rec), UNA + 400)        # partial, below one mss: cwnd - 400
    assert k.cwnd == 8600 and k.has(R.RETRANSMIT_NOW) and k.has(R.IN_RECOVERY)
    k = ack(cubic(**rec), UNA + 10000)      # ack == recover is still partial: 9,000 - 10,000 + 1,000 = 0
    assert k.cwnd == 0 and k.has(R.IN_RECOVERY)
    k = ack(cubic(**rec), UNA + 10001)      # full: min(ssthresh, max(20,000 outstanding, mss) + mss) = ssthresh
    assert k.cwnd == 7000 and not k.has(R.IN_RECOVERY) and not k.has(R.LAST_WAS_RTO) and not k.has(R.RETRANSMIT_NOW)
    assert k.ca_start_ns == NOW and k.prev_ack == UNA + 10001
    k = ack(cubic(**dict(rec, ssthresh=50000)), UNA + 10001)           # ... = 21,000
    assert k.cwnd == 21000
    k = ack(cubic(**dict(rec, ssthresh=50000)), UNA + 10001, nxt=UNA + 10500, una=UNA + 9900)  # 600 outstanding: 2 mss
    assert k.cwnd == 2000


def test_an_old_ack_is_new_data_to_cubic_and_wraps():
    # ack 100 behind una: bytes_acknowledged = 2^32 - 100, slow start adds min(that, mss)
    k = ack(cubic(dup_acks=2), UNA - 100)
    assert k.cwnd == 5000 and k.dup_acks == 0 and k.prev_ack == UNA - 100
    # in recovery it is a partial ACK of 2^32 - 100 bytes: cwnd - (2^32 - 100) + mss wraps to cwnd + 100 + mss
    k = ack(cubic(flags=R.CUBIC | R.IN_RECOVERY, recover=UNA + 10000, cwnd=9000), UNA - 100)
    assert k.cwnd == 10100


def test_fast_convergence_on_and_off():
    # cwnd 5 mss below w_max 9 mss: w_max = 5,000 * 1.7f / 2 = 4,250
    k = ack(cubic(cwnd=5000, w_max=9000, dup_acks=2), UNA)
    assert (k.w_max, k.cwnd) == (4250, 3500)
    k = ack(cubic(cwnd=5000, w_max=9000, dup_acks=2, flags=R.CUBIC), UNA)   # off: w_max = cwnd
    assert k.w_max == 5000
    k = ack(cubic(cwnd=5999, w_max=5000, dup_acks=2), UNA)  # 5 mss against 5 mss in whole segments: w_max = cwnd
    assert k.w_max == 5999


def test_on_rto():
    k = cubic(cwnd=10000, flags=R.CUBIC | R.FAST_CONVERGENCE | R.IN_RECOVERY, recover=7)
    k.on_rto(UNA)  # nothing retransmitted in flight: ssthresh = max(7,000, 2 mss)
    assert (k.cwnd, k.ssthresh, k.w_max, k.rpif, k.recover) == (1000, 7000, 10000, 1, UNA)
    assert k.has(R.LAST_WAS_RTO) and not k.has(R.IN_RECOVERY)
    k.on_rto(UNA + 5)  # a retransmitted packet in flight: ssthresh stays; w_max: 1 < 10 in segments, 1,000 * 1.7f / 2
    assert (k.cwnd, k.ssthresh, k.w_max, k.rpif, k.recover) == (1000, 7000, 850, 2, UNA + 5)
    k = cubic(cwnd=2500, flags=R.CUBIC)
    k.on_rto(UNA)  # 2,500 * 0.7 = 1,750 < 2 mss
    assert (k.ssthresh, k.w_max) == (2000, 2500)


def test_idle_restart_is_strictly_greater():
    k = cubic(cwnd=9000, ltci=2000, last_send_ns=NOW - SEC - 1)  # rtt_at_last_send = 1 s, idle 1 s + 1 ns
    k.on_cwnd_check_before_send(NOW)
    assert (k.cwnd, k.ltci) == (4000, 0)
    k = cubic(cwnd=9000, ltci=2000, last_send_ns=NOW - SEC)      # exactly the rtt: not a long time
    k.on_cwnd_check_before_send(NOW)
    assert (k.cwnd, k.ltci) == (9000, 2000)
    k = cubic(cwnd=3000, ltci=2000, last_send_ns=0)              # min(initial, cwnd) keeps a smaller cwnd
    k.on_cwnd_check_before_send(NOW)
    assert (k.cwnd, k.ltci) == (3000, 0)
    k = cubic(cwnd=9000, ltci=2000, last_send_ns=NOW + 5)        # the clock behind the last send: saturates at 0
    k.on_cwnd_check_before_send(NOW)
    assert (k.cwnd, k.ltci) == (9000, 2000)


def test_on_send_is_given_the_bytes_in_flight_and_saturates():
    k = cubic(ltci=2000)
    k.on_send(300_000_000, 1500, NOW + 7)
    assert (k.ltci, k.last_send_ns, k.rtt_at_last_send_ns) == (500, NOW + 7, 300_000_000)
    k.on_send(300_000_000, 3000, NOW + 8)
    assert k.ltci == 0
    # the table form: 2 mss of increase, nothing in flight before a first frame of 700 bytes, then frames of 1,000:
    # on_send sees 0, 700, 1,700 in flight (sender.rs:177 runs before SND.NXT moves): 2,000 -> 2,000 -> 1,300 -> 0
    tx = np.zeros(1, N.TX_CONN_DTYPE)
    tx["state"], tx["mss"], tx["snd_una"], tx["snd_nxt"] = N.DK_TCP_ESTABLISHED, 1000, UNA, UNA + 2700
    ak = np.zeros(1, N.ACK_CONN_DTYPE)
    ak["rto"] = 0.25
    for frames, want in (([700], 2000), ([700, 1000], 1300), ([700, 1000, 1000], 0)):
        cc = cc_conn_table(1, mss=1000)
        cc["ltci"] = 2000
        tx["snd_nxt"] = UNA + sum(frames)
        st = R.cc_send_after(tx, ak, cc, NOW, [frames])
        assert st[0] == R.OK and cc["ltci"][0] == want and cc["rtt_at_last_send_ns"][0] == 250_000_000
        assert cc["last_send_ns"][0] == NOW and tx["cwnd"][0] == 4000 + want


def test_saturating_casts():
    assert [R.f32_as_u32(np.float32(v)) for v in (np.nan, -1.5, -0.0, 0.99, 4294967040.0, 4294967296.0, np.inf)] == \
        [0, 0, 0, 0, 4294967040, 0xFFFFFFFF, 0xFFFFFFFF]
    # cwnd = 0 in congestion avoidance, w_max = 0, K = 0 after an RTO, t = 0 and rtt = 0: w_est = 0 + 0 / 0 = NaN, the
    # comparison with NaN is false, and the increment is (0 - 0) / 0 * mss = NaN, which the cast makes 0
    k = cubic(cwnd=0, ssthresh=0, w_max=0, flags=R.CUBIC | R.LAST_WAS_RTO)
    assert ack(k, UNA + 1, rto=0.0).cwnd == 0
    # the same with a w_max: (8 - 0) / 0 = +inf, saturating: cwnd = 0 + 0xFFFFFFFF
    k = cubic(cwnd=0, ssthresh=0, w_max=8000, flags=R.CUBIC | R.LAST_WAS_RTO)
    assert ack(k, UNA + 1, rto=0.0).cwnd == 0xFFFFFFFF
    # a huge t: ca_start at 0 and the clock at 2^64 - 1 ns, t = 1.8e10 s, 0.4 t^3 = 2.5e30 (finite in f32): the increment
    # saturates at 0xFFFFFFFF and the wrapping sum is cwnd - 1
    k = cubic(cwnd=9000, ssthresh=2000, w_max=8000, ca_start_ns=0, flags=R.CUBIC | R.LAST_WAS_RTO)
    assert ack(k, UNA + 1, now=2**64 - 1).cwnd == 8999
    # w_est saturating: rtt = 1 ns in the denominator. w_est = 5.6 + 0.529 * 1.8e10 / 1e-9 = 1e19 > w_cubic is false
    # (2.5e30), so make K large instead: w_max 2^32 - 1 bytes at mss 1 is 4.29e9 segments, K = cbrt(3.2e9) = 1,477 s; t =
    # 1,477 s gives w_cubic = w_max = 4.29e9 < w_est = 3.0e9 + 0.529 * 1,477 / 1e-9: cwnd = (w_est * 1) saturates
    k = cubic(mss=1, cwnd=9000, ssthresh=2000, w_max=0xFFFFFFFF, ca_start_ns=NOW - 1477 * SEC)
    assert ack(k, UNA + 1, rto=1e-9).cwnd == 0xFFFFFFFF


def test_recover_across_the_sequence_wrap():
    rec = dict(flags=R.CUBIC | R.IN_RECOVERY, recover=0xFFFFFFF0, cwnd=9000, ssthresh=7000)
    k = ack(cubic(**rec), 0x10, una=0xFFFFFF00, nxt=0x2000)     # 0x10 is above 0xFFFFFFF0: a full acknowledgement
    assert not k.has(R.IN_RECOVERY) and k.cwnd == 7000
    k = ack(cubic(**rec), 0xFFFFFFF0, una=0xFFFFFF00, nxt=0x2000)  # equal: partial, 0xF0 = 240 bytes
    assert k.has(R.IN_RECOVERY) and k.cwnd == 9000 - 240
    # ack - 1 wraps below zero: ack 0 covers recover 0xFFFFFFF0 (0xFFFFFFFF is above it), ack 0xFFFFFFF1 does not
    k = ack(cubic(cwnd=10000, dup_acks=2, prev_ack=0 - 5000 & R.M32, recover=0xFFFFFFF0), 0, una=0, nxt=0x2000)
    assert k.has(R.IN_RECOVERY) and k.recover == 0x2000
    k = ack(cubic(cwnd=10000, dup_acks=2, prev_ack=0xFFFFFFF1 - 5000, recover=0xFFFFFFF0), 0xFFFFFFF1, una=0xFFFFFFF1)
    assert not k.has(R.IN_RECOVERY)


def test_cbrt_is_correctly_rounded():
    f = np.float32
    assert R.cbrt_f32(f(27.0)) == 3.0 and R.cbrt_f32(f(0.0)) == 0.0 and R.cbrt_f32(f(1e-30)) == f(1e-10)
    rng = np.random.default_rng(5)
    for x in rng.uniform(0.1, 1e5, 300).astype(f):
        y = R.cbrt_f32(x)
        lo, hi = ((Fraction(float(y)) + Fraction(float(R._next_f32(y, u)))) / 2 for u in (False, True))
        assert lo ** 3 < Fraction(float(x)) < hi ** 3


# ---------------------------------------------------------------------------------------------------------------------
# dk_tcp_rto_ns, the host copy of the code the kernels run, against fractions
# ---------------------------------------------------------------------------------------------------------------------
def exact_ns(rto: float) -> int:
    x = Fraction(rto) * SEC
    fl = math.floor(x)
    d = x - fl
    return fl + (1 if d > Fraction(1, 2) or (d == Fraction(1, 2) and fl & 1) else 0)


def test_rto_ns_against_fractions():
    assert rto_ns(0.1) == 100_000_000 == R.rto_ns(0.1) and rto_ns(60.0) == 60 * SEC and rto_ns(1.0) == SEC
    assert rto_ns(0.0) == 0 and rto_ns(-0.0) == 0 and rto_ns(1e9) == 10**18 and rto_ns(5e-324) == 0
    # exact ties: k + 1/2 nanoseconds are k * 2^-9 * 1e-9 ... only values whose product with 10^9 is a half-integer: rto =
    # (2 k + 1) / (2 * 10^9) is not a double, but (2 k + 1) * 2^-10 seconds * 10^9 = (2 k + 1) * 5^9 / 2 is: odd / 2
    for k in (0, 1, 2, 3, 1000, 12345, 2**20 + 1):
        rto = (2 * k + 1) * 2.0 ** -10
        x = Fraction(rto) * SEC
        assert x.denominator == 2, "an exact tie"
        want = exact_ns(rto)
        assert want % 2 == 0 and abs(Fraction(want) - x) == Fraction(1, 2)  # to even
        assert rto_ns(rto) == want == R.rto_ns(rto), rto
    # an f64 product would round twice: 0.1 + ulps, values next to ties
    for base in (0.1, 0.2, 1e-9, 0.5e-9, 1.5e-9, 2.5e-9, 3.0000000005, 59.9999999995, 123456.7890000005):
        for v in (np.nextafter(base, 0), base, np.nextafter(base, 1e10)):
            assert rto_ns(float(v)) == exact_ns(float(v)) == R.rto_ns(float(v)), v
    rng = np.random.default_rng(77)
    vals = np.concatenate([rng.uniform(0.1, 60.0, 6000), rng.uniform(0, 1e9, 2000), 10.0 ** rng.uniform(-12, 9, 2000)])
    assert len(vals) == 10000
    for v in vals:
        assert rto_ns(float(v)) == exact_ns(float(v)), v
    for bad in (float("nan"), -1e-300, 1.0000000000000002e9, float("inf"), -float("inf")):
        assert rto_ns(bad) == 0 and not R.rto_valid(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the table forms
# ---------------------------------------------------------------------------------------------------------------------
def run_host(case, **kw):
    act = C.host_actions(case)
    segs = C.segs_by_conn(case["rx"]["flow_id"], act, case["rx"]["tcp_ack"], case["nconns"])
    tx, cc = case["tx"].copy(), case["cc"].copy()
    out = R.cc_ack(segs, case["table"], tx, case["ak"], cc, case["now"], case["n"], **kw)
    return out, tx, cc, act, segs


def test_walk_case_reaches_every_branch_and_status():
    case = C.walk_case()
    assert case["n"] <= 4096
    R.HITS.clear()
    out, tx, cc, act, segs = run_host(case)
    for name in ("slow_start", "ca_w_est", "ca_cubic", "k_zero", "limited_transmit", "enter_covers", "enter_dropped",
                 "enter_both", "inflate", "partial_ge_mss", "partial_lt_mss", "full_ack", "fast_convergence_shrinks"):
        assert R.HITS[name] > 0, (name, dict(R.HITS))
    visits = [sum(a in R.VISITED for _, a, _ in s) for s in segs]
    assert set(C.VISITS) <= set(visits), visits
    hist = collections.Counter(N.TCP_ACTIONS[a] for a in act)
    for name in ("SKIP", "DUPLICATE", "NO_ACK", "ACK_UNSENT", "STORED", "STORE_DUP", "DELIVERED", "NO_DATA", "FIN",
                 "UNPROCESSED"):
        assert hist[name] > 0, hist
    assert collections.Counter(out["status"].tolist()) == {R.OK: len(cc) - 8, R.E_STATE: 2, R.E_SND_NXT: 2, R.E_MSS: 1, R.E_RTO: 3}
    # unvisited frames carry 0, failing and None rows stay byte for byte
    unvisited = ~np.isin(act, R.VISITED)
    assert (out["cwnd_after"][unvisited] == 0).all()
    for c in range(len(cc)):
        if out["status"][c] != R.OK or not case["cc"]["flags"][c] & R.CUBIC:
            assert cc[c].tobytes() == case["cc"][c].tobytes() and tx[c].tobytes() == case["tx"][c].tobytes(), c
            assert out["new_acks"][c] == out["dup_acks"][c] == 0
        elif visits[c]:
            assert tx["cwnd"][c] == (int(cc["cwnd"][c]) + int(cc["ltci"][c])) & R.M32
            assert out["new_acks"][c] + out["dup_acks"][c] == visits[c]


def test_one_rto_per_call_agrees_with_per_segment_rto_without_samples():
    """The reference reads rto per segment (ctrlblk.rs:628), the call once. Sender::process_ack, run between the
    segments as the reference runs it, moves rto only when it takes an RTT sample: with every queue entry retransmitted
    (no transmit time, Karn) the two readings give the same result on every row; with samples they do not."""
    import collections as cl

    case = C.build([C.Script(m=64, phase=p, rto=0.35) for p in ("avoidance", "above_w_max", "after_rto")], seed=3)
    act = C.host_actions(case)
    seq = case["rx"]["tcp_seq"]

    def trajectory(tx_time):
        """rto as each frame's on_ack_received finds it in the reference."""
        seen = {}
        for c in range(case["nconns"] - 1):
            t, a = case["tx"][c], case["ak"][c]
            flight = int(case["pool"]["len"][c])
            q = cl.deque([0, 500, tx_time] for _ in range(flight // 500 + 1))
            s = RA.Sender(int(t["snd_una"]), int(t["snd_nxt"]), 0, int(a["wl1"]), int(a["wl2"]), 0,
                          RA.Rto(a["srtt"], a["rttvar"], a["rto"], a["received_sample"]), q, 1, 0)
            for i in np.nonzero(case["rx"]["flow_id"] == c)[0]:
                if act[i] in R.VISITED:
                    seen[(c, int(i))] = s.rto.rto
                    if act[i] != R.ACK_UNSENT:
                        s.process_ack(int(seq[i]), int(case["rx"]["tcp_ack"][i]), 0, case["now"])
        return seen

    once = run_host(case)
    quiet = trajectory(RA.NONE)
    assert set(quiet.values()) == {0.35}
    per = run_host(case, per_segment_rto=lambda c, i: quiet[(c, i)])
    assert per[2].tobytes() == once[2].tobytes() and np.array_equal(per[0]["cwnd_after"], once[0]["cwnd_after"])
    moving = trajectory(case["now"] - 20_000_000)  # samples of 20 ms: rto falls to its floor of 0.1 s
    assert len(set(moving.values())) > 1
    per = run_host(case, per_segment_rto=lambda c, i: moving[(c, i)])
    assert not np.array_equal(per[0]["cwnd_after"], once[0]["cwnd_after"])


def test_timers_table_form():
    n = 8
    tx = np.zeros(n, N.TX_CONN_DTYPE)
    tx["state"], tx["mss"], tx["snd_una"] = N.DK_TCP_ESTABLISHED, 1000, UNA
    ak = np.zeros(n, N.ACK_CONN_DTYPE)
    ak["rto"], ak["rtx_armed"], ak["rtx_base_ns"] = 0.3, 1, NOW - 300_000_000   # the deadline is NOW
    cc = cc_conn_table(n, mss=1000)
    cc["cwnd"] = 10000
    ak["rtx_base_ns"][1] += 1                       # a nanosecond in the future
    cc["flags"][2] |= R.RETRANSMIT_NOW              # the flag beats an expired deadline
    ak["rtx_armed"][3] = 0
    cc[4] = cc_conn_table(1, mss=1000, cubic=False)[0]   # None still times out
    tx["state"][5] = N.DK_TCP_CLOSED
    ak["rto"][6] = float("nan")
    ak["rtx_base_ns"][7] = 2**64 - 5                # the deadline saturates: never reached
    out = R.timers(tx, ak, cc, NOW)
    assert out["rtx_fire"].tolist() == [1, 0, 2, 0, 1, 0, 0, 0] and (out["n_fast"], out["n_timeout"]) == (1, 2)
    assert out["status"].tolist() == [0, 0, 0, 0, 0, R.E_STATE, R.E_RTO, 0]
    assert cc["cwnd"].tolist() == [1000, 10000, 10000, 10000, 0, 10000, 10000, 10000]
    assert cc["flags"][2] == R.CUBIC | R.FAST_CONVERGENCE and cc["flags"][0] & R.LAST_WAS_RTO
    assert tx["cwnd"].tolist() == [1000, 10000, 10000, 10000, 0, 0, 0, 10000]
