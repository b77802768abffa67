"""dk_tcp_timers on the MI355X against tests/tcp_cc_reference.py: the deadline at now - 1, now and now + 1 ns, the
fast-retransmit flag beating an expired deadline, unarmed rows, None rows that still time out, ack_fire at its three
instants, the counts, nconns = 0. Every table and output is compared whole, over a canary fill."""
import errno

import numpy as np
import pytest

import tcp_cc_reference as R
from demikernel_amd import _native as N
from demikernel_amd.rx import Fail
from demikernel_amd.tcp_ack import ack_conn_table
from demikernel_amd.tcp_ackemit import dack_conn_table, dack_to_device, dack_to_host
from demikernel_amd.tcp_cc import TimersOut, cc_conn_table, cc_to_device, cc_to_host, timers
from demikernel_amd.tcp_tx import TcpSender, tx_conn_table

pytestmark = pytest.mark.gpu
NOW = 90 * 10**9 + 77
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def sender():
    s = TcpSender(0)
    yield s
    s.close()


def tables(n: int, seed: int = 1):
    """n connections in a cycle of 12 kinds (below), random CUBIC state, rto values whose nanoseconds need the exact
    conversion."""
    rng = np.random.default_rng(seed)
    mss = rng.choice([536, 1000, 1460, 9000], n)
    tx = tx_conn_table(n, snd_nxt=rng.integers(0, 1 << 32, n), mss=mss, cwnd=0x01020304)
    tx["snd_una"] = tx["snd_nxt"] - rng.integers(0, 100000, n).astype(np.uint32)
    ak = ack_conn_table(n)
    ak["rto"] = rng.choice([0.1, 0.2, 0.3, 1.0, 59.9999999995, 60.0, 0.1 + 2.0 ** -40], n)
    ak["rtx_armed"] = 1
    cc = cc_conn_table(n, mss=mss, seq_no=tx["snd_una"], now_ns=NOW - 10**9, fast_convergence=np.arange(n) % 3 != 0)
    cc["cwnd"] = (rng.integers(1, 40, n) * mss).astype(np.uint32)
    cc["w_max"] = (rng.integers(0, 40, n) * mss).astype(np.uint32)
    cc["ssthresh"] = (rng.integers(2, 40, n) * mss).astype(np.uint32)
    cc["ltci"] = rng.integers(0, 3, n) * mss
    cc["rpif"] = rng.integers(0, 3, n)
    cc["flags"] |= np.where(rng.random(n) < 0.3, R.IN_RECOVERY, 0).astype(np.uint32)
    dack = dack_conn_table(n, armed=1, deadline_ns=NOW)
    kind = np.arange(n) % 12
    dl = np.array([R.rto_ns(float(v)) for v in ak["rto"]], np.uint64)
    ak["rtx_base_ns"] = np.uint64(NOW) - dl                      # the deadline is NOW: fires
    ak["rtx_base_ns"][kind == 1] += np.uint64(1)                 # NOW + 1: not yet
    ak["rtx_base_ns"][kind == 2] -= np.uint64(1)                 # NOW - 1: fires
    cc["flags"][kind == 3] |= R.RETRANSMIT_NOW                   # the flag beats the expired deadline
    ak["rtx_armed"][kind == 4] = 0                               # unarmed, however old the base
    for c in np.nonzero((kind == 5) | (kind == 6))[0]:           # None rows: 5 times out, 6 is not due
        cc[c] = cc_conn_table(1, mss=1000, cubic=False)[0]
    ak["rtx_base_ns"][kind == 6] += np.uint64(5)
    cc["flags"][kind == 7] |= R.RETRANSMIT_NOW                   # the flag with nothing armed
    ak["rtx_armed"][kind == 7] = 0
    dack["deadline_ns"][kind == 8] = NOW + 1                     # the delayed ACK: not yet / just passed / disarmed
    dack["deadline_ns"][kind == 9] = NOW - 1
    dack["armed"][kind == 10] = 0
    ak["rtx_armed"][kind == 11] = 7                              # any nonzero value is armed
    return tx, ak, cc, dack


def check(sender, tx, ak, cc, dack, now=NOW, with_dack=True):
    import torch

    n = len(cc)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()  # noqa: E731
    d_tx, d_ak, d_cc, d_dack = up(tx), up(ak), cc_to_device(cc), dack_to_device(dack)
    out = TimersOut(n, ack_fire=with_dack, fill=CANARY)
    timers(sender, d_tx, d_ak, d_cc, now, out, dack=d_dack if with_dack else None)
    torch.cuda.synchronize()
    got = out.to_numpy()
    etx, ecc = tx.copy(), cc.copy()
    exp = R.timers(etx, ak, ecc, now, dack if with_dack else None)
    for k in ("status", "rtx_fire") + (("ack_fire",) if with_dack else ()):
        assert np.array_equal(got[k], exp[k]), (k, np.nonzero(got[k] != exp[k])[0][:8])
    assert (got["n_fast"], got["n_timeout"], got["n_ack"]) == (exp["n_fast"], exp["n_timeout"], exp["n_ack"])
    g_cc, g_tx = cc_to_host(d_cc), d_tx.cpu().numpy().view(N.TX_CONN_DTYPE)
    rows = [c for c in range(n) if g_cc[c].tobytes() != ecc[c].tobytes() or g_tx[c].tobytes() != etx[c].tobytes()]
    assert not rows, (rows[:4], g_cc[rows[:4]], ecc[rows[:4]])
    assert d_ak.cpu().numpy().tobytes() == ak.tobytes() and dack_to_host(d_dack).tobytes() == dack.tobytes()
    got.update(cc=g_cc, tx=g_tx.copy())
    return got


@pytest.mark.parametrize("n", [1, 12, 63, 64, 65, 1000])
def test_every_kind(sender, n):
    tx, ak, cc, dack = tables(n, seed=n)
    got = check(sender, tx, ak, cc, dack)
    kind = np.arange(n) % 12
    want = np.select([kind == 1, kind == 3, kind == 4, kind == 6, kind == 7], [0, 2, 0, 0, 2], 1)
    assert np.array_equal(got["rtx_fire"], want)
    assert np.array_equal(got["ack_fire"], np.where((kind == 8) | (kind == 10), 0, 1))
    assert got["n_fast"] == (want == 2).sum() and got["n_timeout"] == (want == 1).sum()
    cubic = cc["flags"] & R.CUBIC != 0
    fired = (want == 1) & cubic  # on_rto ran: one mss, the flag of the last congestion
    assert (got["cc"]["cwnd"][fired] == tx["mss"][fired]).all() and (got["cc"]["flags"][fired] & R.LAST_WAS_RTO != 0).all()
    assert (got["cc"]["flags"] & R.RETRANSMIT_NOW == 0).all()
    assert (got["tx"]["cwnd"][~cubic] == 0x01020304).all()


def test_failures_and_no_dack(sender):
    tx, ak, cc, dack = tables(24, seed=5)
    tx["state"][0] = N.DK_TCP_CLOSED
    tx["mss"][2] = 0
    ak["rto"][8], ak["rto"][9], ak["rto"][10] = float("nan"), -1.0, 2e9
    tx["mss"][5] = 0            # a None row: mss does not matter
    ak["rtx_base_ns"][11] = 2**64 - 3   # the deadline saturates and is never reached
    got = check(sender, tx, ak, cc, dack, with_dack=False)
    assert got["status"][[0, 2, 5, 8, 9, 10, 11]].tolist() == [R.E_STATE, R.E_MSS, R.OK, R.E_RTO, R.E_RTO, R.E_RTO, R.OK]
    assert got["rtx_fire"][[0, 2, 5, 8, 9, 10, 11]].tolist() == [0, 0, 1, 0, 0, 0, 0] and got["n_ack"] == 0
    got = check(sender, tx, ak, cc, dack, now=2**64 - 1)
    assert got["rtx_fire"][11] == 1


def test_no_connections_and_argument_errors(sender):
    import torch

    tx, ak, cc, dack = tables(2)
    got = check(sender, tx[:0], ak[:0], cc[:0], dack[:0])
    assert (got["n_fast"], got["n_timeout"], got["n_ack"]) == (0, 0, 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()  # noqa: E731
    d_tx, d_ak, d_cc = up(tx), up(ak), cc_to_device(cc)
    odd = torch.zeros(d_cc.numel() + 16, dtype=torch.uint8, device=d_cc.device)[8:8 + d_cc.numel()]
    out = TimersOut(2, fill=CANARY)
    with pytest.raises(Fail) as e:
        timers(sender, d_tx, d_ak, odd, NOW, out)
    assert e.value.errno == errno.EINVAL
    torch.cuda.synchronize()
    assert (out.counts.cpu().numpy().view(np.uint32) == CANARY).all() and cc_to_host(d_cc).tobytes() == cc.tobytes()
