"""K's cube root on the MI355X: the device's function must equal the correctly rounded f32 cube root (tests/
tcp_cc_reference.py's, by rational comparison of midpoint cubes) on perfect cubes, on the f32 neighbours of m^3 for
2,000 random 25-bit midpoints m (the hardest inputs: the real root lies next to a rounding boundary), and on 2,000
uniform values. Twice: through dk_diag_tcp_cc_cbrt, which runs the lanes' function over an array, and through
dk_tcp_cc_ack itself, on a table of connections whose w_max / mss make cubic.rs:200's argument hit the values that are
reachable that way, observed through the congestion-avoidance increment it feeds."""
import functools

import numpy as np
import pytest

import tcp_cc_cases as C
import tcp_cc_reference as R
from demikernel_amd import _native as N

f32 = np.float32


def _bits(x):
    return np.asarray(x, f32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def cases() -> np.ndarray:
    rng = np.random.default_rng(2024)
    cubes = np.array([float(k) ** 3 for k in list(range(1, 200)) + [255, 256, 257]] + [2.0 ** (3 * e) for e in range(-10, 11)])
    # 25-bit midpoints m = (2^24 + odd) * 2^e, e in three residues mod 3, and the two f32 values around m^3
    near = []
    for _ in range(2000):
        m = (2 * int(rng.integers(1 << 23, 1 << 24)) + 1) * 2.0 ** int(rng.integers(-27, -18))  # exact in f64
        cube = f32(m * m * m)
        near += [cube, np.nextafter(cube, f32(0)), np.nextafter(cube, f32(np.inf))]
    uniform = rng.uniform(0.1, 1e5, 2000)
    return np.concatenate([cubes, np.array(near, np.float64), uniform]).astype(f32)


@functools.lru_cache(maxsize=None)
def _exact_cached() -> np.ndarray:
    return np.array([R.cbrt_f32(v) for v in cases()], f32)


def exact(x: np.ndarray) -> np.ndarray:
    return _exact_cached() if x is cases() else np.array([R.cbrt_f32(v) for v in x], f32)


@pytest.mark.gpu
def test_device_cube_root_is_correctly_rounded():
    from demikernel_amd.tcp_cc import device_cbrt

    x = cases()
    got, want = device_cbrt(x), exact(x)
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert not len(bad), (len(bad), x[bad[:8]], got[bad[:8]], want[bad[:8]])
    assert R.cbrt_f32(f32(27.0)) == 3.0 and got[2] == 3.0
    # the check has teeth: a faithful cube root (numpy's f32) misses some of these inputs by an ulp
    assert (_bits(np.cbrt(x)) != _bits(want)).any()


def argument(w_max: int, mss: int):
    """cubic.rs:200's argument for a row."""
    w = f32(f32(w_max) / f32(mss))
    return f32(f32(w * f32(f32(1.0) - R.BETA)) / R.C)


def rows_hitting(targets: np.ndarray):
    """For each target x a (w_max, mss = 2^s) whose argument is exactly x, where one exists."""
    out = []
    for x in targets:
        v = f32(float(x) * 0.4 / 0.3)
        for _ in range(4):
            v = np.nextafter(v, f32(0))
        for _ in range(9):
            m, e = np.frexp(float(v))  # v = m * 2^e, m in [0.5, 1)
            V, e = int(m * (1 << 24)), e - 24
            s = max(0, -e)
            w_max = V << (e + s) if e + s >= 0 else 0
            if 0 < w_max <= R.M32 and s < 32 and argument(w_max, 1 << s) == x:
                out.append((float(x), w_max, 1 << s))
                break
            v = np.nextafter(v, f32(np.inf))
    return out


@pytest.mark.gpu
def test_cube_root_through_the_congestion_window():
    import torch

    from demikernel_amd.tcp import TcpOut, TcpReceiver
    from demikernel_amd.tcp_cc import CcAckOut, cc_ack, cc_to_device, cc_to_host
    from test_gpu_tcp import rx_device

    rows = rows_hitting(cases()[::3])[:1500]
    assert len(rows) > 1000
    # one new ACK per connection on a row in congestion avoidance at t = 0 with rtt = 0: w_est is NaN, so the increment
    # is (w_cubic(0, K) - 1) * mss with w_cubic = 0.4 * (-K)^3 + w_max / mss: K's last bit moves it
    case = C.build([C.Script(m=1, rto=0.0, fillers=False) for _ in rows], seed=8)
    for c, (_, w_max, mss) in enumerate(rows):
        case["tx"]["mss"][c] = mss
        row = case["cc"][c]
        row["cwnd"], row["ssthresh"], row["w_max"], row["ca_start_ns"] = mss, 0, w_max, case["now"]
        case["cc"][c] = row
    conn = case["rx"]["flow_id"]  # every frame a new ACK of one byte
    case["rx"]["tcp_ack"][:] = case["tx"]["snd_una"][conn] + np.uint32(1)
    case["rx"]["meta"][:] = N.V["OK_TCP"] | 6 << 8 | 0x10 << 16 | 0x50 << 24
    case["rx"]["tcp_seq"][:] = case["table"]["receive_next"][conn]
    case["rx"]["payload"][:] = 54
    tcp = TcpReceiver(0)
    try:
        r, out = rx_device(case["rx"]), TcpOut(case["n"], case["nconns"])
        d_rx = tcp.conns_to_device(case["table"])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()  # noqa: E731
        d_tx, d_ak, d_cc = up(case["tx"]), up(case["ak"]), cc_to_device(case["cc"])
        tcp.process(r, d_rx, out)
        res = CcAckOut(case["n"], case["nconns"])
        cc_ack(tcp, r, out, d_rx, d_tx, d_ak, d_cc, case["now"], res)
        torch.cuda.synchronize()
        act, got, got_cc = out.to_numpy()["action"], res.to_numpy(), cc_to_host(d_cc)
    finally:
        tcp.close()
    segs = C.segs_by_conn(case["rx"]["flow_id"], act, case["rx"]["tcp_ack"], case["nconns"])
    R.HITS.clear()
    tx, cc = case["tx"].copy(), case["cc"].copy()
    exp = R.cc_ack(segs, case["table"], tx, case["ak"], cc, case["now"], case["n"])
    assert R.HITS["ca_cubic"] == len(rows) and (got["status"][:-1] == R.OK).all()  # the last row is no connection
    assert np.array_equal(got["cwnd_after"], exp["cwnd_after"]) and got_cc.tobytes() == cc.tobytes()
    # the observation has teeth: with a merely faithful cube root some of these windows differ
    tx2, cc2 = case["tx"].copy(), case["cc"].copy()
    off = R.cc_ack(segs, case["table"], tx2, case["ak"], cc2, case["now"], case["n"], cbrt=lambda v: f32(np.cbrt(f32(v))))
    assert not np.array_equal(off["cwnd_after"], exp["cwnd_after"])


def test_rows_hit_their_targets():
    """CPU: the search above does what it says."""
    rows = rows_hitting(cases()[:300:3])
    assert len(rows) > 60
    for x, w_max, mss in rows:
        assert argument(w_max, mss) == f32(x) and 0 < w_max <= R.M32 and mss & (mss - 1) == 0
    assert N.CC_CONN_DTYPE.itemsize == 64
