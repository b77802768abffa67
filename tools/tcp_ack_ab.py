#!/usr/bin/env python3
"""Interleaved A/B of the sender's ACK pass against the receive walk it follows, in one process on one batch:
`--segments` data segments of 1,500-byte frames over `--conns` connections, arriving round-robin and in order, every
one DELIVERED by dk_tcp_rx_process and carrying a new ACK that acknowledges exactly one entry of its connection's
unacknowledged queue, every entry with a transmit time: one pop and one RTT sample per segment, the worst case for
the queue pass. Shape "dups": 2 % of the segments repeat the ACK before them instead; shape "karn": as "new" but every
entry retransmitted (no transmit time, so no RTT sample: what the pass costs without the fold). Neither call reads a frame byte, so
the batch is made as dk_rx results on the device (the frames exist as descriptors only).

  rx            dk_tcp_rx_process alone: the parent's cost, the yardstick
  rx_ack        dk_tcp_rx_process + dk_tcp_ack_process, the engine's rule between the forms
  rx_ack_lane   the same with one lane per connection forced (skipped above --lane-max segments per connection: one
                thread walking that many segments and entries takes seconds per call)
  rx_ack_wave   the same with one wave per connection forced
  rx_ack_chip   the same with the chip form forced (the segments' windows across the chip)

Every arm first restores the three connection tables (device copies inside the timed span, the same in every arm), so
every call does the same work. All arms are the bare C entry points through ctypes. Timing: HIP events on the launch
stream around `--iters` calls, `--reps` rounds alternating the arms after an untimed preheat; median µs per call and
the spread over rounds. The ACK pass's cost is an arm's time minus `rx`'s; `ack_over_rx` is that over `rx`. Before
timing, the forms' outputs and state are compared with each other bit for bit and with the closed form of this batch.
One JSON line per (connections, shape) on stdout.

    python tools/tcp_ack_ab.py [--segments 1048576] [--conns 1,64,16384] [--shape new|dups|karn|both] [--iters 20] [--reps 7]
        [--lane-max 65536] [--note TEXT] [--out profiles/tcp_ack_ab.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME, PAYLOAD, ENTRY = 1500, 1446, 1460


def run(a, nc, shape, lib, bid):
    import torch

    from demikernel_amd import _native as N
    from demikernel_amd.rx import RxResults
    from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table
    from demikernel_amd.tcp_ack import TcpAcker, TcpAckOut, UnackedQueue, ack_conn_table
    from demikernel_amd.tcp_tx import tx_conn_table

    dev = torch.device("cuda", 0)
    n = a.segments
    per = n // nc
    assert per * nc == n, "--segments must be a multiple of every --conns value"
    rng = np.random.default_rng(11)
    now = 100 * 10**9
    i = np.arange(n, dtype=np.int64)
    c_of, k = i % nc, i // nc  # round-robin arrival: segment k of connection c
    rn = rng.integers(0, 1 << 32, nc, dtype=np.int64)
    una = rng.integers(0, 1 << 32, nc, dtype=np.int64)
    step = np.ones(n, np.int64)  # entries this segment's ACK adds
    if shape == "dups":
        step[(rng.random(n) < 0.02) & (k > 0)] = 0
    acked_entries = np.cumsum(step.reshape(per, nc), axis=0).reshape(n)  # segment i is [k, c] of (per, nc)
    rx = RxResults(n, 1, device=dev, tcp_fields=True, counts=False)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v.astype(np.uint32)).view(np.int32)).to(dev)  # noqa: E731
    rx.t["meta"].copy_(up(np.full(n, N.V["OK_TCP"] | 6 << 8 | 0x18 << 16 | 0x50 << 24, np.int64)))
    rx.t["flow_id"].copy_(up(c_of))
    rx.t["payload"].copy_(up(np.full(n, 54 | PAYLOAD << 16, np.int64)))
    rx.t["tcp_seq"].copy_(up((rn[c_of] + k * PAYLOAD) & 0xFFFFFFFF))
    rx.t["tcp_ack"].copy_(up((una[c_of] + acked_entries * ENTRY) & 0xFFFFFFFF))
    rx.t["tcp_win"].copy_(up(rng.integers(0, 65536, n)))
    nxt = (una + per * ENTRY) & 0xFFFFFFFF
    t_rx = conn_table(nc, receive_next=rn, send_next=nxt, buffer_size=0x7FFF0000)
    t_tx = tx_conn_table(nc, snd_nxt=nxt, snd_una=una, snd_wnd=65535)
    t_ak = ack_conn_table(nc, wl1=rn, wl2=una, q_first=np.arange(nc) * per, q_count=per)
    tx_time = now - rng.integers(10**5, 10**9, n) if shape != "karn" else np.full(n, N.DK_TCP_TX_TIME_NONE, np.uint64)
    queue = UnackedQueue.from_numpy(np.arange(n, dtype=np.int64) * ENTRY & 0xFFFFFFFF, np.full(n, ENTRY), tx_time)
    tcp = TcpReceiver(0)
    tab0 = [tcp.conns_to_device(t_rx), torch.from_numpy(t_tx.view(np.uint8).copy()).to(dev), TcpAcker.conns_to_device(t_ak)]
    tab = [t.clone() for t in tab0]
    out, aout = TcpOut(n, nc), TcpAckOut(n, nc)
    stream = torch.cuda.Stream(device=0)
    sp = ctypes.c_void_p(stream.cuda_stream)
    r, o, q, ao = rx.c_struct(), out.c_struct(), queue.c_struct(), aout.c_struct()

    def restore():
        for t, t0 in zip(tab, tab0):
            t.copy_(t0, non_blocking=True)  # on `stream` (the timed loop runs under it)

    def rx_call():
        restore()
        assert lib.dk_tcp_rx_process(tcp._ctx, ctypes.byref(r), n, tab[0].data_ptr(), nc, ctypes.byref(o), sp) == 0

    def ack_call(form):
        rx_call()
        assert lib.dk_diag_tcp_ack_set_form(tcp._ctx, form) == 0
        assert lib.dk_tcp_ack_process(tcp._ctx, ctypes.byref(r), n, out.action.data_ptr(), tab[0].data_ptr(),
                                      tab[1].data_ptr(), tab[2].data_ptr(), nc, ctypes.byref(q), n, now,
                                      ctypes.byref(ao), sp) == 0

    calls = {"rx": rx_call, "rx_ack": lambda: ack_call(-1), "rx_ack_lane": lambda: ack_call(0),
             "rx_ack_wave": lambda: ack_call(1), "rx_ack_chip": lambda: ack_call(2)}
    skipped = []
    if per > a.lane_max:
        skipped.append("rx_ack_lane")
        del calls["rx_ack_lane"]

    # the forms against each other and against this batch's closed form, before any timing
    seen = {}
    with torch.cuda.stream(stream):
        for name in [x for x in calls if x != "rx"]:
            calls[name]()
            torch.cuda.synchronize()
            h = aout.to_numpy()
            seen[name] = (h, tab[1].cpu().numpy().copy(), tab[2].cpu().numpy().copy(), queue.to_numpy(),
                          lib.dk_diag_tcp_ack_last_form(tcp._ctx))
    act = out.action.cpu().numpy()
    first = next(iter(seen.values()))
    same = all(all(np.array_equal(s[0][f], first[0][f]) for f in first[0]) and np.array_equal(s[1], first[1]) and
               np.array_equal(s[2], first[2]) and all(np.array_equal(s[3][f], first[3][f]) for f in first[3])
               for s in seen.values())
    h = first[0]
    total = acked_entries.reshape(per, nc)[-1]
    closed = bool((act == N.A["DELIVERED"]).all() and (h["status"] == 0).all() and
                  np.array_equal(h["acked"], (step * ENTRY).astype(np.uint32)) and
                  np.array_equal(h["new_acks"], step.reshape(per, nc).sum(0).astype(np.uint32)) and
                  np.array_equal(h["samples"], (total * (shape != "karn")).astype(np.uint32)) and
                  np.array_equal(h["bytes_acked"], (total * ENTRY).astype(np.uint32)))

    with torch.cuda.stream(stream):
        t_end = time.perf_counter() + a.preheat_seconds
        while time.perf_counter() < t_end:  # untimed clock ramp
            rx_call()
            torch.cuda.synchronize()
        times = {name: [] for name in calls}
        for rep in range(a.reps + 1):
            for name, fn in calls.items():
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.iters):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                if rep:  # the first round is warmup
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    torch.cuda.synchronize()
    res = {name: {"us": round(float(np.median(ts)), 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)]}
           for name, ts in times.items()}
    base = res["rx"]["us"]
    for name in res:
        if name != "rx":
            res[name]["ack_us"] = round(res[name]["us"] - base, 2)
            res[name]["ack_over_rx"] = round((res[name]["us"] - base) / base, 4)
    line = json.dumps({"tool": "tcp_ack_ab", **({"note": a.note} if a.note else {}), "build": bid, "shape": shape,
                       "segments": n, "conns": nc, "per_conn": per, "iters": a.iters, "reps": a.reps,
                       "rx_walk": tcp.last_walk, "rule_form": {0: "lane", 1: "wave", 2: "chip"}.get(seen["rx_ack"][4]),
                       "forms_bit_identical": bool(same), "matches_closed_form": closed, "skipped": skipped, **res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    tcp.close()
    return bool(same) and closed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1 << 20)
    ap.add_argument("--conns", default="1,64,16384")
    ap.add_argument("--shape", choices=["new", "dups", "karn", "both"], default="both")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lane-max", type=int, default=65536, help="segments per connection above which the lane arm is skipped")
    ap.add_argument("--preheat-seconds", type=float, default=0.25)
    ap.add_argument("--note", default=None, help="free text carried in the JSON line")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch  # noqa: F401

    import __graft_entry__
    from demikernel_amd import _native as N

    bid = __graft_entry__.check_loaded_build()
    lib = N.load_library()
    ok = True
    for nc in [int(x) for x in a.conns.split(",")]:
        for shape in (["new", "dups"] if a.shape == "both" else [a.shape]):
            ok = run(a, nc, shape, lib, bid) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
