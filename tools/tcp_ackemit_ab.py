#!/usr/bin/env python3
"""Interleaved A/B of the receiver's ACK pass against the receive walk it follows, in one process on one batch:
`--segments` data segments of 100 bytes over `--conns` connections, arriving round-robin, made as dk_rx results on the
device (neither call reads a frame byte). Shape "inorder": every segment in order and DELIVERED, so the delayed ACK
sends one ACK per two segments. Shape "strays": 5 % of the segments lie beyond the window instead (OUT_OF_WINDOW, the
key kernel classifies them early, apart from the walked ones): each is acknowledged at once with the RCV.NXT of its
arrival and clears the deadline.

  rx             dk_tcp_rx_process alone: the parent's cost, the yardstick
  rx_emit        dk_tcp_rx_process + dk_tcp_ack_emit, the engine's rule between the forms
  rx_emit_lane   the same with one lane per connection forced (skipped above --lane-max segments per connection)
  rx_emit_scan   the same with the scan form forced

Every arm first restores the receive table and the dack table (device copies inside the timed span, the same in every
arm), so every call does the same work. All arms are the bare C entry points through ctypes. Timing: HIP events on the
launch stream around `--iters` calls, `--reps` rounds alternating the arms after an untimed preheat; median µs per
call and the spread over rounds. The pass's cost is an arm's time minus `rx`'s; `emit_over_rx` is that over `rx`.
Before timing, the forms' outputs, frames and dack tables are compared with each other byte for byte and with the closed
form of this batch (which frames trigger an ACK, and the ack number each carries). One JSON line per (connections,
shape) on stdout.

    python tools/tcp_ackemit_ab.py [--segments 1048576] [--conns 1,64,16384] [--shape inorder|strays|both] [--iters 10]
        [--reps 7] [--lane-max 4096] [--note TEXT] [--out profiles/tcp_ackemit_ab.jsonl]
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

PAYLOAD, WSCALE, BUFFER, SLOT = 100, 14, 0xFFFF << 14, 64


def run(a, nc, shape, lib, bid):
    import torch

    from demikernel_amd import _native as N
    from demikernel_amd import synth, tx_links
    from demikernel_amd.rx import RxResults
    from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table
    from demikernel_amd.tcp_ackemit import AckEmitResults, dack_conn_table, dack_to_device
    from demikernel_amd.tcp_tx import tx_conn_table

    dev = torch.device("cuda", 0)
    n = a.segments
    per = n // nc
    assert per * nc == n and per * PAYLOAD < BUFFER, "--segments must be a multiple of every --conns value"
    rng = np.random.default_rng(13)
    now = 100 * 10**9
    i = np.arange(n, dtype=np.int64)
    c_of, k = i % nc, i // nc  # round-robin arrival: segment k of connection c
    rn = rng.integers(0, 1 << 32, nc, dtype=np.int64)
    snd = rng.integers(0, 1 << 32, nc, dtype=np.int64)
    stray = (rng.random(n) < 0.05) if shape == "strays" else np.zeros(n, bool)
    s2 = stray.reshape(per, nc)
    rank = (np.cumsum(~s2, axis=0) - ~s2).reshape(n)  # in-order segments of the connection before this one
    seq = rn[c_of] + rank * PAYLOAD + np.where(stray, BUFFER + 12345, 0)
    # the closed form: a stray is acknowledged at once and clears the deadline; an in-order segment is acknowledged
    # when an odd number of them has arrived since (armed starts at 0); an ACK carries RCV.NXT after its segment
    kk = np.arange(per)[:, None]
    last = np.maximum.accumulate(np.where(s2, kk, -1), axis=0)
    want_ack = (s2 | ((kk - last) % 2 == 0)).reshape(n)
    want_no = (rn[c_of] + (rank + ~stray) * PAYLOAD) & 0xFFFFFFFF
    rx = RxResults(n, 1, device=dev, tcp_fields=True, counts=False)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v.astype(np.uint32)).view(np.int32)).to(dev)  # noqa: E731
    rx.t["meta"].copy_(up(np.full(n, N.V["OK_TCP"] | 6 << 8 | 0x18 << 16 | 0x50 << 24, np.int64)))
    rx.t["flow_id"].copy_(up(c_of))
    rx.t["payload"].copy_(up(np.full(n, 54 | PAYLOAD << 16, np.int64)))
    rx.t["tcp_seq"].copy_(up(seq & 0xFFFFFFFF))
    rx.t["tcp_ack"].copy_(up(snd[c_of]))
    t_rx = conn_table(nc, receive_next=rn, send_next=snd, buffer_size=BUFFER)
    u32 = lambda: rng.integers(0, 1 << 32, nc, dtype=np.uint64)  # noqa: E731
    t_tx = tx_conn_table(nc, snd_nxt=snd, rcv_wscale=WSCALE, local_ip=u32(), remote_ip=u32(), ports=u32())
    t_dk = dack_conn_table(nc)
    links = torch.from_numpy(np.ascontiguousarray(tx_links([(synth.BOB_MAC, synth.ALICE_MAC)])).view(np.uint8).copy()).to(dev)
    tcp = TcpReceiver(0)
    d_tx = torch.from_numpy(t_tx.view(np.uint8).copy()).to(dev)
    tab0 = [tcp.conns_to_device(t_rx), dack_to_device(t_dk)]
    tab = [t.clone() for t in tab0]
    out, res = TcpOut(n, nc), AckEmitResults(n, nc, n)
    d_out = torch.zeros(n * SLOT, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=0)
    sp = ctypes.c_void_p(stream.cuda_stream)
    r, o, ro = rx.c_struct(), out.c_struct(), res.c_struct()
    lay = N.DkTcpTxLayout(SLOT, 0)

    def restore():
        for t, t0 in zip(tab, tab0):
            t.copy_(t0, non_blocking=True)  # on `stream` (the timed loop runs under it)

    def rx_call():
        restore()
        assert lib.dk_tcp_rx_process(tcp._ctx, ctypes.byref(r), n, tab[0].data_ptr(), nc, ctypes.byref(o), sp) == 0

    def emit_call(form):
        rx_call()
        assert lib.dk_diag_tcp_ack_emit_set_form(tcp._ctx, form) == 0
        assert lib.dk_tcp_ack_emit(tcp._ctx, ctypes.byref(r), n, out.action.data_ptr(), out.view.data_ptr(),
                                   tab[0].data_ptr(), d_tx.data_ptr(), tab[1].data_ptr(), nc, links.data_ptr(), 1, now,
                                   d_out.data_ptr(), d_out.numel(), ctypes.byref(lay), n, 0, ctypes.byref(ro), sp) == 0

    calls = {"rx": rx_call, "rx_emit": lambda: emit_call(-1), "rx_emit_lane": lambda: emit_call(0),
             "rx_emit_scan": lambda: emit_call(1)}
    skipped = []
    if per > a.lane_max:
        skipped.append("rx_emit_lane")
        del calls["rx_emit_lane"]

    # the forms against each other and against this batch's closed form, before any timing
    seen = {}
    with torch.cuda.stream(stream):
        for name in [x for x in calls if x != "rx"]:
            d_out.zero_()
            calls[name]()
            torch.cuda.synchronize()
            h = res.to_numpy()
            seen[name] = (h, d_out[:h["n_frames"] * SLOT].cpu().numpy().copy(), tab[1].cpu().numpy().copy(),
                          lib.dk_diag_tcp_ack_emit_last_form(tcp._ctx))
    first = next(iter(seen.values()))
    same = all(all(np.array_equal(s[0][f], first[0][f]) for f in first[0]) and np.array_equal(s[1], first[1]) and
               np.array_equal(s[2], first[2]) for s in seen.values())
    h, frames = first[0], first[1].reshape(-1, SLOT)
    on_wire = (frames[:, 42].astype(np.int64) << 24 | frames[:, 43].astype(np.int64) << 16 |
               frames[:, 44].astype(np.int64) << 8 | frames[:, 45])
    closed = bool((h["status"] == 0).all() and h["n_frames"] == int(want_ack.sum()) and
                  np.array_equal(h["ack_frame"] != 0xFFFFFFFF, want_ack) and
                  np.array_equal(h["frame_seg"], np.nonzero(want_ack)[0]) and np.array_equal(on_wire, want_no[want_ack]))

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
    out_res = {name: {"us": round(float(np.median(ts)), 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)]}
               for name, ts in times.items()}
    base = out_res["rx"]["us"]
    for name in out_res:
        if name != "rx":
            out_res[name]["emit_us"] = round(out_res[name]["us"] - base, 2)
            out_res[name]["emit_over_rx"] = round((out_res[name]["us"] - base) / base, 4)
    line = json.dumps({"tool": "tcp_ackemit_ab", **({"note": a.note} if a.note else {}), "build": bid, "shape": shape,
                       "segments": n, "conns": nc, "per_conn": per, "acks": int(h["n_frames"]), "iters": a.iters,
                       "reps": a.reps, "rx_walk": tcp.last_walk,
                       "rule_form": {0: "lane", 1: "scan"}.get(seen["rx_emit"][3]), "forms_byte_identical": bool(same),
                       "matches_closed_form": closed, "skipped": skipped, **out_res})
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
    ap.add_argument("--shape", choices=["inorder", "strays", "both"], default="both")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lane-max", type=int, default=4096, help="segments per connection above which the lane arm is skipped")
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
        for shape in (["inorder", "strays"] if a.shape == "both" else [a.shape]):
            ok = run(a, nc, shape, lib, bid) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
