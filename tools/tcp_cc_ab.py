#!/usr/bin/env python3
"""Cost of the congestion-control calls beside the calls they stand next to, in one process on one stream.

  cc_ack / ack_lane   dk_tcp_cc_ack against dk_tcp_ack_process's lane form on the same `--segs`-segment batch of pure
                      ACKs over `--conns` connections (default: 16,384, 64 and 1 connections in turn). Each timed
                      iteration is dk_tcp_rx_process, then the call; the dk_tcp_rx_process call alone is timed too and
                      subtracted. The tables are restored before every iteration (device copies, inside the timing of
                      all three arms alike).
  timers / rtx_sparse dk_tcp_timers over `--table` connections (none due) against dk_tcp_retransmit with one connection
                      in `--sparse` firing.

Timing: HIP events around `--iters` iterations, `--reps` rounds alternating the arms after an untimed preheat; median
µs per call and the spread over rounds. One JSON line per shape on stdout.

    python tools/tcp_cc_ab.py [--segs 1048576] [--conns 16384,64,1] [--table 65536] [--sparse 256] [--iters 5]
        [--reps 5] [--out profiles/tcp_cc_ab.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segs", type=int, default=1 << 20)
    ap.add_argument("--conns", default="16384,64,1")
    ap.add_argument("--table", type=int, default=65536)
    ap.add_argument("--sparse", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as G
    from demikernel_amd import _native as N
    from demikernel_amd import synth, tx_links
    from demikernel_amd.rx import RxResults
    from demikernel_amd.tcp import TcpOut, TcpReceiver, conn_table
    from demikernel_amd.tcp_ack import TcpAcker, TcpAckOut, UnackedQueue, ack_conn_table
    from demikernel_amd.tcp_cc import CcAckOut, TimersOut, cc_ack, cc_conn_table, cc_to_device, timers
    from demikernel_amd.tcp_rtx import RtxResults, fire_to_device, retransmit
    from demikernel_amd.tcp_tx import TcpSender, tx_conn_table

    assert torch.cuda.is_available(), "needs a GPU"
    bid = G.check_loaded_build()
    dev = torch.device("cuda", 0)
    lines = []

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / iters

    def run(arms, iters):
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                t[k].append(timed(fn, iters))
        return {k: {"median_us": round(float(np.median(v)), 2), "min_us": round(float(min(v)), 2),
                    "max_us": round(float(max(v)), 2)} for k, v in t.items()}

    n, mss = a.segs, 1000
    for nc in (int(v) for v in a.conns.split(",")):
        rng = np.random.default_rng(nc)
        per = n // nc
        una = rng.integers(0, 1 << 32, nc, dtype=np.uint64).astype(np.uint32)
        flight = min(per * 100, 1 << 30)
        conn = np.tile(np.arange(nc, dtype=np.uint32), per)  # connections interleaved, each in order
        k = np.repeat(np.arange(per, dtype=np.uint64), nc)
        rx = {"meta": np.full(n, N.V["OK_TCP"] | 6 << 8 | 0x10 << 16 | 0x50 << 24, np.uint32), "flow_id": conn,
              "tcp_seq": np.full(n, 5000, np.uint32), "payload": np.full(n, 54, np.uint32),
              # rising ACKs with every fourth a duplicate of the one before
              "tcp_ack": (una[conn] + ((k - (k % 4 == 3)) * 100 % flight).astype(np.uint32))}
        r = RxResults(n, 1, device=dev, tcp_fields=True, counts=False)
        for key, v in rx.items():
            r.t[key].copy_(torch.from_numpy(np.ascontiguousarray(v, np.uint32).view(np.int32)))
        tcp = TcpReceiver(0)
        table = conn_table(nc, receive_next=5000, send_next=una + np.uint32(flight))
        tx = tx_conn_table(nc, snd_nxt=una + np.uint32(flight), snd_una=una, mss=mss, snd_wnd=1 << 20)
        ak = ack_conn_table(nc, wl1=4000, wl2=una - np.uint32(5), q_first=np.arange(nc), q_count=1)
        cc = cc_conn_table(nc, mss=mss, seq_no=una, now_ns=10**9)
        cc["ssthresh"], cc["w_max"] = 8 * mss, 20 * mss  # slow start for four segments, then congestion avoidance
        up = lambda t: torch.from_numpy(np.ascontiguousarray(t).view(np.uint8).copy()).to(dev)  # noqa: E731
        saved = [up(table), up(tx), up(ak), up(cc)]
        d_rx, d_tx, d_ak, d_cc = (s.clone() for s in saved)
        queue = UnackedQueue.from_numpy(np.zeros(nc), np.full(nc, flight), np.full(nc, N.DK_TCP_TX_TIME_NONE, np.uint64))
        qlen = queue.len.clone()
        out, aout, cout = TcpOut(n, nc), TcpAckOut(n, nc), CcAckOut(n, nc)
        acker = TcpAcker("lane")

        def reset():
            for d, s in zip((d_rx, d_tx, d_ak, d_cc), saved):
                d.copy_(s)
            queue.len.copy_(qlen)
            tcp.process(r, d_rx, out)

        def arm_cc():
            reset()
            cc_ack(tcp, r, out, d_rx, d_tx, d_ak, d_cc, 3 * 10**9, cout)

        def arm_ack():
            reset()
            acker.process(tcp, r, out, d_rx, d_tx, d_ak, queue, 3 * 10**9, aout)

        res = run({"rx_process": reset, "rx_then_cc_ack": arm_cc, "rx_then_ack_lane": arm_ack}, a.iters)
        torch.cuda.synchronize()
        st, sa = cout.to_numpy(), aout.to_numpy()
        assert (st["status"] == 0).all() and (sa["status"] == 0).all(), (st["status"][:4], sa["status"][:4])
        rec = {"tool": "tcp_cc_ab", "build": bid, "segs": n, "conns": nc, "iters": a.iters, "reps": a.reps,
               "note": a.note, **res}
        for k2 in ("rx_then_cc_ack", "rx_then_ack_lane"):
            rec[k2.replace("rx_then_", "") + "_alone_us"] = round(res[k2]["median_us"] - res["rx_process"]["median_us"], 2)
        lines.append(rec)
        tcp.close()

    nt = a.table
    rng = np.random.default_rng(2)
    u32 = lambda: rng.integers(0, 1 << 32, nt, dtype=np.uint64)  # noqa: E731
    sender = TcpSender(0)
    tx = tx_conn_table(nt, snd_nxt=u32(), snd_wnd=1 << 30, mss=1460, rcv_nxt=u32(), local_ip=u32(), remote_ip=u32(),
                       ports=u32(), ip_word=rng.integers(0, 65536, nt) | 64 << 16)
    ak = ack_conn_table(nt, q_first=np.arange(nt), q_count=1)
    ak["rtx_armed"], ak["rtx_base_ns"] = 1, 10**9
    d_tx, d_ak = sender.conns_to_device(tx), TcpAcker.conns_to_device(ak)
    d_cc = cc_to_device(cc_conn_table(nt, mss=1460))
    queue = UnackedQueue.from_numpy(np.arange(nt, dtype=np.uint32) * 1460, np.full(nt, 1460, np.uint32), np.zeros(nt, np.uint64))
    d_src = torch.randint(0, 256, (nt * 1460,), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((nt // a.sparse + 1) * 1536, dtype=torch.uint8, device=dev)
    d_links = torch.from_numpy(np.ascontiguousarray(tx_links([(synth.BOB_MAC, synth.ALICE_MAC)])).view(np.uint8).copy()).to(dev)
    sp = np.zeros(nt, np.uint8)
    sp[::a.sparse] = 2
    fire, rres, tout = fire_to_device(sp), RtxResults(nt // a.sparse + 1, nt), TimersOut(nt, ack_fire=False)
    res = run({"timers": lambda: timers(sender, d_tx, d_ak, d_cc, 10**9 + 5, tout),  # rto 1 s: none is due
               "rtx_sparse": lambda: retransmit(sender, d_src, fire, d_tx, d_ak, queue, 1000, d_links, d_out, rres,
                                                slot_stride=1536)}, max(a.iters, 20))
    torch.cuda.synchronize()
    g = tout.to_numpy()
    assert g["n_fast"] == g["n_timeout"] == 0 and (g["status"] == 0).all()
    lines.append({"tool": "tcp_cc_ab", "build": bid, "table": nt, "sparse_frames": int((sp != 0).sum()), "note": a.note, **res})
    sender.close()
    for rec in lines:
        line = json.dumps(rec)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
