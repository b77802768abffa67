#!/usr/bin/env python3
"""Interleaved A/B of dk_tcp_retransmit against dk_tcp_tx_segment emitting the same frames, in one process on one
stream: `--conns` connections, each with one `--bytes`-byte entry at the front of its unacknowledged queue.

  rtx_dense    dk_tcp_retransmit, every connection firing (TIMEOUT): --conns frames
  segment      dk_tcp_tx_segment cutting one --bytes buffer per connection at mss = --bytes: the same payload through
               the same copy into the same slots, the yardstick
  rtx_sparse   dk_tcp_retransmit with one connection in --sparse firing (FAST): plan, scan and commit over the whole
               table, a few hundred frames

Before timing, the first dense call's frames are compared with the first segment call's byte for byte (SND.UNA equals
SND.NXT at that point, so the two calls must build the same frames). Timing: HIP events around `--iters` calls,
`--reps` rounds alternating the arms after an untimed preheat; median µs per call and the spread over rounds. One JSON
line on stdout.

    python tools/tcp_rtx_ab.py [--conns 65536] [--bytes 1460] [--sparse 256] [--iters 20] [--reps 9] [--note TEXT]
        [--out profiles/tcp_rtx_ab.jsonl]
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
    ap.add_argument("--conns", type=int, default=65536)
    ap.add_argument("--bytes", type=int, default=1460)
    ap.add_argument("--sparse", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--stride", type=int, default=1536)
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as G
    from demikernel_amd import synth, tx_links
    from demikernel_amd.tcp_ack import TcpAcker, UnackedQueue, ack_conn_table
    from demikernel_amd.tcp_rtx import RtxResults, fire_to_device, retransmit
    from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults, tx_conn_table

    assert torch.cuda.is_available(), "needs a GPU"
    bid = G.check_loaded_build()
    n, L, stride = a.conns, a.bytes, a.stride
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    u32 = lambda: rng.integers(0, 1 << 32, n, dtype=np.uint64)  # noqa: E731
    tx = tx_conn_table(n, snd_nxt=u32(), snd_wnd=1 << 30, mss=L, rcv_nxt=u32(), local_ip=u32(), remote_ip=u32(),
                       ports=u32(), ip_word=rng.integers(0, 65536, n) | 64 << 16)
    ak = ack_conn_table(n, q_first=np.arange(n), q_count=1)
    ak["rtx_armed"] = 1
    off = np.arange(n, dtype=np.uint32) * L
    sender = TcpSender(0)
    d_src = torch.randint(0, 256, (n * L,), dtype=torch.uint8, device=dev)
    d_out, d_out2 = (torch.zeros(n * stride, dtype=torch.uint8, device=dev) for _ in range(2))
    links = tx_links([(synth.BOB_MAC, synth.ALICE_MAC)])
    d_links = torch.from_numpy(np.ascontiguousarray(links).view(np.uint8).copy()).to(dev)
    d_tx, d_tx_seg, d_ak = sender.conns_to_device(tx), sender.conns_to_device(tx), TcpAcker.conns_to_device(ak)
    queue = UnackedQueue.from_numpy(off, np.full(n, L, np.uint32), np.zeros(n, np.uint64))
    dense = fire_to_device(np.full(n, 1, np.uint8))
    sp = np.zeros(n, np.uint8)
    sp[::a.sparse] = 2
    sparse = fire_to_device(sp)
    rres, sres = RtxResults(n, n), TcpTxResults(n, n)
    push = PushList.from_numpy(np.arange(n), off, np.full(n, L))
    word = lambda t: int(t.cpu().numpy().view(np.uint32)[0])  # noqa: E731

    def rtx(fire, out=d_out):
        retransmit(sender, d_src, fire, d_tx, d_ak, queue, 1000, d_links, out, rres, slot_stride=stride)

    def seg(out=d_out):
        sender.segment(d_src, push, d_tx_seg, d_links, out, sres, slot_stride=stride)

    # the two paths build the same frames
    rtx(dense, d_out)
    seg(d_out2)
    torch.cuda.synchronize()
    assert word(rres.n_frames) == n == word(sres.n_frames)
    assert torch.equal(d_out, d_out2), "dk_tcp_retransmit's frames differ from dk_tcp_tx_segment's"
    assert torch.equal(rres.off_out, sres.off_out) and torch.equal(rres.len_out, sres.len_out)
    rtx(sparse)
    torch.cuda.synchronize()
    assert word(rres.n_frames) == int((sp != 0).sum())

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.iters  # µs per call

    arms = {"rtx_dense": lambda: rtx(dense), "segment": seg, "rtx_sparse": lambda: rtx(sparse)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, fn in arms.items():
            t[k].append(timed(fn))
    rec = {"tool": "tcp_rtx_ab", "build": bid, "conns": n, "bytes": L, "stride": stride,
           "sparse_frames": int((sp != 0).sum()), "iters": a.iters, "reps": a.reps, "note": a.note}
    for k, v in t.items():
        v = np.array(v)
        rec[k] = {"median_us": round(float(np.median(v)), 2), "min_us": round(float(v.min()), 2),
                  "max_us": round(float(v.max()), 2)}
    ratios = np.array(t["rtx_dense"]) / np.array(t["segment"])
    rec["dense_over_segment"] = {"median": round(float(np.median(ratios)), 4), "min": round(float(ratios.min()), 4),
                                 "max": round(float(ratios.max()), 4)}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sender.close()


if __name__ == "__main__":
    main()
