#!/usr/bin/env python3
"""dk_tcp_tx_commit (each form forced, and the engine's rule) against UnackedQueue.append_frames, the torch code it
replaces, on the same dk_tcp_tx_segment outputs, in one process on one stream.

A commit takes its turn after a segmentation call, so every timed iteration is: restore the TX and ACK tables (device
copies), dk_tcp_tx_segment, then the arm's call; the first two alone are an arm of their own ("segment") and are
subtracted. append_frames is given the frame count as a host constant, which spares it the read-back a caller would
need. The rule's arm runs twice ("rule", "rule_again"): the difference of the two is the A/A noise floor of the
measurement. Shapes (connections x frames per connection x q_cap), each once with room behind the live entries
("in_place": q_count = frames / 2 at the region's start) and once with the live range ending at the region's end
("compact": the same entries have to move first). mss = 8, one buffer per connection.

Timing: HIP events around `--iters` iterations, `--reps` rounds alternating the arms after an untimed preheat; median
µs per iteration and the spread over rounds. Before timing, every arm's queue is compared with append_frames' on the
host (the live entries, q_count, rtx_armed, rtx_base_ns). One JSON line per shape and mode on stdout.

    python tools/commit_ab.py [--shapes 4096x16x64,256x1024x2048,1x65536x131072] [--iters 20] [--reps 7]
        [--out profiles/commit_ab.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MSS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x16x64,256x1024x2048,1x65536x131072")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as G
    from demikernel_amd import synth, tx_links
    from demikernel_amd.tcp_ack import TcpAcker, UnackedQueue, ack_conn_table
    from demikernel_amd.tcp_commit import CommitOut, last_form, tx_commit
    from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults, tx_conn_table

    assert torch.cuda.is_available(), "needs a GPU"
    bid = G.check_loaded_build()
    dev = torch.device("cuda", 0)
    now = 5 * 10**9

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

    sender = TcpSender(0)
    d_links = torch.from_numpy(np.ascontiguousarray(tx_links([(synth.BOB_MAC, synth.ALICE_MAC)])).view(np.uint8).copy()).to(dev)
    for shape in a.shapes.split(","):
        nc, fpc, q_cap = (int(v) for v in shape.split("x"))
        n = nc * fpc
        assert fpc % 2 == 0 and fpc // 2 + fpc <= q_cap and n * 64 < 1 << 31
        stride = 64
        d_src = torch.randint(0, 256, (n * MSS,), dtype=torch.uint8, device=dev)
        d_out = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        push = PushList.from_numpy(np.arange(nc), np.arange(nc, dtype=np.int64) * fpc * MSS, np.full(nc, fpc * MSS))
        res = TcpTxResults(n, nc)
        tx = tx_conn_table(nc, snd_nxt=np.arange(nc, dtype=np.int64) * 99_991, snd_wnd=1 << 30, mss=MSS)
        saved_tx = sender.conns_to_device(tx)
        d_tx = saved_tx.clone()
        rng = np.random.default_rng(nc)
        for mode in ("in_place", "compact"):
            r0 = np.arange(nc, dtype=np.int64) * q_cap
            live = fpc // 2
            ak = ack_conn_table(nc, q_first=r0 if mode == "in_place" else r0 + q_cap - live, q_count=live)
            saved_ak = TcpAcker.conns_to_device(ak)
            d_ak = saved_ak.clone()
            pool = [rng.integers(0, 1 << 31, nc * q_cap).astype(np.uint32), rng.integers(0, 1 << 16, nc * q_cap).astype(np.uint32),
                    rng.integers(0, 1 << 40, nc * q_cap).astype(np.uint64)]

            def fresh_queue():
                q = UnackedQueue.from_numpy(*pool)
                q.nconns, q.capacity, q.nq = nc, q_cap, nc * q_cap
                return q

            queue, cout = fresh_queue(), CommitOut(nc)

            def segment():
                d_tx.copy_(saved_tx)
                d_ak.copy_(saved_ak)
                sender.segment(d_src, push, d_tx, d_links, d_out, res, slot_stride=stride)

            def commit(form):
                def arm():
                    segment()
                    tx_commit(sender, push, res, d_ak, queue, now, cout, form=form)
                return arm

            def append():
                segment()
                queue.append_frames(d_ak, res, push, now, n)

            # results first: every arm on a fresh pool, its live queues against append_frames'
            def live_queues():
                torch.cuda.synchronize()
                t, p = TcpAcker.conns_to_host(d_ak), queue.to_numpy()
                qf, qc = t["q_first"].astype(np.int64), t["q_count"].astype(np.int64)
                at = (qf[:, None] + np.arange(live + fpc)[None, :]).reshape(-1)
                assert (qc == live + fpc).all(), qc[:4]
                return [p[k][at].tobytes() for k in ("off", "len", "tx_time")] + [t[k].tobytes() for k in ("q_count", "rtx_armed", "rtx_base_ns")]

            append()
            want = live_queues()
            forms = {}
            for form in ("conn", "chip", None):
                queue = fresh_queue()
                commit(form)()
                assert live_queues() == want, f"{shape} {mode}: the {form} form's queues are not append_frames'"
                assert not cout.to_numpy()["status"].any()
                forms[form or "rule"] = last_form(sender)
            assert int(res.n_frames.cpu().numpy().view(np.uint32)[0]) == n
            queue = fresh_queue()
            t = run({"segment": segment, "conn": commit("conn"), "chip": commit("chip"), "rule": commit(None),
                     "append_frames": append, "rule_again": commit(None)}, a.iters)
            rec = {"tool": "commit_ab", "build": bid, "conns": nc, "frames_per_conn": fpc, "q_cap": q_cap, "mode": mode,
                   "rule_form": forms["rule"], "iters": a.iters, "reps": a.reps, "note": a.note, **t}
            for k in ("conn", "chip", "rule", "rule_again", "append_frames"):
                rec[k + "_alone_us"] = round(t[k]["median_us"] - t["segment"]["median_us"], 2)
            rec["aa_noise_us"] = round(abs(t["rule"]["median_us"] - t["rule_again"]["median_us"]), 2)
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    sender.close()


if __name__ == "__main__":
    main()
