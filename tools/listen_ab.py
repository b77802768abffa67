#!/usr/bin/env python3
"""dk_tcp_listen_process on a connection storm, beside the dk_rx_process call it follows on the same batch, in one
process on one stream.

1,048,576 frames in 64-byte slots for 1,024 listeners, every frame from a remote of its own, in three shapes:
  accept     every frame is a SYN and every listener has room: n inserts, n SYN+ACKs
  refuse     the same SYNs with every backlog full: n RSTs, nothing changes
  handshake  half the frames are the handshake ACKs of entries made before (n / 2 ready records), the other half new
             SYNs, interleaved
There is no parent implementation to compare with and the Python model is not a baseline: the pass is stated relative to
the receive kernel, which reads the same frames. A call changes the table and the listeners, so every timed call starts
from the same state: the table and the listener rows are restored (untimed) before it, and HIP events bracket the one
call. Arms alternate (rx, listen, rx_again: the difference of the two rx arms is the A/A noise floor) for `--reps` rounds
after an untimed preheat; median µs and the spread over rounds. Before timing, the call's words, statuses and the
listeners' inflight are checked. One JSON line per shape on stdout. --once runs every shape's call once after the
preheat, for a `rocprofv3 --kernel-trace --stats` run of its own (the split per launch).

    python tools/listen_ab.py [--frames 1048576] [--listeners 1024] [--reps 7] [--once] [--out profiles/listen_ab.jsonl]
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
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--listeners", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as G
    from demikernel_amd import Config, RxEngine, SocketId, flow_array, ipv4, synth, tx_links
    from demikernel_amd import tcp_listen as TL

    assert torch.cuda.is_available(), "needs a GPU"
    bid = G.check_loaded_build()
    dev = torch.device("cuda", 0)
    n, nl, now = a.frames, a.listeners, 5 * 10**9
    assert n % (2 * nl) == 0
    per = n // nl
    cap = 1
    while cap < 2 * n:
        cap <<= 1
    ports = 1024 + np.arange(nl)
    flows = flow_array([SocketId.Passive((synth.BOB_IPV4, int(p))) for p in ports])
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    eng.set_sockets(flows)
    d_links = TL.to_device(tx_links([(synth.BOB_MAC, synth.ALICE_MAC)]))
    d_lsn = TL.to_device(np.arange(nl, dtype=np.uint32))
    rng = np.random.default_rng(5)

    def batch_of(src_ip, sport, lidx, flags, seq, ack):
        k = len(src_ip)
        tr = synth.Traffic(ip_len=np.full(k, 40, np.uint16), frame_len=np.full(k, 60, np.uint16),
                           proto=np.full(k, 6, np.uint8), src_ip=src_ip.astype(np.uint32),
                           dst_ip=np.full(k, ipv4(synth.BOB_IPV4), np.uint32), sport=sport.astype(np.uint16),
                           dport=ports[lidx].astype(np.uint16), seq=seq.astype(np.uint32), ack=ack.astype(np.uint32),
                           flags=flags.astype(np.uint8), window=np.full(k, 65535, np.uint16),
                           ip_id=np.zeros(k, np.uint16), ttl=np.full(k, 64, np.uint8), flow=lidx.astype(np.int64))
        return synth.build_device(tr, eng)

    def remotes(first, k):
        i = first + np.arange(k, dtype=np.uint64)
        ip = (10 | ((i >> 16) & 0xFF) << 8 | ((i >> 8) & 0xFF) << 16 | (1 + (i & 0xFF) % 250) << 24).astype(np.uint32)
        return ip, (1024 + (i * 7) % 60000).astype(np.uint16)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0

    def shape(name, batch, listeners, table, expect):
        rows0 = table.rows()
        d_L = TL.to_device(listeners)
        saved_L = d_L.clone()
        rx = eng.results(batch.n, tcp_fields=True, tcp_opts=True)
        d_out = torch.zeros(batch.n * 64, dtype=torch.uint8, device=dev)
        res = TL.ListenResults(batch.n, batch.n, batch.n, nl)
        bsum = int(listeners["max_backlog"].astype(np.uint64).sum())

        def restore():
            table.write(rows0)
            d_L.copy_(saved_L)
            torch.cuda.synchronize()

        def receive():
            eng.receive_batch(batch, rx)

        def listen():
            TL.listen_process(table, rx, d_L, d_lsn, d_links, now, d_out, res, slot_stride=64, backlog_sum=bsum)

        receive()
        listen()  # the preheat, and the check
        torch.cuda.synchronize()
        got = res.to_numpy()
        assert (got["status"] == TL.OK).all(), np.bincount(got["status"])
        assert (got["n_frames"], got["n_ready"]) == expect[:2], (got["n_frames"], got["n_ready"], expect)
        assert int(TL.listeners_to_host(d_L)["inflight"].astype(np.int64).sum()) == expect[2]
        hist = {TL.ACTIONS[k]: int(c) for k, c in enumerate(np.bincount(got["action"], minlength=9)) if c}
        if a.once:
            restore()
            receive()
            listen()
            torch.cuda.synchronize()
            return
        t = {"rx": [], "listen": [], "rx_again": []}
        for _ in range(a.reps):
            for k, fn in (("rx", receive), ("listen", listen), ("rx_again", receive)):
                if k == "listen":
                    restore()
                t[k].append(timed(fn))
        rec = {"tool": "listen_ab", "build": bid, "shape": name, "frames": batch.n, "listeners": nl, "cap": cap,
               "actions": hist, "n_frames": got["n_frames"], "n_ready": got["n_ready"], "reps": a.reps, "note": a.note}
        for k, v in t.items():
            rec[k] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(min(v)), 1),
                      "max_us": round(float(max(v)), 1)}
        rec["listen_over_rx"] = round(rec["listen"]["median_us"] / rec["rx"]["median_us"], 2)
        rec["aa_noise_us"] = round(abs(rec["rx"]["median_us"] - rec["rx_again"]["median_us"]), 1)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    lidx = (np.arange(n) % nl).astype(np.int64)  # the listeners' frames interleave
    ip, port = remotes(0, n)
    syn, seq = np.full(n, 0x02), rng.integers(0, 1 << 32, n, dtype=np.uint64)
    syns = batch_of(ip, port, lidx, syn, seq, np.zeros(n))
    L = TL.listener_table(nl, flow_id=np.arange(nl), local_ip=ipv4(synth.BOB_IPV4), local_port=ports, max_backlog=per,
                          nonce=rng.integers(0, 1 << 32, nl, dtype=np.uint64))
    table = TL.ListenTable(cap)
    empty = table.rows()
    shape("accept", syns, L, table, (n, 0, n))
    full = L.copy()
    full["inflight"] = full["max_backlog"]
    table.write(empty)
    shape("refuse", syns, full, table, (n, 0, n))
    table.write(empty)
    # handshake: entries for the first half of the remotes, made by the device; their ACKs from the table's own rows
    h = n // 2
    first = batch_of(ip[:h], port[:h], lidx[:h], syn[:h], seq[:h], np.zeros(h))
    d_L = TL.to_device(L)
    rx = eng.results(h, tcp_fields=True, tcp_opts=True)
    eng.receive_batch(first, rx)
    res = TL.ListenResults(h, h, h, nl)
    TL.listen_process(table, rx, d_L, d_lsn, d_links, now, torch.zeros(h * 64, dtype=torch.uint8, device=dev), res,
                      slot_stride=64, backlog_sum=n)
    torch.cuda.synchronize()
    rows = table.rows()
    live = rows[rows["state"] == TL.SYN_RCVD]
    assert len(live) == h
    order = rng.permutation(n)
    k_l = (live["key"] >> np.uint64(48)).astype(np.int64)
    k_ip = ((live["key"] >> np.uint64(16)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    k_port = (live["key"] & np.uint64(0xFFFF)).astype(np.uint16)
    m_ip, m_port = np.concatenate([k_ip, ip[h:]]), np.concatenate([k_port, port[h:]])
    m_l = np.concatenate([k_l, lidx[h:]])
    m_flags = np.concatenate([np.full(h, 0x10), syn[h:]])
    m_seq = np.concatenate([live["remote_isn"].astype(np.uint64) + 1, seq[h:]])
    m_ack = np.concatenate([live["local_isn"].astype(np.uint64) + 1, np.zeros(n - h, np.uint64)])
    mixed = batch_of(m_ip[order], m_port[order], m_l[order], m_flags[order], m_seq[order] & 0xFFFFFFFF,
                     m_ack[order] & 0xFFFFFFFF)
    shape("handshake", mixed, TL.listeners_to_host(d_L), table, (n - h, h, n))
    table.close()
    eng.close()


if __name__ == "__main__":
    main()
