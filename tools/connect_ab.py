#!/usr/bin/env python3
"""dk_tcp_connect_process on a storm of answers, and dk_tcp_connect_start on a storm of connect() calls, beside the
dk_rx_process call on the same batch, in one process on one stream.

1,048,576 connecting sockets (rows), 60-byte answers in 64-byte slots. One answer per row, in three mixes, and two shapes with several per row:
  accepted  every frame is the SYN+ACK that acknowledges its row's ISN: n handshake ACKs, n ready records
  refused   every frame is a RST+ACK with the right ack: n error records, no frame
  eagain    every frame is a stray ACK: n resent SYNs
  pairs     n / 2 rows get a stray ACK and, later in the batch, their SYN+ACK: the rows with two ranked frames, which a
            count and a minimum still settle
  triples   n / 3 rows get two stray ACKs and then their SYN+ACK: every frame goes through the serial rank walk, the
            pass's worst case
and `start`: dk_tcp_connect_start of the n rows (n ISNs, n SYNs).
There is no parent implementation to compare with and the Python model is not a baseline: the calls are stated relative
to the receive kernel, which reads the same frames. A call changes the rows, so every timed call starts from the same
state: the rows (and the generator) are restored, untimed, before it, and HIP events bracket the one call. Arms
alternate (rx, connect, rx_again: the difference of the two rx arms is the A/A noise floor) for `--reps` rounds after an
untimed preheat; median µs and the spread over rounds. Before timing, the call's words, statuses and actions are
checked. One JSON line per shape on stdout. --once runs every shape's call once after the preheat, for a
`rocprofv3 --kernel-trace --stats` run of its own (the split per launch).

    python tools/connect_ab.py [--rows 1048576] [--reps 7] [--once] [--out profiles/connect_ab.jsonl]
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
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as G
    from demikernel_amd import Config, RxEngine, ipv4, synth, tx_links
    from demikernel_amd import _native as N
    from demikernel_amd import tcp_connect as TC

    assert torch.cuda.is_available(), "needs a GPU"
    bid = G.check_loaded_build()
    dev = torch.device("cuda", 0)
    n, now = a.rows, 5 * 10**9
    lip = ipv4(synth.BOB_IPV4)
    i = np.arange(n, dtype=np.uint64)
    rip = (10 | ((i >> 16) & 0xFF) << 8 | ((i >> 8) & 0xFF) << 16 | (1 + (i & 0xFF) % 250) << 24).astype(np.uint32)
    rport = (1024 + (i * 7) % 60000).astype(np.uint16)
    lport = (1024 + i % 64000).astype(np.uint16)
    flows = np.zeros(n, N.FLOW_DTYPE)
    flows["kind"], flows["local_ip"], flows["remote_ip"] = N.DK_FLOW_TCP_ACTIVE, lip, rip
    flows["local_port"], flows["remote_port"] = lport, rport
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    eng.set_sockets(flows)
    d_links = TC.to_device(tx_links([(synth.BOB_MAC, synth.ALICE_MAC)]))
    rows = TC.connector_table(n, flow_id=np.arange(n), local_ip=lip, local_port=lport, remote_ip=rip, remote_port=rport)
    d_map = TC.to_device(TC.conn_of_flow(n, rows))
    d_idle, d_gen0 = TC.to_device(rows), TC.to_device(TC.isn_gen(0xC0FFEE, 0))
    d_rows, d_gen = d_idle.clone(), d_gen0.clone()
    d_start = TC.to_device(np.arange(n, dtype=np.uint32))
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(5)

    def batch_of(flags, seq, ack, idx=None):
        """One frame per entry of idx (the row it is for; every row once by default)."""
        idx = np.arange(n, dtype=np.int64) if idx is None else idx
        k = len(idx)
        tr = synth.Traffic(ip_len=np.full(k, 40, np.uint16), frame_len=np.full(k, 60, np.uint16),
                           proto=np.full(k, 6, np.uint8), src_ip=rip[idx], dst_ip=np.full(k, lip, np.uint32),
                           sport=rport[idx], dport=lport[idx], seq=np.broadcast_to(seq, k).astype(np.uint32),
                           ack=np.broadcast_to(ack, k).astype(np.uint32),
                           flags=np.broadcast_to(np.asarray(flags), k).astype(np.uint8),
                           window=np.full(k, 65535, np.uint16), ip_id=np.zeros(k, np.uint16), ttl=np.full(k, 64, np.uint8),
                           flow=idx)
        return synth.build_device(tr, eng)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0

    def run(name, batch, call, restore, res, check):
        rx = eng.results(batch.n, tcp_fields=True, tcp_opts=True)

        def receive():
            eng.receive_batch(batch, rx)

        def connect():
            call(rx)

        restore()
        receive()
        connect()  # the preheat, and the check
        torch.cuda.synchronize()
        got = res.to_numpy()
        hist = check(got)
        if a.once:
            restore()
            receive()
            connect()
            torch.cuda.synchronize()
            return
        t = {"rx": [], "connect": [], "rx_again": []}
        for _ in range(a.reps):
            for k, fn in (("rx", receive), ("connect", connect), ("rx_again", receive)):
                if k == "connect":
                    restore()
                t[k].append(timed(fn))
        rec = {"tool": "connect_ab", "build": bid, "shape": name, "frames": batch.n, "rows": n, "actions": hist,
               "n_frames": got["n_frames"], "n_ready": got["n_ready"], "reps": a.reps, "note": a.note}
        for k, v in t.items():
            rec[k] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(min(v)), 1),
                      "max_us": round(float(max(v)), 1)}
        rec["connect_over_rx"] = round(rec["connect"]["median_us"] / rec["rx"]["median_us"], 2)
        rec["aa_noise_us"] = round(abs(rec["rx"]["median_us"] - rec["rx_again"]["median_us"]), 1)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    # start: n ISNs and n SYNs; the rows it leaves are the state every process shape starts from
    sres = TC.ConnectResults(4, n, n, n)

    def start_call(_rx):
        TC.connect_start(d_rows, d_start, d_gen, d_links, now, d_out, sres, slot_stride=64)

    def start_restore():
        d_rows.copy_(d_idle)
        d_gen.copy_(d_gen0)
        torch.cuda.synchronize()

    def start_check(got):
        assert (got["status"] == TC.OK).all(), np.bincount(got["status"])
        assert (got["n_frames"], got["n_ready"]) == (n, 0)
        return {"SYN": n}

    seq = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    run("start", batch_of(0x10, seq, np.zeros(n)), start_call, start_restore, sres, start_check)
    start_restore()
    start_call(None)
    torch.cuda.synchronize()
    d_connecting = d_rows.clone()
    isn = TC.rows_to_host(d_rows)["local_isn"].astype(np.uint64)
    pres = TC.ConnectResults(n, n, n, n)

    def process_call(rx):
        TC.connect_process(rx, d_rows, d_map, d_links, now + 1000, d_out, pres, slot_stride=64)

    def process_restore():
        d_rows.copy_(d_connecting)
        torch.cuda.synchronize()

    def process_check(want, nf, nr):
        def check(got):
            assert (got["status"] == TC.OK).all(), np.bincount(got["status"])
            acts = got["action"][:sum(want.values())]  # the batch's frames
            hist = {TC.ACTIONS[k]: int(c) for k, c in enumerate(np.bincount(acts, minlength=7)) if c}
            assert hist == want and (got["n_frames"], got["n_ready"]) == (nf, nr), (hist, got["n_frames"], got["n_ready"])
            return hist
        return check

    for name, flags, ack, want, nf, nr in (("accepted", 0x12, isn + 1, "ESTABLISHED", n, n),
                                           ("refused", 0x14, isn + 1, "REFUSED", 0, n),
                                           ("eagain", 0x10, isn + 2, "RETRY_SYN", n, 0)):
        run(name, batch_of(flags, seq, ack & 0xFFFFFFFF), process_call, process_restore, pres,
            process_check({want: n}, nf, nr))
    for name, per in (("pairs", 2), ("triples", 3)):  # several frames a row, a row's frames n / per apart
        nr = n // per
        idx = np.tile(np.arange(nr, dtype=np.int64), per)
        last = np.arange(nr * per) >= nr * (per - 1)  # the row's SYN+ACK, behind its strays
        run(name, batch_of(np.where(last, 0x12, 0x10), seq[idx], (isn[idx] + np.where(last, 1, 2).astype(np.uint64)) & 0xFFFFFFFF, idx),
            process_call, process_restore, pres, process_check({"ESTABLISHED": nr, "RETRY_SYN": nr * (per - 1)}, nr * per, nr))
    eng.close()


if __name__ == "__main__":
    main()
