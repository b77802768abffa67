#!/usr/bin/env python3
"""Interleaved A/B of the two TX entry points on one blob in one process: dk_tx_checksum (the in-place checksum fill
over already-built frames: the yardstick) and dk_tx_serialize (every header byte built from descriptors). The batch is
C2's: `--frames` x 1500-byte TCP frames in 64-byte aligned slots, built on the device; the serialize descriptors are the
same frames' fields, so both calls leave the blob as it was (checked at the end, with every header byte wiped first).

Both arms are the bare C entry points through ctypes with every argument prepared beforehand and the outputs
preallocated: between the two events each arm queues its one kernel per iteration and nothing else (no allocation, no
fill), so the figure is the kernel's launch-to-launch time, not a wrapper's.
Timing: HIP events on the launch stream around `--iters` launches, `--reps` rounds alternating the two calls, after an
untimed preheat (the GPU's clock ramp, as bench.py); median µs per launch and the spread over rounds. Algorithmic bytes
per frame: fill = frame + 6 B descriptor read, 4 B of checksum fields written (bench.py's primary count; the 64-byte line
it physically rewrites beside it); serialize = payload + the descriptor arrays passed read, H + 6 (+ 4 with status)
written. One JSON line on stdout (append it to profiles/ with tools/collect_ab.py or a redirect).

    python tools/tx_serialize_ab.py [--frames 1048576] [--iters 20] [--reps 7] [--no-status] [--fill-split 0] [--required-only]
        [--note TEXT] [--out profiles/x.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, as bench.py counts it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--ip-len", type=int, default=1500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--preheat-seconds", type=float, default=0.25)
    ap.add_argument("--no-status", action="store_true")
    ap.add_argument("--fill-split", type=int, default=-1,
                    help="dk_diag_tx_set_tuning split for the fill: 0 runs it in dk_tx_kernel, the persistent form "
                         "dk_tx_serialize has, instead of the split kernel its rule picks for large frames")
    ap.add_argument("--required-only", action="store_true",
                    help="pass only the six required descriptor arrays (no tcp_seq / tcp_ack / tcp_win / ip_word): what "
                         "four fewer per-frame arrays are worth; the headers then differ from the batch's, so the "
                         "bit-exact check is skipped and the blob is not the fill's afterwards")
    ap.add_argument("--note", default=None, help="free text carried in the JSON line")
    ap.add_argument("--out", default=None, help="append the JSON line to this file too")
    a = ap.parse_args()
    import ctypes

    import torch

    import __graft_entry__
    from demikernel_amd import Config, RxEngine, TxSegments, synth, tx_links, tx_serialize, tx_tuning
    from demikernel_amd.tx import ip_word

    bid = __graft_entry__.check_loaded_build()
    tx_tuning(split=a.fill_split)
    n = a.frames
    eng = RxEngine(Config(synth.BOB_IPV4), device=0)
    flows = synth.make_flows(1024)
    tr = synth.traffic(n, a.ip_len, flows)
    batch = synth.build_device(tr, eng)  # headers scattered from the host, checksums by dk_tx_checksum
    off, _ = synth.layout(tr.frame_len)
    plen = (tr.ip_len.astype(np.int64) - 40).astype(np.uint16)
    segs = TxSegments.from_numpy(
        (off.astype(np.int64) + 54).astype(np.uint32), plen,
        (6 << 8 | tr.flags.astype(np.uint32) << 16 | 0x50 << 24).astype(np.uint32), tr.src_ip, tr.dst_ip,
        (tr.sport.astype(np.uint32) | tr.dport.astype(np.uint32) << 16),
        **({} if a.required_only else dict(tcp_seq=tr.seq, tcp_ack=tr.ack, tcp_win=tr.window.astype(np.uint32),
                                           ip_word=ip_word(tr.ip_id, tr.ttl))))
    links = torch.from_numpy(tx_links([(synth.BOB_MAC, synth.ALICE_MAC)]).view(np.uint8).copy()).to(batch.blob.device)
    stream = torch.cuda.Stream(device=0)
    status = not a.no_status
    # the timed calls: the C entry points alone, arguments built once, outputs preallocated
    lib = eng.lib
    dev = batch.blob.device
    o_off = torch.empty(n, dtype=torch.int32, device=dev)
    o_len = torch.empty(n, dtype=torch.int16, device=dev)
    o_st = torch.empty(n, dtype=torch.int32, device=dev) if status else None
    cs = segs.c_struct(0)
    sp = ctypes.c_void_p(stream.cuda_stream)
    fill_args = (batch.blob.data_ptr(), batch.frames_bytes, batch.off.data_ptr(), batch.len.data_ptr(), n, sp)
    ser_args = (batch.blob.data_ptr(), batch.blob.numel(), ctypes.byref(cs), links.data_ptr(), 1, o_off.data_ptr(),
                o_len.data_ptr(), o_st.data_ptr() if status else None, sp)

    def fill():
        assert lib.dk_tx_checksum(*fill_args) == 0

    def serialize():
        assert lib.dk_tx_serialize(*ser_args) == 0

    calls = {"dk_tx_checksum": fill, "dk_tx_serialize": serialize}

    # parity first: with every header byte wiped, serialize alone restores the blob the fill completed
    torch.cuda.synchronize()
    want = batch.blob.clone()
    hdr = torch.from_numpy(off.astype(np.int64)).to(batch.blob.device)[:, None] + torch.arange(54, device=batch.blob.device)
    with torch.cuda.stream(stream):
        batch.blob[hdr.reshape(-1)] = 0xA5
        out = tx_serialize(batch.blob, segs, links, stream=stream, status=status)  # the Python wrapper, once
        o_off.fill_(-1)
        o_len.fill_(-1)
        calls["dk_tx_serialize"]()
    torch.cuda.synchronize()
    same = (a.required_only or bool(torch.equal(batch.blob, want))) and bool((out.off == batch.off).all()) and \
        bool((out.len == batch.len).all()) and (not status or bool((out.status == 0).all())) and \
        bool((o_off == batch.off).all()) and bool((o_len == batch.len).all()) and \
        (not status or bool((o_st == 0).all()))
    del hdr

    with torch.cuda.stream(stream):
        t_end = time.perf_counter() + a.preheat_seconds
        while time.perf_counter() < t_end:  # untimed clock ramp
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for rep in range(a.reps + 1):
            for name, fn in calls.items():
                for _ in range(3):
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
    same = same and (a.required_only or bool(torch.equal(batch.blob, want)))

    frame_bytes = int(tr.frame_len.astype(np.int64).sum())
    payload_bytes = int(plen.astype(np.int64).sum())
    # payload_off, payload_len, meta, src_ip, dst_ip, ports (+ tcp_seq, tcp_ack, tcp_win, ip_word)
    desc = 4 + 2 + 4 * (4 if a.required_only else 8)
    algo = {"dk_tx_checksum": frame_bytes + n * (6 + 4),
            "dk_tx_serialize": payload_bytes + n * (desc + 54 + 6 + (4 if status else 0))}
    res = {}
    for name, ts in times.items():
        t = float(np.median(ts))
        res[name] = {"us": round(t, 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)],
                     "algorithmic_bytes": algo[name], "achieved_gbps": round(algo[name] / t / 1e3, 1),
                     "roofline_frac": round(algo[name] / t / 1e3 / HBM_PEAK_GBS, 4)}
    res["dk_tx_checksum"]["roofline_frac_64B_write_floor"] = round(
        (frame_bytes + n * (6 + 64)) / res["dk_tx_checksum"]["us"] / 1e3 / HBM_PEAK_GBS, 4)
    line = json.dumps({"tool": "tx_serialize_ab", **({"note": a.note} if a.note else {}), "build": bid,
                       "timed": "C entry points, preallocated outputs: one kernel per iteration in each arm", "frames": n, "ip_len": a.ip_len, "slot_align": 64,
                       "iters": a.iters, "reps": a.reps, "status_array": status, "fill_split": a.fill_split,
                       "descriptor_arrays": 6 if a.required_only else 10,
                       "blob_restored_bit_exact": None if a.required_only else same,
                       "serialize_over_fill": round(res["dk_tx_serialize"]["us"] / res["dk_tx_checksum"]["us"], 4),
                       **res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    eng.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
