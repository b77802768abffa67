#!/usr/bin/env python3
"""Interleaved A/B of the fused TCP send segmentation against the unfused path, in one process on one workload: C2's,
`--frames` frames of `--mss` payload bytes into `--stride`-byte slots, pushed over `--conns` connections either as one
large buffer per connection (shape "large") or as one single-segment buffer per frame (shape "single").

  segment   dk_tcp_tx_segment: plan, copy + checksum + headers in one pass over the payload, commit. The connection
            table is restored before every call (one 4 KB device copy, inside the timed span) so every call sends the
            same frames.
  unfused   what the project offered before: one hipMemcpy2DAsync device to device (rows of mss bytes, source pitch mss,
            destination pitch = stride) into the slots' payload positions, then dk_tx_serialize on prebuilt descriptors.
            It reads every payload byte twice.
  copy      the hipMemcpy2DAsync of `unfused` alone: the floor for moving these bytes once.

All arms are the bare C entry points through ctypes, arguments prepared and outputs preallocated beforehand. Timing: HIP
events on the launch stream around `--iters` launches, `--reps` rounds alternating the arms, after an untimed preheat;
median µs per launch and the spread over rounds. Algorithmic bytes per frame: read L + the push and connection records,
write 54 + L + 6 (unfused: + L read and L written once more, + its 38 descriptor bytes; copy: L + L). Before timing, the
fused output is compared with the unfused path's, byte for byte. One JSON line per shape on stdout.

    python tools/tx_segment_ab.py [--frames 1048576] [--mss 1460] [--stride 1536] [--lead 0] [--conns 64] [--shape large|single|both] [--iters 20] [--reps 7]
        [--note TEXT] [--out profiles/tx_segment_ab.jsonl]
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

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, as bench.py counts it
D2D = 3  # hipMemcpyDeviceToDevice


def hip_runtime():
    """The HIP runtime this process already loaded (torch's), for hipMemcpy2DAsync."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 mapped")


def run_shape(a, shape, lib, hip, bid):
    import torch

    from demikernel_amd import TxSegments, synth, tx_links
    from demikernel_amd import _native as N
    from demikernel_amd.tcp_tx import PushList, TcpSender, TcpTxResults, tx_conn_table

    dev = torch.device("cuda", 0)
    n, mss, stride, nc = a.frames, a.mss, a.stride, a.conns
    per = n // nc
    assert per * nc == n, "--frames must be a multiple of --conns"
    flows = synth.make_flows(nc, passive=False)
    rng = np.random.default_rng(7)
    tx = tx_conn_table(nc, snd_nxt=rng.integers(0, 1 << 32, nc), rcv_nxt=rng.integers(0, 1 << 32, nc),
                       rcv_wnd_hdr=rng.integers(0, 65536, nc), snd_wnd=0xFFFFFFFF, mss=mss,
                       local_ip=flows["remote_ip"], remote_ip=flows["local_ip"],
                       ports=flows["remote_port"].astype(np.uint32) | flows["local_port"].astype(np.uint32) << 16,
                       ip_word=rng.integers(0, 65536, nc) | 64 << 16)
    if shape == "large":
        conn, off, lens = np.arange(nc), np.arange(nc, dtype=np.int64) * per * mss, np.full(nc, per * mss)
    else:
        conn, off, lens = np.repeat(np.arange(nc), per), np.arange(n, dtype=np.int64) * mss, np.full(n, mss)
    src = torch.randint(0, 256, (n * mss,), dtype=torch.uint8, device=dev)
    out = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    out2 = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    links = torch.from_numpy(tx_links([(synth.BOB_MAC, synth.ALICE_MAC)]).view(np.uint8).copy()).to(dev)
    sender = TcpSender(0)
    d_tx0, d_tx = sender.conns_to_device(tx), sender.conns_to_device(tx)
    push = PushList.from_numpy(conn, off, lens)
    res = TcpTxResults(n, push.n, frame_buf=False)
    stream = torch.cuda.Stream(device=0)
    sp = ctypes.c_void_p(stream.cuda_stream)
    p, r, lay = push.c_struct(), res.c_struct(), N.DkTcpTxLayout(stride, a.lead)
    seg_args = (sender._ctx, src.data_ptr(), src.numel(), ctypes.byref(p), push.n, d_tx.data_ptr(), nc, None,
                links.data_ptr(), 1, out.data_ptr(), out.numel(), ctypes.byref(lay), n, 0, ctypes.byref(r), sp)
    # the unfused path's descriptors: the frames the segmentation produces
    f = np.arange(n, dtype=np.int64)
    c_of = f // per
    j = f % per
    last = (j == per - 1) if shape == "large" else np.ones(n, bool)
    seq = (tx["snd_nxt"][c_of].astype(np.int64) + j * mss) & 0xFFFFFFFF
    segs = TxSegments.from_numpy(
        (f * stride + a.lead + 54).astype(np.uint32), np.full(n, mss, np.uint16),
        (6 << 8 | np.where(last, 0x18, 0x10) << 16 | 0x50 << 24).astype(np.uint32), tx["local_ip"][c_of],
        tx["remote_ip"][c_of], tx["ports"][c_of], tcp_seq=seq.astype(np.uint32), tcp_ack=tx["rcv_nxt"][c_of],
        tcp_win=tx["rcv_wnd_hdr"][c_of].astype(np.uint32), ip_word=tx["ip_word"][c_of])
    o_off = torch.empty(n, dtype=torch.int32, device=dev)
    o_len = torch.empty(n, dtype=torch.int16, device=dev)
    cs = segs.c_struct(0)
    ser_args = (out2.data_ptr(), out2.numel(), ctypes.byref(cs), links.data_ptr(), 1, o_off.data_ptr(),
                o_len.data_ptr(), None, sp)
    cp_args = (ctypes.c_void_p(out2.data_ptr() + a.lead + 54), ctypes.c_size_t(stride), ctypes.c_void_p(src.data_ptr()),
               ctypes.c_size_t(mss), ctypes.c_size_t(mss), ctypes.c_size_t(n), D2D, sp)

    def segment():
        d_tx.copy_(d_tx0, non_blocking=True)  # on `stream` (the timed loop runs under it)
        assert lib.dk_tcp_tx_segment(*seg_args) == 0

    def copy():
        assert hip.hipMemcpy2DAsync(*cp_args) == 0

    def unfused():
        copy()
        assert lib.dk_tx_serialize(*ser_args) == 0

    calls = {"segment": segment, "unfused": unfused, "copy": copy}
    with torch.cuda.stream(stream):
        segment()
        unfused()
    torch.cuda.synchronize()
    h = res.to_numpy()
    same = bool(torch.equal(out, out2)) and h["n_frames"] == n and bool((h["status"] == 0).all()) and \
        bool((res.off_out == o_off).all()) and bool((res.len_out == o_len).all())

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
    L = mss
    records = push.n * 12 + nc * 64
    algo = {"segment": n * (L + 54 + L + 6) + records, "unfused": n * (2 * L + 2 * L + 38 + 54 + 6),
            "copy": n * 2 * L}
    fused_algo = algo["segment"]
    out_res = {}
    for name, ts in times.items():
        t = float(np.median(ts))
        out_res[name] = {"us": round(t, 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)],
                         "bytes_moved": algo[name], "achieved_gbps": round(algo[name] / t / 1e3, 1),
                         # every arm against the bytes the job needs: read L + records, write 54 + L + 6 per frame
                         "hbm_peak_frac_on_algorithmic_bytes": round(fused_algo / t / 1e3 / HBM_PEAK_GBS, 4)}
    line = json.dumps({"tool": "tx_segment_ab", **({"note": a.note} if a.note else {}), "build": bid, "shape": shape,
                       "frames": n, "mss": mss, "stride": stride, "lead": a.lead, "conns": nc, "buffers": push.n, "iters": a.iters,
                       "reps": a.reps, "fused_equals_unfused_bit_exact": same,
                       "segment_over_unfused": round(out_res["segment"]["us"] / out_res["unfused"]["us"], 4),
                       "segment_over_copy": round(out_res["segment"]["us"] / out_res["copy"]["us"], 4), **out_res})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    sender.close()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--mss", type=int, default=1460)
    ap.add_argument("--stride", type=int, default=1536)
    ap.add_argument("--lead", type=int, default=0, help="frame_lead: bytes between a slot's start and its frame")
    ap.add_argument("--conns", type=int, default=64)
    ap.add_argument("--shape", choices=["large", "single", "both"], default="both")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--preheat-seconds", type=float, default=0.25)
    ap.add_argument("--note", default=None, help="free text carried in the JSON line")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch  # noqa: F401

    import __graft_entry__
    from demikernel_amd import _native as N

    bid = __graft_entry__.check_loaded_build()
    lib, hip = N.load_library(), hip_runtime()
    hip.hipMemcpy2DAsync.restype = ctypes.c_int
    ok = True
    for shape in (["large", "single"] if a.shape == "both" else [a.shape]):
        ok = run_shape(a, shape, lib, hip, bid) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
