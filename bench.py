#!/usr/bin/env python3
"""Benchmark: device-resident receive-path transform (checksum + parse + demux) on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
                                                           (N > 1: launched by torch.distributed.run)

A step = one dk_rx_process pass over one HBM-resident batch of the workload (default: BASELINE config 2,
1,048,576 x 1500 B IPv4/TCP frames over 1,024 flows, 1 % corrupted tail), plus, for N > 1, the RCCL all-reduce of the
per-flow packet counts (dk_rx_flow_counts_allreduce over a dk_comm.h communicator: the only collective on this path,
every --gather-every batches on the launch stream). Weak scaling: every rank owns one batch (its packet
shard).
`value` = sum of frame bytes processed by all ranks / max-over-ranks time.  Rank 0 prints one JSON line.
A plain run sets up, warms up, times the K steps and prints the line; --dump-outputs DIR also writes what the last
timed step computed (the result arrays and the accumulated counters) as DIR/<name>.npy.
With --full the line also carries the measured streaming-read ceiling and, at N = 1, the CPU baselines and the other
BASELINE configs as extras (C3 64 B UDP, C4 IMIX shard, C5 10k-flow shard kernel-only and end to end from pinned host
memory, C1-shaped CPU baseline), each with its own roofline fields (--no-cpu / --no-extras leave those parts out).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
DESC_BYTES = 6         # u32 offset + u16 length per frame
RESULT_BYTES = 24      # meta, src_ip, dst_ip, ports, payload, flow_id (u32 each)

WORKLOADS = {
    # name: (description, frames, ip_len spec, flow kind, nflows)
    "c1_tcp1078": ("tcp-echo-shaped: 1078 B IPv4/TCP (1 KiB payload) on one 4-tuple to port 12345", 1 << 17, 1064,
                   "tcp", 1),
    "c2_tcp1500": ("1M x 1500B IPv4/TCP, 1024 flows, device-resident", 1 << 20, 1486, "tcp", 1024),
    "c3_udp64": ("1M x 64B IPv4/UDP (min-size), device-resident, 8 rotating batches", 1 << 20, 50, "udp", 1024),
    "c3_udp64_random_ports": ("C3 with the 1,024 UDP binds on random ports (1024..65535) instead of consecutive ones",
                              1 << 20, 50, "udp_random_ports", 1024),
    "c4_imix": ("IMIX 40/576/1500 at 7:4:1, 2M frames per GPU (16M over 8 GPUs)", 1 << 21, "imix", "tcp", 1024),
    "c4_imix_tilesorted": ("IMIX with each 256-frame tile sorted by size (tuning probe, not a bench line)", 1 << 21,
                           "imix_tilesorted", "tcp", 1024),
    "c4_imix_periodic": ("IMIX with one shuffled 64-frame pattern (37 x 40 B, 21 x 576 B, 6 x 1500 B) repeated: every "
                         "chunk the same bytes (tuning probe for load balance, not a bench line)", 1 << 21,
                         "imix_periodic", "tcp", 1024),
    "c5_tcp1500_10k": ("1500B IPv4/TCP, 10k flows, 2M frames per GPU (16M over 8 GPUs)", 1 << 21, 1486, "tcp", 10000),
}


def dist_env():
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), ws


def make_batch(eng, name, rank, seed_base, world=1, frames=0):
    """This rank's packet shard of the global batch (world x frames-per-GPU frames, weak scaling): the frame-size
    sequence is global and seeded, the shard boundaries are byte-balanced (demikernel_amd.shard), and each rank
    synthesises only its own frames on its own GPU. frames > 0 overrides the workload's frames per GPU."""
    from demikernel_amd import synth
    from demikernel_amd.shard import byte_balanced_shards

    _, n, ip_len, kind, nflows = WORKLOADS[name]
    n = frames or n
    flows = synth.make_flows(nflows, kind=kind)
    total = n * world
    if isinstance(ip_len, str) and ip_len.startswith("imix"):
        ip_all = synth.imix_ip_lengths(total, seed_base)
        if ip_len == "imix_tilesorted":
            m = total // 256 * 256
            ip_all[:m] = np.sort(ip_all[:m].reshape(-1, 256), axis=1).reshape(-1)
        elif ip_len == "imix_periodic":
            pat = np.random.default_rng(seed_base).permutation(np.repeat(np.array([40, 576, 1500], np.uint16),
                                                                         [37, 21, 6]))
            ip_all = np.resize(pat, total).astype(np.uint16)
    else:
        ip_all = np.full(total, ip_len, np.uint16)
    frame_all = np.maximum(ip_all.astype(np.int64) + 14, synth.ETH_MIN_FRAME)
    a, b = byte_balanced_shards(frame_all, world)[rank]
    seed = seed_base + 7919 * rank
    n = b - a
    tr = synth.traffic(n, ip_all[a:b], flows, seed=seed)
    eng.set_sockets(flows)
    batch = synth.build_device(tr, eng, seed=seed)
    synth.corrupt_device(batch, batch.off.cpu().numpy().view(np.uint32), synth.corruption_plan(n, 0.01, tr, seed))
    return batch, flows, tr


PREHEAT_S = 0.25  # untimed clock ramp before each measurement (bench --preheat-seconds)


def set_preheat(seconds: float) -> None:
    global PREHEAT_S
    PREHEAT_S = max(float(seconds), 0.0)


def preheat(eng, batch, stream, seconds):
    """Untimed, before the warmup steps: the receive kernel over this batch for `seconds` of wall time, into a scratch
    result record without counters (the measured steps' counters see none of it). A fresh process measured its first
    ~10 ms of launches 4-7 % slower than steady state (C2 246.7 vs 240.5 us, IMIX 157.0 vs 144.9 us: the GPU's clocks
    ramping, not caches: 300 ms of copies over unrelated buffers removed it too, tools/timing_check.py), and 5 warmup
    steps are ~1 ms of work."""
    import torch

    if seconds <= 0:
        return
    scratch = eng.results(batch.n, counts=False)
    t = time.perf_counter()
    while time.perf_counter() - t < seconds:
        for _ in range(8):
            eng.receive_batch(batch, scratch, stream=stream)
        torch.cuda.synchronize()
    del scratch


GATHER_EVERY = 8  # batches per all-reduce of the counters at N > 1 (bench --gather-every)


def time_kernel(eng, batches, res, steps, warmup, stream, dist=None, comm=None):
    """Run the untimed preheat, then warmup + timed steps. A step = the receive pass over one batch, whose counter
    rows the next step's kernel completes (DK_RX_BATCH_DEFER_COUNTS; the last step's by one flush launch inside the
    timed region), + for N > 1 the all-reduce of the counters over RCCL every GATHER_EVERY steps and after the last
    (ShardedReceiver: double-buffered accumulating counters, the collective on the launch stream). Returns (wall seconds for `steps`,
    per-step seconds on the launch stream from HIP events around the timed region incl. the flush, per-step collective
    seconds measured unoverlapped)."""
    import torch

    from demikernel_amd.shard import ShardedReceiver

    sr = ShardedReceiver(eng, res, comm, stream, gather_every=GATHER_EVERY, side_stream=False)
    preheat(eng, batches[0], stream, PREHEAT_S)
    for k in range(warmup):
        sr.step(batches[k % len(batches)])
    sr.drain()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    # HIP events bracket the timed region only (an event pair around every launch adds a marker + cache writeback per
    # step and perturbs the kernel it measures): per-launch time = region / steps, on the stream the kernels run on.
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    for k in range(steps):
        sr.step(batches[k % len(batches)])
    sr.flush()  # the last step's deferred counters (one small launch on the stream, inside the timed region)
    e1.record(stream)
    sr.drain()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    kern = e0.elapsed_time(e1) / 1e3 / steps
    coll = []
    if comm is not None:  # the collective alone, unoverlapped, for the report
        for _ in range(5):
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record(sr.side)
            sr.reduce(0, sr.side)
            c1.record(sr.side)
            torch.cuda.synchronize()
            coll.append(c0.elapsed_time(c1) / 1e3)
    return wall, kern, coll, sr


def mbuf_zero_copy_rate(dev, stream, n=1 << 17, slot=2048, data_off=128, reps=5):
    """C2-sized frames (1500 B TCP, 1,024 flows) in 2 KiB mbuf slots of a page-locked host buffer (a DPDK mempool
    registered with hipHostRegister), processed by dk_rx_process straight from host memory: the kernel's loads cross
    PCIe. Median GB/s of frame bytes over `reps` launches."""
    import torch

    from demikernel_amd import Config, FrameBatch, RxEngine, synth

    eng = RxEngine(Config(synth.BOB_IPV4), device=dev)
    flows = synth.make_flows(1024)
    tr = synth.traffic(n, np.full(n, 1486, np.uint16), flows, seed=synth.SEED + 77)
    packed, poff, lens = synth.build_numpy(tr)
    mb = np.zeros(n * slot, np.uint8)
    off = (np.arange(n, dtype=np.uint64) * slot + data_off).astype(np.uint32)
    view = mb.reshape(n, slot)
    view[:, data_off: data_off + 1500] = packed.reshape(n, -1)[:, :1500] if poff[1] - poff[0] == 1536 else \
        np.stack([packed[o: o + 1500] for o in poff])
    pinned = torch.from_numpy(mb).pin_memory()
    eng.set_sockets(flows)
    b = FrameBatch.host_mapped(pinned, off, lens, device=dev)
    r = eng.results(n)
    eng.receive_batch(b, r, stream=stream)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        eng.receive_batch(b, r, stream=stream)
        e1.record(stream)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    t = float(np.median(ts))
    fb = int(lens.astype(np.int64).sum())
    got = r.to_numpy()
    return {"gbps": round(fb / t / 1e9, 2), "mpkt_s": round(n / t / 1e6, 1), "frames": n, "slot_bytes": slot,
            "data_off": data_off, "delivered_frac": round(float(np.mean((got["meta"] & 0xFF) == 0)), 3),
            "stat": "median", "reps": reps,
            "pipeline": "dk_rx_process on a host-mapped (page-locked) blob: zero-copy, PCIe-bound"}


DUMP_MAX_BYTES = 64 << 20  # --dump-outputs writes at most this much in all
DUMP_SEED = 20240607


def dump_outputs(path, res, sr):
    """--dump-outputs: what the timed path's caller holds after the last timed step, as float64 .npy files (every u32
    and every counter here is exact in a float64): the per-frame result arrays the last step wrote and the flow /
    verdict counters accumulated over the warmup and timed steps. When the per-frame arrays would pass DUMP_MAX_BYTES,
    the same fixed, seeded sample of frames is taken from each (its indices in frame_index.npy)."""
    os.makedirs(path, exist_ok=True)
    got = res.to_numpy()
    fc, vc = sr.counts()
    counts = {"flow_counts": fc.cpu().numpy().view(np.uint64), "verdict_counts": vc.cpu().numpy().view(np.uint64)}
    frame = {k: v for k, v in got.items() if k not in counts}
    budget = DUMP_MAX_BYTES - 8 * sum(v.size for v in counts.values())
    keep = budget // (8 * (len(frame) + 1))  # frames per array, frame_index included
    idx = np.arange(res.n, dtype=np.int64)
    if res.n > keep:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(res.n, size=keep, replace=False))
        frame = {k: v[idx] for k, v in frame.items()}
    frame["frame_index"] = idx
    for k, v in {**frame, **counts}.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(v, dtype=np.float64))


def cpu_info():
    """What the CPU baseline ran on: model name, CPUs this process may use (affinity), cgroup CPU quota."""
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else round(int(q) / int(per), 2)
    except (OSError, ValueError):
        pass
    return {"cpu_model": model, "cpus_usable": len(os.sched_getaffinity(0)), "cpu_logical": os.cpu_count(),
            "cgroup_cpu_quota": quota}


def host_sample(batch, sample_frames):
    """The first `sample_frames` frames of a device batch, copied to host (blob, off, lens)."""
    n = min(sample_frames, batch.n)
    off = batch.off[:n].cpu().numpy().view(np.uint32).copy()
    lens = batch.len[:n].cpu().numpy().view(np.uint16).copy()
    end = int(off[-1]) + int(lens[-1])
    return batch.blob[:end].cpu().numpy(), off, lens


def cpu_rate(blob, off, lens, flows, min_seconds, threads=1):
    """Oracle (CPU restatement of the reference) over host arrays, repeated for >= min_seconds; median rates."""
    from demikernel_amd import ipv4, synth
    from oracle.oracle import OraclePeer

    peer = OraclePeer(ipv4(synth.BOB_IPV4))
    peer.set_flows(flows)
    nbytes = int(lens.astype(np.int64).sum())
    times, used, t_all = [], 1, time.perf_counter()
    while time.perf_counter() - t_all < min_seconds or len(times) < 3:
        t = time.perf_counter()
        if threads == 1:
            peer.process(blob, off, lens)
        else:
            _, used = peer.process_mt(blob, off, lens, threads)
        times.append(time.perf_counter() - t)
    t = float(np.median(times))
    return {"gbps": nbytes / t / 1e9, "mpkt_s": len(off) / t / 1e6, "cores": used, "frames": len(off),
            "bytes": nbytes, "reps": len(times)}


def cpu_baseline(batch, flows, sample_frames, min_seconds, threads=1):
    """Oracle on a bounded sample of the same workload, host cores (kept for tools that import it)."""
    blob, off, lens = host_sample(batch, sample_frames)
    r = cpu_rate(blob, off, lens, flows, min_seconds, threads)
    return r["gbps"], r["cores"], r["frames"], r["bytes"], r["reps"]


def host_path_rate(eng, batch, flows, nframes, reps=5):
    """End-to-end GB/s of frame bytes for a pinned host batch through dk_rx_process_host (PCIe-inclusive): pinned
    host frames + descriptors -> HBM -> kernel -> results back to pinned host arrays. Median of `reps`."""
    import torch

    from demikernel_amd import RxResults

    n = min(nframes, batch.n)
    off = batch.off[:n].cpu().numpy().view(np.uint32).copy()
    lens = batch.len[:n].cpu().numpy().view(np.uint16).copy()
    end = int(off[-1]) + int(lens[-1])
    pinned = torch.empty(end, dtype=torch.uint8, pin_memory=True)
    pinned.copy_(batch.blob[:end])
    off_p = torch.from_numpy(off.view(np.int32)).pin_memory()
    len_p = torch.from_numpy(lens.view(np.int16)).pin_memory()
    res = RxResults(n, len(flows), host=True)
    nbytes = int(lens.astype(np.int64).sum())
    aligned = bool(np.all(off % 16 == 0))  # the batch's alignment hint, computed once outside the timed region
    rates = []
    for _ in range(reps):
        t = time.perf_counter()
        eng.receive_batch_host(pinned.numpy(), off_p.numpy(), len_p.numpy(), res, aligned16=aligned)
        rates.append(nbytes / (time.perf_counter() - t) / 1e9)
    return {"gbps": round(float(np.median(rates)), 2), "gbps_max": round(max(rates), 2), "frames": n, "bytes": nbytes,
            "reps": reps, "stat": "median",
            "pipeline": "dk_rx_process_host from pinned, GPU-mapped host memory: frames read in place by one launch "
                        "(zero-copy), descriptors H2D, results D2H (pageable memory: 3 streams of staged copies)"}


def zero_copy_rate(eng, batch, flows, nframes, reps=5):
    """End-to-end GB/s of frame bytes with the frames left in pinned host memory and read by the kernel in place over
    PCIe (FrameBatch.host_mapped; the DPDK-mbuf path): descriptors H2D, kernel, results D2H into pinned host arrays,
    all inside the timed region. Median of `reps`."""
    import torch

    from demikernel_amd import FrameBatch, RxResults

    n = min(nframes, batch.n)
    off = batch.off[:n].cpu().numpy().view(np.uint32).copy()
    lens = batch.len[:n].cpu().numpy().view(np.uint16).copy()
    end = int(off[-1]) + int(lens[-1])
    pinned = torch.empty(end, dtype=torch.uint8, pin_memory=True)
    pinned.copy_(batch.blob[:end])
    off_p = torch.from_numpy(off.view(np.int32)).pin_memory()
    len_p = torch.from_numpy(lens.view(np.int16)).pin_memory()
    b = FrameBatch.host_mapped(pinned, off, lens, device=eng.device)
    res = eng.results(n)
    host = RxResults(n, len(flows), host=True)
    nbytes = int(lens.astype(np.int64).sum())
    rates = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        b.off.copy_(off_p, non_blocking=True)
        b.len.copy_(len_p, non_blocking=True)
        eng.receive_batch(b, res)
        for k, v in res.t.items():
            host.t[k].copy_(v, non_blocking=True)
        torch.cuda.synchronize()
        rates.append(nbytes / (time.perf_counter() - t) / 1e9)
    rates = rates[1:]
    return {"gbps": round(float(np.median(rates)), 2), "gbps_max": round(max(rates), 2), "frames": n, "bytes": nbytes,
            "reps": reps, "stat": "median",
            "pipeline": "frames read in place from pinned host memory (zero-copy), descriptors H2D, results D2H"}


def ring_path_rate(eng, batch, flows, nframes, block_size=1 << 22, reps=5):
    """end-to-end GB/s of frame bytes for frames sitting in a TPACKET_V3 receive ring (the
    layout AF_PACKET fills; page-locked with hipHostRegister): block scan on the host, H2D of the blocks' byte ranges,
    kernel, D2H of the results (dk_rx_process_tpacket3). PCIe-inclusive; reported beside `value`, never as `value`."""
    from demikernel_amd import RxResults
    from demikernel_amd import ring as RG

    n = min(nframes, batch.n)
    off = batch.off[:n].cpu().numpy().view(np.uint32).astype(np.int64)
    lens = batch.len[:n].cpu().numpy().view(np.uint16).copy()
    end = int(off[-1]) + int(lens[-1])
    blob = batch.blob[:end].cpu().numpy()
    # the ring's pages on the GPU's NUMA node (as a LibOS creating the PACKET_RX_RING from a thread there gets them):
    # placed by first touch on the other socket the path lost 5 % (tools/ring_numa.py)
    node = RG.gpu_numa_node(batch.blob.device.index or 0)
    ring, used, _, elen = RG.build_tpacket3(blob, off, lens, block_size, numa_node=node)
    r = RG.TpacketRing(ring, block_size)
    res = RxResults(n, len(flows), host=True)
    nbytes = int(elen.astype(np.int64).sum())
    rates, scans = [], []
    try:
        for _ in range(reps):
            t = time.perf_counter()
            nf, nb = r.receive(eng, 0, used, res)
            rates.append(nbytes / (time.perf_counter() - t) / 1e9)
            assert nf == n and nb == used
            t = time.perf_counter()  # the host's share: the block scan alone (dk_ring_scan_tpacket3)
            r.scan(0, used, n)
            scans.append(time.perf_counter() - t)
    finally:
        r.close()
    return {"gbps": round(float(np.median(rates)), 2), "gbps_max": round(max(rates), 2), "frames": n, "bytes": nbytes,
            "blocks": used, "block_size": block_size, "reps": reps, "stat": "median",
            "host_scan_ms": round(float(np.median(scans)) * 1e3, 3), "ring_numa_node": node,
            "pipeline": "TPACKET_V3 block scan + dk_rx_process_host over the registered ring"}


def tcp_rate(stream, nseg=1 << 20, nconns=1 << 14, iters=10, cpu_seconds=3.0, buffer_size=1 << 24, reorder=3.0):
    """dk_tcp_rx_process over one dk_rx batch's results (nseg 1460-byte TCP segments spread
    over nconns established connections, reordered / duplicated / stray as synth.tcp_streams makes them), Mseg/s from
    HIP events around each call (the connection table is restored from a pristine copy between calls, outside the
    timed span); the CPU restatement (oracle/dk_tcp_oracle.cpp, 1 thread) on the same arrays beside it."""
    import torch

    from demikernel_amd import RxResults, synth
    from demikernel_amd._native import TCP_ACTIONS as TCP_ACTION_NAMES
    from demikernel_amd.tcp import TcpOut, TcpReceiver
    from oracle import oracle as O

    dev = stream.device
    _, tr, table = synth.tcp_streams(nseg, nconns, 1500, buffer_size=buffer_size, reorder=reorder)
    rx = {"meta": (6 << 8 | tr.flags.astype(np.uint32) << 16 | 0x50 << 24).astype(np.uint32),
          "flow_id": tr.flow.astype(np.uint32), "tcp_seq": tr.seq, "tcp_ack": tr.ack,
          "payload": (54 | (tr.ip_len.astype(np.uint32) - 40) << 16).astype(np.uint32)}
    r = RxResults(nseg, 1, device=dev, tcp_fields=True, counts=False)
    for k, v in rx.items():
        r.t[k].copy_(torch.from_numpy(v.view(np.int32)))
    tcp = TcpReceiver(dev.index or 0)
    pristine = tcp.conns_to_device(table)
    conns = pristine.clone()
    out = TcpOut(nseg, len(table), dev.index or 0)
    times = []
    walks = []
    with torch.cuda.stream(stream):
        for i in range(iters + 2):
            conns.copy_(pristine)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            tcp.process(r, conns, out, stream=stream)
            e1.record(stream)
            torch.cuda.synchronize()
            walks.append(tcp.last_walk)
            if i >= 2:
                times.append(e0.elapsed_time(e1) / 1e3)
    got = out.to_numpy()
    hist = np.bincount(got["action"], minlength=13)
    t = float(np.median(times))
    tcp.close()
    # CPU restatement on the same segments (bounded: repeat until cpu_seconds)
    reps, t0 = 0, time.perf_counter()
    while True:
        O.tcp_process(table.copy(), rx)
        reps += 1
        if time.perf_counter() - t0 >= cpu_seconds:
            break
    tc = (time.perf_counter() - t0) / reps
    return {"mseg_s": round(nseg / t / 1e6, 1), "ms_avg": round(t * 1e3, 4), "segments": nseg, "connections": nconns,
            "buffer_size": buffer_size, "reorder": reorder,
            "delivered_frac": round(float(hist[1]) / nseg, 3),
            "actions": {name: int(c) for name, c in zip(TCP_ACTION_NAMES, hist) if c},
            "cpu_baseline": {"mseg_s": round(nseg / tc / 1e6, 2), "cores": 1, "kind": "port", "reps": reps},
            "walk": walks[-1], "walk_first_call": walks[0],
            "pipeline": "key + onesweep radix sort (rocPRIM) + ranges + per-connection walk (lanes = connections, "
                        "store in LDS; one wave per connection with a parallel 64-segment check at >= 8 "
                        "segments per connection; at >= 1,024 and <= 256 connections the scan walk: windows "
                        "precomputed across the chip, 64 windows per wave scan, decided windows written in parallel — "
                        "unless the context's last finished call stored >= 0.1 % of its segments out of order at >= 16 "
                        "connections: then the wave walk)"}


def rx_kernel_name(frame_bytes, n):
    """The receive kernel family the host picks for a batch (rx_host.cpp launch_batch: mean blob bytes per frame; the
    blob holds 64-byte-aligned slots, so its size is rounded up per frame)."""
    per = frame_bytes // max(n, 1)
    return ("dk_rx_small_kernel" if per <= 96 else "dk_rx_split_kernel" if per >= 1280 else
            "dk_rx_kernel (staged)" if per >= 128 else "dk_rx_kernel")


def tx_rate(eng, batch, frame_bytes, stream, iters=20):
    """TX checksums over an HBM-resident batch in both contracts: dk_tx_checksum (frame bytes read, the two fields
    patched in place) and dk_tx_checksum_fields (the same read pass, the pair returned as 4 bytes per frame)."""
    import torch

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3 / iters

    t = timed(lambda: eng.tx_checksum(batch, stream=stream))
    fields = torch.empty(batch.n, dtype=torch.int32, device=batch.off.device)
    tf = timed(lambda: eng.tx_checksum_fields(batch, fields, stream=stream))
    # Bytes per frame: the frame read + its descriptor + the write. The fields themselves are 4 bytes (IPv4 + L4
    # checksum), but an in-place patch cannot reach HBM as less than one 64-byte write (the DRAM burst; WRITE_SIZE
    # counts exactly 64 B per frame, profiles/pmc_traffic.json): that physical write floor is what the in-place
    # roofline counts; the 4-byte figure is kept beside it. The fields form writes exactly the 4 bytes.
    algo = frame_bytes + batch.n * (DESC_BYTES + 64)
    algo_fields = frame_bytes + batch.n * (DESC_BYTES + 4)
    big = frame_bytes // max(batch.n, 1) >= 1024
    # Primary fraction: the field bytes (frame + descriptor + the 4 bytes of checksums), as every round before round 5
    # counted it; the 64-byte line floor of an in-place patch beside it.
    return {"gbps": round(frame_bytes / t / 1e9, 1), "kernel_ms_avg": round(t * 1e3, 4),
            "roofline_achieved_gbps": round(algo_fields / t / 1e9, 1),
            "roofline_frac": round(algo_fields / t / 1e9 / HBM_PEAK_GBS, 4),
            "algorithmic_bytes_per_launch": algo_fields,
            "bytes_counted": "frame + 6 B descriptor + the 4 B of checksum fields per frame",
            "roofline_frac_64B_write_floor": round(algo / t / 1e9 / HBM_PEAK_GBS, 4),
            "bytes_counted_64B_write_floor": "frame + 6 B descriptor + 64 B written per frame (the physical write "
                                             "floor of an in-place patch: WRITE_SIZE counts 64 B per frame)",
            "kernel": "dk_tx_split_kernel" if big else "dk_tx_kernel",
            "fields_form": {"entry": "dk_tx_checksum_fields", "gbps": round(frame_bytes / tf / 1e9, 1),
                            "kernel_ms_avg": round(tf * 1e3, 4),
                            "roofline_achieved_gbps": round(algo_fields / tf / 1e9, 1),
                            "roofline_frac": round(algo_fields / tf / 1e9 / HBM_PEAK_GBS, 4),
                            "algorithmic_bytes_per_launch": algo_fields,
                            "bytes_counted": "frame + 6 B descriptor + 4 B of checksum pair written per frame",
                            "kernel": "dk_tx_split_kernel<fields>" if big else "dk_tx_kernel<fields>"}}


def read_ceiling(batch, stream, iters=10):
    """On-box streaming-read ceiling: dk_diag_read_probe over the same frame blob, register loads
    (global mode 3, buffer mode 6) and LDS-DMA (mode 4), 4 and 8 waves per CU; best GB/s and its configuration."""
    import torch

    from demikernel_amd import _native as N

    lib = N.load_library()
    nbytes = batch.blob.numel() // 16 * 16
    cus = torch.cuda.get_device_properties(batch.blob.device).multi_processor_count
    best = (0.0, "")
    names = {3: "global_load register", 4: "LDS-DMA", 6: "buffer_load register"}
    for mode in (3, 4, 6):
        for per_cu in (4, 8):
            grid = per_cu * cus // 4  # 256-thread workgroups: 4 waves each
            scratch = torch.zeros(grid, dtype=torch.int32, device=batch.blob.device)
            call = lambda: lib.dk_diag_read_probe(ctypes.c_void_p(batch.blob.data_ptr()), nbytes,  # noqa: E731
                                                  ctypes.c_void_p(scratch.data_ptr()), grid, mode,
                                                  ctypes.c_void_p(stream.cuda_stream))
            for _ in range(3):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(iters):
                call()
            e1.record(stream)
            torch.cuda.synchronize()
            gbs = nbytes / (e0.elapsed_time(e1) / 1e3 / iters) / 1e9
            if gbs > best[0]:
                best = (gbs, f"dk_diag_read_probe mode {mode} ({names[mode]} loads), "
                             f"{per_cu} waves/CU, {nbytes / 1e9:.2f} GB")
    return best


def load_traffic_profile(workload):
    """HBM bytes per launch from the committed rocprofv3 --pmc summary (profiles/), if one exists for this workload."""
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(p):
        return None
    try:
        d = json.load(open(p))
        return d.get(workload, {}).get("hbm_bytes_per_launch")
    except Exception:
        return None


def rx_extra(name, dev, stream, steps=30, warmup=3, rotate=1, dst_ip=True, tcp_fields=False):
    """Device-resident kernel rate of another BASELINE config on this GPU (its own engine and batches; `rotate`
    distinct batches when one would sit in the 256 MB MALL), with its roofline fields. tcp_fields: the record a LibOS
    binding consumes — tcp_seq / tcp_ack / tcp_win (12 more bytes per frame) and the tcp_opts records
    (written for option-bearing segments only: none in these batches)."""
    from demikernel_amd import Config, RxEngine, synth

    eng = RxEngine(Config(synth.BOB_IPV4), device=dev)
    made = [make_batch(eng, name, 0, synth.SEED + 1000 * k) for k in range(rotate)]
    batches = [m[0] for m in made]
    _, flows, tr = made[0]
    n = batches[0].n
    res = eng.results(n, dst_ip=dst_ip, tcp_fields=tcp_fields, tcp_opts=tcp_fields)
    wall, kern, _, _ = time_kernel(eng, batches, res, steps, warmup, stream)
    fb = int(tr.frame_len.astype(np.int64).sum())
    rb = (RESULT_BYTES if dst_ip else RESULT_BYTES - 4) + (12 if tcp_fields else 0)
    algo = fb + n * (DESC_BYTES + rb)
    out = {"workload": WORKLOADS[name][0], "frames": n, "flows": len(flows), "batches_rotated": rotate,
           "gbps": round(fb * steps / wall / 1e9, 2), "mpkt_s": round(n * steps / wall / 1e6, 1),
           "kernel_ms_avg": round(kern * 1e3, 4), "kernel": rx_kernel_name(int(batches[0].frames_bytes), n),
           "result_bytes_per_frame": rb,
           "roofline": {"bound": "hbm", "achieved": round(algo / kern / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(algo / kern / 1e9 / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": algo,
                        "traffic": load_traffic_profile(name + ("_libos" if tcp_fields else ""))}}
    return out, eng, batches[0], flows


def device_identity(dev) -> dict:
    """What identifies this rank's GPU in the line (name, PCI location / UUID where torch exposes them)."""
    import torch

    p = torch.cuda.get_device_properties(dev)
    ident = {"device_index": int(dev), "name": p.name}
    for k in ("pci_bus_id", "pci_device_id", "pci_domain_id"):
        if hasattr(p, k):
            ident[k] = int(getattr(p, k))
    if hasattr(p, "uuid"):
        ident["uuid"] = str(p.uuid)
    return ident


class CommSizeError(SystemExit):
    """A scaling line whose RCCL communicator does not hold every rank is refused (exit status 4)."""

    def __init__(self, nranks, world):
        super().__init__(4)
        self.nranks, self.world = nranks, world

    def __str__(self):
        return f"bench: the RCCL communicator holds {self.nranks} ranks, the job {self.world}: no scaling line"


def check_comm_size(nranks, world):
    """in RCCL mode the communicator's own rank count (dk_comm_count) must equal the job's world
    size, or the run exits non-zero before any line is printed."""
    if nranks != world:
        e = CommSizeError(nranks, world)
        print(str(e), file=sys.stderr, flush=True)
        raise e


def scale_fields(world, comm, per_rank, coll_s, gather_every):
    """The fields by which a multi-GPU line proves itself: how many ranks the product's RCCL
    communicator holds (dk_comm_count; None when the counters went through the test-only torch stand-in or there is
    no communicator), each rank's own kernel time next to the max-over-ranks wall time, the collective's own time and
    how often it runs."""
    nranks = None
    kind = "none"
    if comm is not None and hasattr(comm, "count"):  # demikernel_amd.Comm: the include/dk_comm.h communicator
        nranks = int(comm.count())
        kind = "rccl (dk_rx_flow_counts_allreduce_to over dk_comm.h)"
        check_comm_size(nranks, world)
    elif comm is not None:
        kind = "TEST ONLY: torch.distributed all_reduce (--counts-via-torch-gloo-test)"
    rows = sorted(per_rank, key=lambda r: r["rank"])
    ks = [r["kernel_ms_per_step"] for r in rows]
    return {"rccl_nranks": nranks, "collective_kind": kind, "world_size": world,
            "gather_every": gather_every if world > 1 else None,
            "collective_ms_avg": round(float(np.mean(coll_s)) * 1e3, 4) if coll_s else None,
            "per_rank": rows,
            "kernel_ms_per_step_max": round(max(ks), 4) if ks else None,
            "kernel_ms_per_step_min": round(min(ks), 4) if ks else None}


def main():
    global GATHER_EVERY
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="c2_tcp1500", choices=sorted(k for k in WORKLOADS if k != "c1_tcp1078"))
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--cpu-sample", type=int, default=1 << 17)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the streaming-read ceiling, the CPU baselines and the "
                         "other BASELINE configs (the extras of the line); a plain run only times --workload")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step computed (result arrays, accumulated counters) to "
                         "DIR/<name>.npy (rank 0, float64, at most 64 MB: a fixed seeded sample of frames beyond that)")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the CPU baselines")
    ap.add_argument("--host-frames", type=int, default=1 << 19)
    ap.add_argument("--no-extras", action="store_true", help="--full without the read ceiling and the other configs")
    ap.add_argument("--preheat-seconds", type=float, default=PREHEAT_S,
                    help="untimed receive launches before each measurement's warmup steps (GPU clock ramp)")
    ap.add_argument("--backend", default="gloo", choices=["nccl", "gloo"],
                    help="N > 1: process group for the barrier and the max-over-ranks timing only (the counters are "
                         "reduced by dk_rx_flow_counts_allreduce_to over RCCL)")
    ap.add_argument("--gather-every", type=int, default=GATHER_EVERY,
                    help="N > 1: batches per all-reduce of the node-wide counters (exact at every gather and at the "
                         "end; RCCL's kernel does not run beside the receive kernels, DESIGN.md §7)")
    ap.add_argument("--frames-per-gpu", type=int, default=0,
                    help="override the workload's frames per GPU (tests only; the line's config records it)")
    ap.add_argument("--counts-via-torch-gloo-test", action="store_true",
                    help="TEST ONLY: reduce the counters through torch.distributed gloo instead of the product's RCCL "
                         "communicator (2 ranks on one GPU, which RCCL refuses); the line names it")
    ap.add_argument("--counts-out", default="",
                    help="write the node-wide flow / verdict counters after the timed steps to this .npz (rank 0)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    extras, cpu = args.full and not args.no_extras, args.full and not args.no_cpu
    set_preheat(args.preheat_seconds)
    GATHER_EVERY = max(args.gather_every, 1)

    import torch

    rank, local_rank, world = dist_env()
    dist, comm = None, None
    if world > 1:
        import torch.distributed as dist  # noqa: F811

        local_dev = local_rank % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local_dev)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_dev))
        else:
            dist.init_process_group("gloo")
    else:
        torch.cuda.set_device(0)
    dev = torch.cuda.current_device()

    from demikernel_amd import Comm, Config, RxEngine, synth
    from demikernel_amd.shard import broadcast_comm_id

    collective = "none"
    if world > 1 and args.counts_via_torch_gloo_test:
        from demikernel_amd.shard import TorchCountsAllreduce

        comm = TorchCountsAllreduce(dist.group.WORLD if args.backend == "gloo" else dist.new_group(backend="gloo"))
        collective = "TEST ONLY: torch.distributed gloo all_reduce of the counters (--counts-via-torch-gloo-test)"
    elif world > 1:  # the receive path's own RCCL communicator (include/dk_comm.h), bootstrapped over the process group
        try:
            comm = Comm.init_rank(world, broadcast_comm_id(dist, Comm.unique_id), rank, dev)
        except Exception as e:  # noqa: BLE001 — no silent fallback: a scaling line must come from the product collective
            print(f"bench: rank {rank}: dk_comm_init_rank failed ({e}); the packet-sharded path needs the RCCL "
                  f"communicator of include/dk_comm.h", file=sys.stderr, flush=True)
            sys.exit(3)
        check_comm_size(comm.count(), world)  # before any timing: a mis-sized communicator prints no line
        collective = (f"dk_rx_flow_counts_allreduce_to (RCCL all-reduce of accumulating u64 flow + verdict counters) "
                      f"every {GATHER_EVERY} batches and after the last, on the launch stream (RCCL's kernel does not "
                      f"run beside the receive kernels: profiles/r04_overlap.json), double-buffered counter sets "
                      f"(node-wide counts exact at every gather)")

    eng = RxEngine(Config(synth.BOB_IPV4), device=dev)
    stream = torch.cuda.current_stream(dev)
    name = args.workload
    batch, flows, tr = make_batch(eng, name, rank, synth.SEED, world, args.frames_per_gpu)
    batches = [batch]
    if name.startswith("c3_udp64"):  # 64 B batches fit in the 256 MB MALL: rotate 8 distinct batches (> 512 MB)
        batches += [make_batch(eng, name, rank, synth.SEED + 1000 * k, world, args.frames_per_gpu)[0]
                    for k in range(1, 8)]
    res = eng.results(batch.n)
    frame_bytes = int(tr.frame_len.astype(np.int64).sum())

    wall, kern_avg, coll, sr = time_kernel(eng, batches, res, args.steps, args.warmup, stream, dist, comm)
    if args.counts_out and rank == 0:
        fc, vc = sr.counts()
        np.savez(args.counts_out, flow_counts=fc.cpu().numpy().view(np.uint64),
                 verdict_counts=vc.cpu().numpy().view(np.uint64), steps=args.steps + args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res, sr)
    mine = {"rank": rank, "kernel_ms_per_step": round(kern_avg * 1e3, 4),
            "wall_ms_per_step": round(wall / args.steps * 1e3, 4), "frames": batch.n, "frame_bytes": frame_bytes,
            "gpu": device_identity(dev)}
    if dist is not None:
        cdev = "cuda" if args.backend == "nccl" else "cpu"
        t = torch.tensor([wall], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())
        tb = torch.tensor([frame_bytes, batch.n], dtype=torch.int64, device=cdev)
        dist.all_reduce(tb)
        total_bytes, total_frames = int(tb[0]), int(tb[1])
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    else:
        total_bytes, total_frames = frame_bytes, batch.n
        per_rank = [mine]

    value = total_bytes * args.steps / wall / 1e9
    algo = frame_bytes + batch.n * (DESC_BYTES + RESULT_BYTES)
    achieved = algo / kern_avg / 1e9
    traffic = load_traffic_profile(name)

    out = {
        "metric": "GB/s packet bytes checksummed+parsed (device-resident)",
        "value": round(value, 2),
        "unit": "GB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "untimed_preheat_s": PREHEAT_S,
        "ms_per_step": round(wall / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (seeded frames generated on device; 1% corrupted tail)",
        "config": {"workload": WORKLOADS[name][0], "name": name, "frames_per_gpu": batch.n,
                   "global_frames": total_frames, "parallelism": f"packet-shard x{world}",
                   "collective": collective},
        "mpkt_s": round(total_frames * args.steps / wall / 1e6, 2),
        # the content hash compiled into the loaded libdk_rx.so (__graft_entry__.tree_build_id of its sources)
        "build_id": eng.build_id(),
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                     "kernel_ms_avg": round(kern_avg * 1e3, 4),
                     "algorithmic_bytes_per_launch": algo, "kernel": rx_kernel_name(int(batch.frames_bytes), batch.n)},
    }
    if extras:
        ceil_gbs, ceil_cfg = read_ceiling(batch, stream)
        out["roofline"]["measured_read_ceiling"] = {"value": round(ceil_gbs, 1), "unit": "GB/s", "probe": ceil_cfg,
                                                    "frac": round(achieved / ceil_gbs, 4)}
    out.update(scale_fields(world, comm, per_rank, coll, GATHER_EVERY))
    host = cpu_info()
    if rank == 0 and world == 1 and cpu:
        blob_s, off_s, lens_s = host_sample(batch, args.cpu_sample)
        r = cpu_rate(blob_s, off_s, lens_s, flows, args.cpu_seconds)
        out["cpu_baseline"] = {"value": round(r["gbps"], 3), "unit": "GB/s", "cores": 1, "kind": "port",
                               "mpkt_s": round(r["mpkt_s"], 2),
                               "sample": f"first {r['frames']} frames of the same batch ({r['bytes'] / 1e6:.0f} MB), "
                                         f"{r['reps']} reps over >= {args.cpu_seconds:.0f} s, median; "
                                         f"oracle/dk_oracle.cpp (C++ restatement of the Rust path, clang -O3, 1 thread "
                                         f"as the reference's single-threaded LibOS)", **host}
        if extras:
            # the reference's own config 1 shape (tcp-echo: 1 KiB payloads on one 4-tuple to port 12345,
            # tools/ci/job/linux.py:145, examples/tcp-echo/client.rs:82) and config 3 (64 B UDP), 1 core each
            e1 = RxEngine(Config(synth.BOB_IPV4), device=dev)
            b1, f1, _ = make_batch(e1, "c1_tcp1078", 0, synth.SEED)
            r1 = cpu_rate(*host_sample(b1, b1.n), f1, 3.0)
            out["cpu_baseline"]["c1"] = {"gbps": round(r1["gbps"], 3), "mpkt_s": round(r1["mpkt_s"], 2), "cores": 1,
                                         "sample": f"{r1['frames']} x 1078 B TCP frames, one Active 4-tuple, "
                                                   f"{r1['reps']} reps, median"}
            del e1, b1
            e3 = RxEngine(Config(synth.BOB_IPV4), device=dev)
            b3, f3, _ = make_batch(e3, "c3_udp64", 0, synth.SEED)
            r3 = cpu_rate(*host_sample(b3, 1 << 20), f3, 3.0)
            out["cpu_baseline"]["c3"] = {"gbps": round(r3["gbps"], 3), "mpkt_s": round(r3["mpkt_s"], 2), "cores": 1,
                                         "sample": f"{r3['frames']} x 64 B UDP frames (the C3 batch), {r3['reps']} "
                                                   f"reps, median"}
            del e3, b3
            # the same restatement on every CPU this process may use (OpenMP packet shards), as a scaled figure: the
            # CPUs in its affinity mask, capped by its cgroup CPU quota (more threads than the quota only time-slice)
            threads = host["cpus_usable"]
            if host["cgroup_cpu_quota"]:
                threads = max(1, min(threads, int(host["cgroup_cpu_quota"])))
            rm = cpu_rate(blob_s, off_s, lens_s, flows, max(args.cpu_seconds / 2, 1.0), threads=threads)
            out["cpu_baseline_all_cores"] = {"value": round(rm["gbps"], 3), "unit": "GB/s", "cores": rm["cores"],
                                             "mpkt_s": round(rm["mpkt_s"], 2), **host}
    if rank == 0 and world == 1 and extras and name == "c2_tcp1500":
        # the other BASELINE configs on this GPU (per-GPU shards of C4 / C5), each with its own roofline
        c3, e, _, _ = rx_extra("c3_udp64", dev, stream, steps=40, warmup=4, rotate=8)
        c3b, e, _, _ = rx_extra("c3_udp64", dev, stream, steps=40, warmup=4, rotate=8, dst_ip=False)
        c3["compact_20B_results"] = {k: c3b[k] for k in ("gbps", "mpkt_s", "kernel_ms_avg", "roofline")}
        c3r, e, _, _ = rx_extra("c3_udp64_random_ports", dev, stream, steps=40, warmup=4, rotate=8)
        c3["random_ports"] = {k: c3r[k] for k in ("workload", "gbps", "mpkt_s", "kernel_ms_avg", "roofline")}
        out["c3_udp64"] = c3
        del e
        # C1's shape (the reference's own CPU-runnable case: 1078 B frames, one 4-tuple to port 12345) on the GPU; 3
        # rotating batches (141 MB each) so they do not sit in the 256 MB MALL
        try:
            out["c1_tcp1078"], e, _, _ = rx_extra("c1_tcp1078", dev, stream, rotate=3)
            del e
        except Exception as exc:  # noqa: BLE001 — an extra field must not cost the headline line; the error is reported
            out["c1_tcp1078"] = {"error": repr(exc)}
        # the record the Rust LibOS binding consumes (deliver() needs seq / ack / window, and the
        # option list on SYNs): C2 with tcp_fields and tcp_opts, 36 B of results per frame
        out["c2_libos_record"], e, _, _ = rx_extra("c2_tcp1500", dev, stream, tcp_fields=True)
        out["c2_libos_record"]["workload"] += " (LibOS record: + tcp_seq/ack/win, tcp_opts)"
        del e
        # IMIX rotates 2 distinct batches (1.7 GB): one 830 MB batch re-read every step gains 3-6 % from the 256 MB
        # MALL / translation caches; the one-batch figure is kept beside it
        c4, e, _, _ = rx_extra("c4_imix", dev, stream, rotate=2)
        del e
        c4b, e, _, _ = rx_extra("c4_imix", dev, stream, rotate=1)
        c4["one_batch"] = {k: c4b[k] for k in ("gbps", "mpkt_s", "kernel_ms_avg", "roofline")}
        out["c4_imix"] = c4
        del e
        out["c5_device"], e5, b5, f5 = rx_extra("c5_tcp1500_10k", dev, stream)
        # C5 end to end: the per-GPU shard in pinned host memory -> HBM -> kernel -> results to pinned host memory
        out["c5_host_path"] = host_path_rate(e5, b5, f5, b5.n)
        out["c5_host_path"]["workload"] = WORKLOADS["c5_tcp1500_10k"][0]
        out["c5_zero_copy"] = zero_copy_rate(e5, b5, f5, b5.n)
        out["c5_zero_copy"]["workload"] = WORKLOADS["c5_tcp1500_10k"][0]
        del e5, b5
        # DPDK-style zero-copy ingest: 1500 B frames in 2 KiB mbuf slots in page-locked host memory, read by the
        # kernel over PCIe through the mapped address (no staging copy)
        out["mbuf_zero_copy"] = mbuf_zero_copy_rate(dev, stream)
        # host-resident path (NIC ring / socket buffer in pinned host memory) on a C2 slice, and the TPACKET_V3 ring
        out["host_path"] = host_path_rate(eng, batch, flows, args.host_frames)
        out["ring_path"] = ring_path_rate(eng, batch, flows, args.host_frames)
        # TX checksum fill (dk_tx_checksum) over the same batch (rewrites its checksum fields)
        out["tx_checksum"] = tx_rate(eng, batch, frame_bytes, stream)
        out["tx_checksum"]["traffic"] = load_traffic_profile(name + "_tx")
        out["tcp_rx"] = tcp_rate(stream)
        # few connections with many segments each (the wave-per-connection walk)
        out["tcp_rx_64conns"] = tcp_rate(stream, 1 << 20, 64, cpu_seconds=1.0)
        # one connection with 1M in-order segments (a single LAN stream: no reordering) and a 1 GiB receive window
        # (the largest TCP window scaling allows, RFC 7323): ~70 % delivered in order, the ~29 % past the window
        # classified out of window in the key pass and never walked
        out["tcp_rx_1conn"] = tcp_rate(stream, 1 << 20, 1, cpu_seconds=1.0, buffer_size=1 << 30, reorder=0.0)
        out["tcp_rx_1conn"]["stream"] = ("in order (reorder 0), 1 GiB window: the definition since round 5 (round 4 "
                                         "timed a reordered stream whose 64 KiB window filled early; not comparable)")
    if rank == 0:
        print(json.dumps(out), flush=True)
    if comm is not None and hasattr(comm, "destroy"):
        comm.destroy()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
