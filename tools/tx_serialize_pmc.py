#!/usr/bin/env python3
"""HBM traffic of the in-place TX fill and of dk_tx_serialize per frame, from two rocprofv3 counter passes over
tools/tx_serialize_ab.py (one counter per pass, no tracing beside it; run on the GPU box from the repo root):

    K="dk_tx_serialize_kernel|dk_tx_split_kernel"
    rocprofv3 --pmc FETCH_SIZE --kernel-include-regex "$K" -T -d OUT/pmc_fetch -o run --output-format csv -- \
        python tools/tx_serialize_ab.py --iters 2 --reps 1 --preheat-seconds 0
    rocprofv3 --pmc WRITE_SIZE --kernel-include-regex "$K" -T -d OUT/pmc_write -o run --output-format csv -- \
        python tools/tx_serialize_ab.py --iters 2 --reps 1 --preheat-seconds 0
    python tools/tx_serialize_pmc.py OUT [--frames 1048576] > profiles/tx_serialize_pmc.csv

Per kernel and counter: launches, the mean counter value (KB) and bytes per frame. FETCH_SIZE counts half the bytes on
gfx950 (tools/summarize_profile.py calibrates the same factor against the read probe); WRITE_SIZE is as counted.
"""
import argparse
import collections
import csv
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--frames", type=int, default=1 << 20)
    a = ap.parse_args()
    w = csv.writer(sys.stdout)
    w.writerow(["kernel", "counter", "launches", "mean_KB", "bytes_per_frame"])
    for sub, counter, unit in (("pmc_fetch", "FETCH_SIZE", 2048.0), ("pmc_write", "WRITE_SIZE", 1024.0)):
        agg = collections.defaultdict(list)
        with open(os.path.join(a.out_dir, sub, "run_counter_collection.csv")) as f:
            for r in csv.DictReader(f):
                if r["Counter_Name"] == counter:
                    agg[r["Kernel_Name"]].append(float(r["Counter_Value"]))
        for k, v in sorted(agg.items()):
            m = sum(v) / len(v)
            w.writerow([k, counter, len(v), round(m, 1), round(m * unit / a.frames, 1)])


if __name__ == "__main__":
    main()
