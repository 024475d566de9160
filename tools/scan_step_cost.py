#!/usr/bin/env python3
"""Host cost of one scan step: median microseconds spent inside chi2_scan_begin and inside scan_end, with two scans in
flight as in bench.py's run_steps, on bench.py's flagship matrix (256 x 5-Mbp genomes, k = 13, unit weights,
Bonferroni cut-off).  Prints one JSON line.

    python3 tools/scan_step_cost.py [--steps 4000] [--samples 256] [--length 5000000] [--kmer 13]

begin_us is what the host pays to queue a scan; end_us holds the wait for the oldest scan, so it is the host's own
work only when the GPU is ahead of the host.  step_us is the wall-clock of the loop divided by its steps."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--length", type=int, default=5_000_000)
    ap.add_argument("--kmer", type=int, default=13)
    args = ap.parse_args()
    from phenotypeseeker_amd.engine import PskContext
    from phenotypeseeker_amd.synth import GenomeSet

    n, k = args.samples, args.kmer
    gs = GenomeSet(n, args.length, seed=12345)
    with PskContext(0) as ctx:
        ctx.begin(k, n)
        for lo in range(0, n, 64):
            ctx.count_kmers_batch(lo, [gs.sample(i)[1] for i in range(lo, min(lo + 64, n))], 8)
        m = ctx.build_presence()
        pheno = np.array([1 if i % 2 == 0 else 0 for i in range(n)], dtype=np.int8)
        scan_args = (pheno, None, 2, n - 2, 0.05, False, m)
        ctx.chi2_scan(*scan_args)
        ctx.rescan_timed(300)          # clocks settled, as bench.py does before its steps
        now = time.perf_counter_ns
        begin_ns, end_ns, kernel_ms = [], [], []
        npass = 0
        for _ in range(2):
            ctx.chi2_scan_begin(*scan_args)
        t_loop = now()
        for i in range(args.steps):
            t0 = now()
            npass = ctx.scan_end()
            t1 = now()
            kernel_ms.append(ctx.last_scan_ms())
            end_ns.append(t1 - t0)
            if i + 2 < args.steps:
                t0 = now()
                ctx.chi2_scan_begin(*scan_args)
                begin_ns.append(now() - t0)
        t_loop = now() - t_loop
        skip = min(len(begin_ns) // 10, 100)      # the first steps: the queue is not in its steady state yet
        out = {"tool": "scan_step_cost", "rows": int(m), "samples": n, "k": k, "steps": args.steps, "survivors": int(npass),
               "begin_us_p50": float(np.median(begin_ns[skip:])) / 1e3, "begin_us_p95": float(np.percentile(begin_ns[skip:], 95)) / 1e3,
               "end_us_p50": float(np.median(end_ns[skip:])) / 1e3, "end_us_p95": float(np.percentile(end_ns[skip:], 95)) / 1e3,
               "step_us": t_loop / args.steps / 1e3, "kernel_us_p50": float(np.median(kernel_ms[skip:])) * 1e3,
               "lib": os.environ.get("PSK_LIB") or "in-tree"}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
