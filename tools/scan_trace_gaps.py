#!/usr/bin/env python3
"""From a rocprofv3 --kernel-trace CSV of `bench.py --steps K`: the median duration of the scan kernel and the median
gap between consecutive scans (start of scan i + 1 minus end of scan i) over the last K dispatches -- bench.py's timed
region, which ends the run.  Prints one JSON line.

    python3 tools/scan_trace_gaps.py <..._kernel_trace.csv> [K=200] [kernel name part=chi2_scan_kernel_cx]"""
import csv
import json
import sys

import numpy as np


def main():
    path = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    part = sys.argv[3] if len(sys.argv) > 3 else "chi2_scan_kernel_cx"
    rows, others = [], 0
    with open(path) as f:
        for r in csv.DictReader(f):
            if part in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
            else:
                others += 1
    rows.sort()
    timed = rows[-steps:]
    dur = np.array([e - s for s, e in timed]) / 1e3
    gap = np.array([timed[i + 1][0] - timed[i][1] for i in range(len(timed) - 1)]) / 1e3
    pct = lambda a, q: float(np.percentile(a, q)) if len(a) else None
    print(json.dumps({"trace": path, "kernel": part, "dispatches_in_trace": len(rows), "other_dispatches": others, "timed": len(timed),
                      "kernel_us_p50": pct(dur, 50), "kernel_us_min": pct(dur, 0), "kernel_us_p95": pct(dur, 95),
                      "gap_us_p50": pct(gap, 50), "gap_us_min": pct(gap, 0), "gap_us_p95": pct(gap, 95),
                      "period_us_p50": pct(dur[:-1] + gap, 50) if len(gap) else None}))


if __name__ == "__main__":
    main()
