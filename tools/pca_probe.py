#!/usr/bin/env python3
"""`--pca` through psk_pca_fit and psk_pca_transform on 0/1 designs of n = 256, 1024, 4096 samples and p = 1,000 and 100,000
columns, drawn as tools/gen_pca_golden.py draws its designs (every third column copies one of three latent sample groups with
10 % noise, the others are Bernoulli(0.35)).  pca_fit computes all min(n, p) components; pca_transform scores every training row
under the leading components with explained variance > 0.9, 64 of them at most (what a t-test filter leaves is fewer).  After a warm-up call of each shape, REPS calls are timed by a host clock
around the call (each call ends in a stream synchronise, so this is upload + kernels + read-back, not kernel time); the median,
the spread and the sweeps of the eigen-solver are printed.  With --cpu it times scikit-learn's StandardScaler().fit_transform +
PCA().fit and their transform on the same designs instead (on the cores the process is granted), as the baseline; no GPU needed.
usage: tools/pca_probe.py [--cpu] [--reps R] [n:p ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5


def design(n, p, seed=11):
    rng = np.random.default_rng(seed)
    group = rng.integers(0, 3, n)
    X = (rng.random((n, p), dtype=np.float32) < 0.35).astype(np.float32)
    for j in range(0, p, 3):
        X[:, j] = (group == (j // 3) % 3) ^ (rng.random(n) < 0.10)
    return X


def timed(call, reps):
    """(median, min, max) in ms of `reps` calls after one warm-up call."""
    call()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ms)), min(ms), max(ms)


args = sys.argv[1:]
cpu = "--cpu" in args
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else REPS
shapes = [tuple(int(v) for v in a.split(":")) for a in args if ":" in a] or [(n, p) for p in (1000, 100000) for n in (256, 1024, 4096)]
if cpu:
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    for n, p in shapes:
        X = design(n, p).astype(np.float64)
        made = {}

        def fit():
            made["s"] = StandardScaler().fit(X)
            made["p"] = PCA().fit(made["s"].transform(X))
        print("scikit-learn StandardScaler + PCA n=%d p=%d: fit median %.1f ms (%.1f..%.1f), solver %s"
              % ((n, p) + timed(fit, reps) + (made["p"]._fit_svd_solver,)), flush=True)
        print("scikit-learn StandardScaler + PCA n=%d p=%d: transform median %.1f ms (%.1f..%.1f)"
              % ((n, p) + timed(lambda: made["p"].transform(made["s"].transform(X)), reps)), flush=True)
    sys.exit(0)

from phenotypeseeker_amd.engine import PskContext  # noqa: E402

with PskContext(0) as ctx:
    for n, p in shapes:
        X = design(n, p)
        r = ctx.pca_fit(X)
        print("psk_pca_fit n=%d p=%d: %d components, %d sweeps, median %.1f ms (%.1f..%.1f)"
              % ((n, p, len(r["lambda"]), r["sweeps"]) + timed(lambda: ctx.pca_fit(X), reps)), flush=True)
        keep = r["lambda"] / (n - 1) > 0.9
        comp = r["components"][keep][:64]
        print("psk_pca_transform n=%d p=%d: %d components, median %.1f ms (%.1f..%.1f)"
              % ((n, p, len(comp)) + timed(lambda: ctx.pca_transform(X, r["mean"], r["scale"], comp), reps)), flush=True)
