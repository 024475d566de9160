#!/usr/bin/env python3
"""`-bc XGBC` / `-reg XGBR` through psk_gb_fit and psk_gb_decision on 0/1 designs of (n, p) = (256, 1000) and (2048, 1000) drawn
as tools/nb_probe.py draws its own, with scikit-learn's defaults (100 stages, learning rate 0.1, depth 3), both losses: one fit on
all samples, the 11 fits of a `-cv1 10` run in one call (10 folds held out in turn + all samples), and psk_gb_decision of the
all-sample model on every row.  After a warm-up call of each shape, REPS calls are timed by a host clock around the call (each
call ends in a stream synchronise, so this is upload + pack + kernel + read-back, not kernel time); the median and the spread are
printed.  Run it under `rocprofv3 --kernel-trace --stats` for the durations of gb_fit_kernel and gb_decision_kernel
(docs/NOTEBOOK.md).  With --cpu it times scikit-learn's GradientBoostingClassifier() / GradientBoostingRegressor() on the same
designs instead -- one fit and its predictions of every row -- for scale only (no GPU needed).  With --counts it times the 11 fits
of a `-cv1 10` run (n = 256 unless given) twice: through psk_gb_fit_counts on a count design of about 4 distinct values a column,
and through psk_gb_fit on the same design binarised; it prints both with the number of threshold planes, P, the count kernel
scanning P planes where the 0/1 kernel scans p columns.
usage: tools/gb_probe.py [--cpu | --counts] [n ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FOLDS, REPS = 10, 5


def design(n, p=1000, seed=7):
    rng = np.random.default_rng(seed)
    X = (rng.random((n, p)) < rng.uniform(.1, .9, p)).astype(np.float64)
    z = X[:, :6].sum(axis=1) + rng.normal(0.0, 1.0, n)
    return X, (z, (z > 3).astype(np.float64))


def count_design(n, p=1000, seed=7):
    """design()'s presence pattern times a copy number in 1 .. 3: the values 0 .. 3 in a column."""
    rng = np.random.default_rng(seed + 1)
    X = design(n, p, seed)[0] * rng.choice([1, 1, 2, 3], (n, p))
    z = X[:, :3].sum(axis=1) + (X[:, 3:6] >= 2).sum(axis=1) + rng.normal(0.0, 1.0, n)
    return X, (z, (z > np.median(z)).astype(np.float64))


def timed(call, reps=REPS):
    """(median, min, max) in ms of `reps` calls after one warm-up call."""
    call()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ms)), min(ms), max(ms)


from phenotypeseeker_amd import cv  # noqa: E402
from phenotypeseeker_amd.model_gb import init_raw_prediction  # noqa: E402

args = sys.argv[1:]
cpu, counts = "--cpu" in args, "--counts" in args
sizes = [int(a) for a in args if not a.startswith("--")] or ([256] if counts else [256, 2048])
NAMES = ("squared_error", "log_loss")
if cpu:
    from sklearn.ensemble import GradientBoostingClassifier, GradientBoostingRegressor
    for n in sizes:
        X, ys = design(n)
        for loss, name in enumerate(NAMES):
            y = ys[loss] if loss == 0 else ys[loss].astype(np.int64)
            est = (GradientBoostingClassifier if loss else GradientBoostingRegressor)(random_state=0)
            print("scikit-learn %s n=%d p=1000: one fit median %.1f ms (%.1f..%.1f)" % ((type(est).__name__, n) + timed(lambda: est.fit(X, y), 2)),
                  flush=True)
            print("scikit-learn %s n=%d p=1000: predictions of every row median %.2f ms (%.2f..%.2f)"
                  % ((type(est).__name__, n) + timed(lambda: est.predict(X))), flush=True)
    sys.exit(0)

from phenotypeseeker_amd.engine import PskContext  # noqa: E402

if counts:
    with PskContext(0) as ctx:
        for n in sizes:
            X, ys = count_design(n)
            P = int(sum(len(np.unique(X[:, j])) - 1 for j in range(X.shape[1])))
            held = list(range(FOLDS)) + [-1]
            for loss, name in enumerate(NAMES):
                y = ys[loss]
                folds = cv.stratified_kfold(y.astype(np.int64), FOLDS) if loss else cv.kfold(n, FOLDS)
                init = [init_raw_prediction(y[folds != f], name) for f in held]
                on_counts = lambda: ctx.gb_fit_counts(X, y, folds, held, name, 100, 0.1, 3, init, staged=False)
                on_bits = lambda: ctx.gb_fit((X > 0).astype(np.float32), y, folds, held, name, 100, 0.1, 3, init, staged=False)
                print("psk_gb_fit_counts %s n=%d p=1000 P=%d: %d fits of 100 stages median %.2f ms (%.2f..%.2f)"
                      % ((name, n, P, len(held)) + timed(on_counts)), flush=True)
                print("psk_gb_fit        %s n=%d p=1000 (binarised): %d fits of 100 stages median %.2f ms (%.2f..%.2f)"
                      % ((name, n, len(held)) + timed(on_bits)), flush=True)
                f = on_counts()[-1]
                print("  nodes per tree %.1f; splits above 0.5: %d of %d" % (f["node_count"].mean(), int((f["threshold"] > 0.5).sum()),
                                                                            int((f["nodes"][:, :, 1] > 0).sum())), flush=True)
    sys.exit(0)

with PskContext(0) as ctx:
    for n in sizes:
        X, ys = design(n)
        X32 = X.astype(np.float32)
        for loss, name in enumerate(NAMES):
            y = ys[loss]
            folds = cv.stratified_kfold(y.astype(np.int64), FOLDS) if loss else cv.kfold(n, FOLDS)
            for held in ([-1], list(range(FOLDS)) + [-1]):
                init = [init_raw_prediction(y[folds != f], name) for f in held]
                fit = lambda: ctx.gb_fit(X32, y, folds, held, name, 100, 0.1, 3, init, staged=False)
                print("psk_gb_fit %s n=%d p=1000: %d fit(s) of 100 stages median %.2f ms (%.2f..%.2f)"
                      % ((name, n, len(held)) + timed(fit)), flush=True)
            f = fit()[-1]
            dec = lambda: ctx.gb_decision(X32, f["node_count"], f["nodes"], f["value"], init[-1], 0.1, 3)
            print("psk_gb_decision %s n=%d p=1000: every row median %.3f ms (%.3f..%.3f)" % ((name, n) + timed(dec)), flush=True)
            raw = dec()
            assert np.array_equal(raw, f["raw"])
            print("  nodes per tree %.1f; training %s %.4f" % (f["node_count"].mean(), "accuracy" if loss else "mean squared error",
                                                              np.mean((raw >= 0) == (y == 1)) if loss else np.mean((y - raw) ** 2)), flush=True)
