#!/usr/bin/env python3
"""The grid search of `-bc DT` (max_depth 1..10 x {gini, entropy} x 10 folds + 20 refits = 220 fits) through psk_tree_fit,
next to psk_logreg_l1_fit (13 values of C, 143 fits) on the same designs: 0/1 designs of (n, p) = (256, 1000) and
(2048, 1000) drawn as tools/gen_tree_golden.py draws its own.  Prints wall-clock and tree sizes; run it under
`rocprofv3 --kernel-trace --stats` for the durations of tree_pack_kernel and tree_fit_kernel (docs/NOTEBOOK.md).  With --cpu
it times scikit-learn's GridSearchCV(DecisionTreeClassifier(), ...) on the same designs instead (no GPU needed).  With --counts
the designs hold k-mer counts and the fits go through psk_tree_fit_counts (the logistic regression is left out).
usage: tools/tree_grid_probe.py [--cpu] [--counts] [n ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEPTHS, CRITERIA, FOLDS = list(range(1, 11)), ["gini", "entropy"], 10


def design(n, p=1000, seed=7):
    rng = np.random.default_rng(seed)
    X = (rng.random((n, p)) < rng.uniform(.1, .9, p)).astype(np.float64)
    y = (X[:, :6].sum(axis=1) + rng.normal(0.0, 1.0, n) > 3).astype(np.int64)
    return X, y


def count_design(n, p=1000, seed=7):
    """The same shape as k-mer counts (tools/gen_count_tree_golden.py's family): Poisson(lambda_j), lambda_j ~ U(0.2, 2.5), 15 % of
    the columns Poisson(30) x Bernoulli(0.7); labels from count thresholds on three columns."""
    rng = np.random.default_rng(seed)
    X = rng.poisson(rng.uniform(0.2, 2.5, p), (n, p)).astype(np.float64)
    heavy = np.nonzero(rng.random(p) < 0.15)[0]
    X[:, heavy] = rng.poisson(30, (n, len(heavy))) * (rng.random((n, len(heavy))) < 0.7)
    y = ((X[:, 0] >= 2).astype(float) + (X[:, 1] >= 3) + (X[:, heavy[0]] > 28) + rng.normal(0.0, 0.6, n) > 1.2).astype(np.int64)
    return X, y


def planes(X):
    """(threshold planes, device bytes of a count call: the planes, the float design and the plane tables; include/psk.h f9)"""
    n, p = X.shape
    P = sum(len(np.unique(X[:, j])) - 1 for j in range(p))
    return P, 8 * ((n + 63) // 64) * P + 4 * n * p + 8 * P + 4 * (p + 1)


args = sys.argv[1:]
cpu, counts = "--cpu" in args, "--counts" in args
sizes = [int(a) for a in args if a.isdigit()] or [256, 2048]
if counts:
    design = count_design
if cpu:
    from sklearn.model_selection import GridSearchCV
    from sklearn.tree import DecisionTreeClassifier
    for n in sizes:
        X, y = design(n)
        t = time.perf_counter()
        g = GridSearchCV(DecisionTreeClassifier(), {"max_depth": DEPTHS, "criterion": CRITERIA}, cv=FOLDS).fit(X, y)
        print("scikit-learn GridSearchCV(DecisionTreeClassifier) n=%d p=1000: 220 fits in %.1f ms, best %s"
              % (n, 1e3 * (time.perf_counter() - t), g.best_params_), flush=True)
    sys.exit(0)

from phenotypeseeker_amd import cv  # noqa: E402
from phenotypeseeker_amd.engine import PskContext  # noqa: E402

with PskContext(0) as ctx:
    for n in sizes:
        X, y = design(n)
        folds = cv.stratified_kfold(y, FOLDS)
        cand = [(d, c) for c in CRITERIA for d in DEPTHS]
        fd = [d for d, _ in cand for _ in range(FOLDS)] + [d for d, _ in cand]
        fc = [c for _, c in cand for _ in range(FOLDS)] + [c for _, c in cand]
        ff = [f for _ in cand for f in range(FOLDS)] + [-1] * len(cand)
        tree_fit = ctx.tree_fit_counts if counts else ctx.tree_fit
        tree_fit(X, y, folds, fd[:2], fc[:2], ff[:2])   # code objects
        t = time.perf_counter()
        fits = tree_fit(X, y, folds, fd, fc, ff)
        nodes = [f["node_count"] for f in fits]
        print("%s n=%d p=1000: %d fits in %.1f ms, %d..%d nodes (%d in all)"
              % ("psk_tree_fit_counts" if counts else "psk_tree_fit", n, len(fits), 1e3 * (time.perf_counter() - t), min(nodes), max(nodes),
                 sum(nodes)), flush=True)
        if counts:
            print("  %d threshold planes, %.1f MB on the device" % (planes(X)[0], planes(X)[1] / 1e6), flush=True)
            continue
        Cs = [float(1.0 / a) for a in np.logspace(-3, 3, 13)]
        fp = [C for C in Cs for _ in range(FOLDS)] + Cs
        lf = [f for _ in Cs for f in range(FOLDS)] + [-1] * len(Cs)
        ctx.logreg_l1_fit(X, y, folds, fp[:2], lf[:2], 1e-4, 10)
        t = time.perf_counter()
        ctx.logreg_l1_fit(X, y, folds, fp, lf, 1e-4, 1000)
        print("psk_logreg_l1_fit n=%d p=1000: %d fits in %.1f ms" % (n, len(fp), 1e3 * (time.perf_counter() - t)), flush=True)
