#!/usr/bin/env python3
"""The grid search of `-bc DT` (max_depth 1..10 x {gini, entropy} x 10 folds + 20 refits = 220 fits) through psk_tree_fit,
next to psk_logreg_l1_fit (13 values of C, 143 fits) on the same designs: 0/1 designs of (n, p) = (256, 1000) and
(2048, 1000) drawn as tools/gen_tree_golden.py draws its own.  Prints wall-clock and tree sizes; run it under
`rocprofv3 --kernel-trace --stats` for the durations of tree_pack_kernel and tree_fit_kernel (docs/NOTEBOOK.md).  With --cpu
it times scikit-learn's GridSearchCV(DecisionTreeClassifier(), ...) on the same designs instead (no GPU needed).
usage: tools/tree_grid_probe.py [--cpu] [n ...]"""
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


args = sys.argv[1:]
cpu = "--cpu" in args
sizes = [int(a) for a in args if a != "--cpu"] or [256, 2048]
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
        ctx.tree_fit(X, y, folds, fd[:2], fc[:2], ff[:2])   # code objects
        t = time.perf_counter()
        fits = ctx.tree_fit(X, y, folds, fd, fc, ff)
        nodes = [f["node_count"] for f in fits]
        print("psk_tree_fit n=%d p=1000: %d fits in %.1f ms, %d..%d nodes (%d in all)"
              % (n, len(fits), 1e3 * (time.perf_counter() - t), min(nodes), max(nodes), sum(nodes)), flush=True)
        Cs = [float(1.0 / a) for a in np.logspace(-3, 3, 13)]
        fp = [C for C in Cs for _ in range(FOLDS)] + Cs
        lf = [f for _ in Cs for f in range(FOLDS)] + [-1] * len(Cs)
        ctx.logreg_l1_fit(X, y, folds, fp[:2], lf[:2], 1e-4, 10)
        t = time.perf_counter()
        ctx.logreg_l1_fit(X, y, folds, fp, lf, 1e-4, 1000)
        print("psk_logreg_l1_fit n=%d p=1000: %d fits in %.1f ms" % (n, len(fp), 1e3 * (time.perf_counter() - t)), flush=True)
