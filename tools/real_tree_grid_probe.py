#!/usr/bin/env python3
"""The two searches of `--pca` with -bc DT / -bc RF on a real-valued design, through psk_tree_fit_real / psk_forest_fit_real:
the 220-fit grid of -bc DT (max_depth 1..10 x {gini, entropy} x 10 folds + 20 refits) and one randomized search of -bc RF
at --n_iter 4 (seed 0, 10 folds, the reference's grid), on a 2,048 x 200 float32 Gaussian design with a planted signal.  With
--counts the same two searches go through psk_tree_fit_counts / psk_forest_fit_counts on the RANK-CODED design (each column
replaced by its ranks 0 .. n - 1: the same partitions, one threshold plane per gap, which fits under PSK_TREE_PLANE_CAP at
this size).  Prints wall-clock, tree sizes and the best parameters; run it under `rocprofv3 --kernel-trace --stats` for the
durations of real_sort_kernel, rtree_fit_kernel, rforest_fit_kernel and their count counterparts (docs/NOTEBOOK.md).
usage: tools/real_tree_grid_probe.py [--counts] [n [p]]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phenotypeseeker_amd import cv, model as M  # noqa: E402
from phenotypeseeker_amd.engine import PskContext  # noqa: E402
from phenotypeseeker_amd.modeling import RF_GRID  # noqa: E402

DEPTHS, CRITERIA, FOLDS, N_ITER, SEED = list(range(1, 11)), ["gini", "entropy"], 10, 4, 0


def design(n, p, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 1.0, (n, p)).astype(np.float32)
    y = (X[:, 0] + 0.8 * X[:, 1] + np.where(X[:, 2] > 0.5, 1.0, -1.0) + rng.normal(0.0, 1.0, n) > 0).astype(np.int64)
    return X.astype(np.float64), y


args = sys.argv[1:]
counts = "--counts" in args
sizes = [int(a) for a in args if a.isdigit()]
n, p = (sizes + [2048, 200])[:2] if len(sizes) != 1 else (sizes[0], 200)
X, y = design(n, p)
if counts:
    X = np.argsort(np.argsort(X, axis=0, kind="stable"), axis=0).astype(np.float64)
    print("rank-coded: %d threshold planes" % sum(len(np.unique(X[:, j])) - 1 for j in range(p)), flush=True)

with PskContext(0) as ctx:
    tree_fit = ctx.tree_fit_counts if counts else ctx.tree_fit_real
    name = ("psk_tree_fit_counts", "psk_forest_fit_counts") if counts else ("psk_tree_fit_real", "psk_forest_fit_real")
    folds = cv.stratified_kfold(y, FOLDS)
    cand = [(d, c) for c in CRITERIA for d in DEPTHS]
    fd = [d for d, _ in cand for _ in range(FOLDS)] + [d for d, _ in cand]
    fc = [c for _, c in cand for _ in range(FOLDS)] + [c for _, c in cand]
    ff = [f for _ in cand for f in range(FOLDS)] + [-1] * len(cand)
    tree_fit(X, y, folds, fd[:2], fc[:2], ff[:2])   # code objects
    t = time.perf_counter()
    fits = tree_fit(X, y, folds, fd, fc, ff)
    nodes = [f["node_count"] for f in fits]
    print("%s n=%d p=%d: %d fits in %.1f ms, %d..%d nodes (%d in all)"
          % (name[0], n, p, len(fits), 1e3 * (time.perf_counter() - t), min(nodes), max(nodes), sum(nodes)), flush=True)
    est = M.RandomForest(random_state=SEED, counts=counts, real=not counts)
    M.RandomForest(n_estimators=2, random_state=SEED, counts=counts, real=not counts).fit(X, y, ctx)   # code objects
    t = time.perf_counter()
    rs = M.RandomizedSearch(est, RF_GRID, N_ITER, FOLDS, random_state=SEED).fit(X, y, ctx)
    trees = sum(q["n_estimators"] for q in rs.cv_results_["params"]) * FOLDS + rs.best_params_["n_estimators"]
    print("%s n=%d p=%d: search of %d candidates x %d folds + refit, %d trees, in %.1f ms; means %s, best %s"
          % (name[1], n, p, N_ITER, FOLDS, trees, 1e3 * (time.perf_counter() - t), np.round(rs.cv_results_["mean_test_score"], 4),
             rs.best_params_), flush=True)
