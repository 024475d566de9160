#!/usr/bin/env python3
"""The reference's default `-bc RF` search -- RandomizedSearchCV(RandomForestClassifier(random_state=0), the seven-key grid,
n_iter=25, cv=10, random_state=0) and the refit of the best candidate -- through model.RandomizedSearch / psk_forest_fit on
synthetic 0/1 designs of (n, p) = (256, 1000) and (2048, 1000), drawn as tools/tree_grid_probe.py draws its own.  Prints the
wall-clock of the search, the share of it spent inside psk_forest_fit calls (uploads, both kernels, downloads) and on the
host's RandomState draws, the number of trees, and the scores, so that a run can be laid next to scikit-learn's: with --cpu it
times scikit-learn's own search with the same seed on the same designs instead (no GPU needed) and prints the same lines.  With
--counts the designs hold k-mer counts and the fits go through psk_forest_fit_counts.
usage: tools/forest_grid_time.py [--cpu] [--counts] [--n_iter K] [n ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from phenotypeseeker_amd.modeling import RF_GRID  # noqa: E402

SEED, FOLDS = 0, 10


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


def report(tag, n, secs, results, best):
    trees = sum(q["n_estimators"] for q in results["params"]) * FOLDS + best["n_estimators"]
    print("%s n=%d p=1000: %d candidates x %d folds + refit = %d trees in %.2f s" % (tag, n, len(results["params"]), FOLDS, trees, secs))
    print("  mean scores %s" % " ".join("%.4f" % v for v in results["mean_test_score"]))
    print("  best %s" % sorted(best.items()), flush=True)


args = sys.argv[1:]
cpu, counts = "--cpu" in args, "--counts" in args
if counts:
    design = count_design
n_iter = int(args[args.index("--n_iter") + 1]) if "--n_iter" in args else 25
sizes = [int(a) for i, a in enumerate(args) if a.isdigit() and args[i - 1] != "--n_iter"] or [256, 2048]
if cpu:
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import RandomizedSearchCV
    for n in sizes:
        X, y = design(n)
        t = time.perf_counter()
        g = RandomizedSearchCV(RandomForestClassifier(random_state=SEED), RF_GRID, n_iter=n_iter, cv=FOLDS, random_state=SEED).fit(X, y)
        report("scikit-learn RandomizedSearchCV(RandomForestClassifier)", n, time.perf_counter() - t, g.cv_results_, g.best_params_)
    sys.exit(0)

from phenotypeseeker_amd import model as M  # noqa: E402
from phenotypeseeker_amd.engine import PskContext  # noqa: E402


class Timed:
    """The context with its forest_fit calls timed."""

    def __init__(self, ctx):
        self.ctx, self.secs, self.calls, self.trees = ctx, 0.0, 0, 0

    def _timed(self, fit, *a, **kw):
        t = time.perf_counter()
        out = fit(*a, **kw)
        self.secs += time.perf_counter() - t
        self.calls += 1
        self.trees += len(a[3])
        return out

    def forest_fit(self, *a, **kw):
        return self._timed(self.ctx.forest_fit, *a, **kw)

    def forest_fit_counts(self, *a, **kw):
        return self._timed(self.ctx.forest_fit_counts, *a, **kw)


with PskContext(0) as ctx:
    X, y = design(64, 50)
    M.RandomForest(n_estimators=2, counts=counts).fit(X, y, ctx)   # code objects
    for n in sizes:
        X, y = design(n)
        timed = Timed(ctx)
        t = time.perf_counter()
        rs = M.RandomizedSearch(M.RandomForest(random_state=SEED, counts=counts), RF_GRID, n_iter, FOLDS, random_state=SEED).fit(X, y, timed)
        secs = time.perf_counter() - t
        report("psk_forest_fit_counts" if counts else "psk_forest_fit", n, secs, rs.cv_results_, rs.best_params_)
        if counts:
            print("  %d threshold planes, %.1f MB on the device per call" % (planes(X)[0], planes(X)[1] / 1e6))
        print("  %.2f s in %d psk_forest_fit calls (%d trees), %.2f s on the host (RandomState draws, weights, scoring)"
              % (timed.secs, timed.calls, timed.trees, secs - timed.secs), flush=True)
