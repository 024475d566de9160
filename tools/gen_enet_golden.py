#!/usr/bin/env python3
"""Writes tests/golden/enet_kat.npz: scikit-learn's ElasticNet(tol=1e-4, max_iter=1000) on the designs of
tests/enet_restated.py -- per design and l1_ratio every alpha on all rows and on two held-out folds (coef_, intercept_,
n_iter_), and one GridSearchCV(cv=10) with its split scores, best alpha and refit.  Needs scikit-learn (the fixture records
its version); the tests need only the .npz.

A case is kept only if, in the restatement (enet_restated.enet_fit), every evaluated gap differs from tol y'y and every
sweep's d_w_max / w_max from tol by more than 1e-6 of the threshold, and the restatement reproduces scikit-learn's n_iter_
and support: the device adds in another order, and a stop decision balanced on rounding could end a sweep apart.  A design
that has such a case is drawn again with the next seed; the seeds used are printed and recorded.
usage: tools/gen_enet_golden.py"""
import os
import sys
import warnings

import numpy as np
import sklearn
from sklearn.linear_model import ElasticNet
from sklearn.model_selection import GridSearchCV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import enet_restated as R  # noqa: E402

warnings.filterwarnings("ignore")      # (ConvergenceWarning: fits cut off at max_iter are part of the fixture)


def fit_ok(X, y, alpha, ratio, sk):
    """The conditions of the module docstring for one fit; sk: the fitted scikit-learn estimator."""
    trace = []
    w, b, it = R.enet_fit(X, y, alpha, ratio, R.TOL, R.MAX_ITER, trace)
    scale = max(np.abs(sk.coef_).max(), 1e-300)
    return (it == int(sk.n_iter_) and np.array_equal(w != 0, sk.coef_ != 0) and np.abs(w - sk.coef_).max() <= 1e-9 * scale
            and R.decisions_clear(trace))


def calls_of(X, y, fold, ratios):
    """[{l1_ratio, alpha, held, coef, icpt, n_iter}] or None when a fit fails the conditions."""
    out = []
    alphas, held = R.plan()
    for ratio in ratios:
        coef, icpt, n_iter = [], [], []
        for a, h in zip(alphas, held):
            tr = fold != h
            sk = ElasticNet(alpha=a, l1_ratio=ratio, tol=R.TOL, max_iter=R.MAX_ITER).fit(X[tr], y[tr])
            if not fit_ok(X[tr], y[tr], a, ratio, sk):
                return None
            coef.append(sk.coef_.copy())
            icpt.append(float(sk.intercept_))
            n_iter.append(int(sk.n_iter_))
        out.append(dict(l1_ratio=ratio, alpha=np.array(alphas), held=np.array(held, dtype=np.int32), coef=np.stack(coef),
                        icpt=np.array(icpt), n_iter=np.array(n_iter, dtype=np.int32)))
    return out


def grid_search(X, y, fold):
    """The recorded GridSearchCV, or None when one of its fits fails the conditions."""
    gs = GridSearchCV(ElasticNet(l1_ratio=R.GS_RATIO, tol=R.TOL, max_iter=R.MAX_ITER), {"alpha": list(R.ALPHAS)}, cv=R.N_FOLDS).fit(X, y)
    for a in R.ALPHAS:
        for h in range(R.N_FOLDS):
            tr = fold != h
            sk = ElasticNet(alpha=a, l1_ratio=R.GS_RATIO, tol=R.TOL, max_iter=R.MAX_ITER).fit(X[tr], y[tr])
            if not fit_ok(X[tr], y[tr], a, R.GS_RATIO, sk):
                return None
    scores = np.array([gs.cv_results_["split%d_test_score" % f] for f in range(R.N_FOLDS)]).T
    be = gs.best_estimator_
    return dict(gs_l1_ratio=R.GS_RATIO, gs_alphas=np.array(R.ALPHAS), gs_split_scores=scores, gs_best_alpha=float(gs.best_params_["alpha"]),
                gs_coef=be.coef_.copy(), gs_icpt=float(be.intercept_))


def main():
    out = dict(sklearn_version=sklearn.__version__, tol=R.TOL, max_iter=R.MAX_ITER, n_designs=len(R.SHAPES))
    for d, (n, p, counts) in enumerate(R.SHAPES):
        ratios = list(R.RATIOS) + ([0.0] if (n, p, counts) == R.RATIO_ZERO_SHAPE else [])
        fold = R.kfold(n)
        for seed in range(1000):
            X, y = R.design(n, p, counts, seed)
            X = X.astype(np.float32).astype(np.float64)
            calls = calls_of(X, y, fold, ratios)
            gs = grid_search(X, y, fold) if calls is not None and (n, p, counts) == R.GS_SHAPE else {}
            if calls is not None and gs is not None:
                break
            print("%d x %d%s: seed %d has a stop decision within the margin, or the restatement leaves scikit-learn's path"
                  % (n, p, " counts" if counts else "", seed), flush=True)
        else:
            raise SystemExit("no seed below 1000 for %d x %d" % (n, p))
        print("%d x %d%s: seed %d, sweeps %s" % (n, p, " counts" if counts else "", seed,
                                                  " | ".join(" ".join(str(v) for v in c["n_iter"]) for c in calls)), flush=True)
        assert X.max() <= 255 and np.array_equal(X, np.round(X))
        out["shape%d" % d] = np.array([n, p, int(counts)])
        out["seed%d" % d] = seed
        out["X%d" % d] = X.astype(np.uint8) if counts else np.packbits(X.astype(np.uint8), axis=1)
        out["y%d" % d] = y
        out["fold%d" % d] = fold
        out["ratios%d" % d] = np.array(ratios)
        for k, c in enumerate(calls):
            for key in ("alpha", "held", "coef", "icpt", "n_iter"):
                out["%s_%d_%d" % (key, d, k)] = c[key]
        if gs:
            out.update(gs, gs_design=d)
    path = os.path.join(ROOT, "tests", "golden", "enet_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
