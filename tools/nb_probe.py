#!/usr/bin/env python3
"""`-bc NB` through psk_nb_fit and psk_nb_jll on 0/1 designs of (n, p) = (256, 1000) and (2048, 1000) drawn as
tools/tree_grid_probe.py draws its own: nb_fit with 11 fits (10 stratified folds held out in turn + all samples) and nb_jll of the
11 models on every row.  After a warm-up call of each shape, REPS calls are timed by a host clock around the call (each call ends
in a stream synchronise, so this is upload + pack + kernels + read-back, not kernel time); the median and the spread are printed.
Run it under `rocprofv3 --kernel-trace --stats` for the durations of tree_pack_kernel, nb_train_kernel, nb_count_kernel and
nb_jll_kernel (docs/NOTEBOOK.md).  With --cpu it times scikit-learn's BernoulliNB on the same designs instead -- 11 fits and
their _joint_log_likelihood on every row -- for scale only (no GPU needed).
usage: tools/nb_probe.py [--cpu] [n ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FOLDS, REPS = 10, 20


def design(n, p=1000, seed=7):
    rng = np.random.default_rng(seed)
    X = (rng.random((n, p)) < rng.uniform(.1, .9, p)).astype(np.float64)
    y = (X[:, :6].sum(axis=1) + rng.normal(0.0, 1.0, n) > 3).astype(np.int64)
    return X, y


def timed(call):
    """(median, min, max) in ms of REPS calls after one warm-up call."""
    call()
    ms = []
    for _ in range(REPS):
        t = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ms)), min(ms), max(ms)


from phenotypeseeker_amd import cv  # noqa: E402

args = sys.argv[1:]
cpu = "--cpu" in args
sizes = [int(a) for a in args if a != "--cpu"] or [256, 2048]
if cpu:
    from sklearn.naive_bayes import BernoulliNB
    for n in sizes:
        X, y = design(n)
        folds = cv.stratified_kfold(y, FOLDS)
        held = list(range(FOLDS)) + [-1]
        models = []

        def fit():
            models[:] = [BernoulliNB().fit(X[folds != f], y[folds != f]) for f in held]
        print("scikit-learn BernoulliNB n=%d p=1000: %d fits median %.2f ms (%.2f..%.2f)" % ((n, len(held)) + timed(fit)), flush=True)
        print("scikit-learn BernoulliNB n=%d p=1000: _joint_log_likelihood of %d models median %.2f ms (%.2f..%.2f)"
              % ((n, len(held)) + timed(lambda: [m._joint_log_likelihood(X) for m in models])), flush=True)
    sys.exit(0)

from phenotypeseeker_amd.engine import PskContext  # noqa: E402
from phenotypeseeker_amd.model import BernoulliNB  # noqa: E402

with PskContext(0) as ctx:
    for n in sizes:
        X, y = design(n)
        X32 = X.astype(np.float32)
        folds = cv.stratified_kfold(y, FOLDS)
        held = list(range(FOLDS)) + [-1]
        fc, cc = ctx.nb_fit(X32, y, folds, held)
        print("psk_nb_fit n=%d p=1000: %d fits median %.3f ms (%.3f..%.3f)"
              % ((n, len(held)) + timed(lambda: ctx.nb_fit(X32, y, folds, held))), flush=True)
        terms = [BernoulliNB()._set_counts(fc[j], cc[j])._jll_terms() for j in range(len(held))]
        delta, prior, neg = (np.stack([t[i] for t in terms]) for i in range(3))
        print("psk_nb_jll n=%d p=1000: %d models median %.3f ms (%.3f..%.3f)"
              % ((n, len(held)) + timed(lambda: ctx.nb_jll(X32, delta, prior, neg))), flush=True)
        jll = ctx.nb_jll(X32, delta, prior, neg)
        print("  training accuracy of the all-sample model %.4f" % np.mean(np.argmax(jll[-1], axis=1) == y), flush=True)
