#!/usr/bin/env python3
"""Records tests/golden/nb_kat.npz from scikit-learn's BernoulliNB() (the file notes the version; 1.7.2 is the contract of
`-bc NB`): the known answers of psk_nb_fit / psk_nb_jll and of model.BernoulliNB.

Designs (n, p): (7, 3), (64, 1), (65, 67), (130, 300), (257, 1031), (4100, 5) -- the smallest that reach the tail of a 64-sample
word, one and several words, fewer columns than lanes, a column stride of 64 that does not divide p, more than one step per
lane, and every lane of the butterfly.  Every design with p >= 5 holds a duplicated (1), a complemented (2), an all-zero (3)
and an all-one (4) column; (257, 1031) is strongly unbalanced.  Each design carries a 3-fold stratified fold vector
(StratifiedKFold(3), unshuffled).  Per design four cases -- all samples, and each fold held out -- with, from scikit-learn:
feature_count_, class_count_, feature_log_prob_, class_log_prior_, and _joint_log_likelihood / predict / predict_proba of ALL
rows.  The designs are stored with np.packbits.

The generator also asserts, of scikit-learn alone, what the tests' label comparison relies on: at most 1 % of a case's
samples have |jll_0 - jll_1| within the rounding band tol_i0 + tol_i1 (tests/nb_restated.py::jll_tolerance).
usage: tools/gen_nb_golden.py"""
import os
import sys

import numpy as np
import sklearn
from sklearn.model_selection import StratifiedKFold
from sklearn.naive_bayes import BernoulliNB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_restated as R  # noqa: E402

SHAPES = [(7, 3), (64, 1), (65, 67), (130, 300), (257, 1031), (4100, 5)]
FOLDS = 3


def design(n, p, seed):
    rng = np.random.default_rng(seed)
    X = (rng.random((n, p)) < rng.uniform(.1, .9, p)).astype(np.uint8)
    kind = "plain"
    if p >= 5:
        X[:, 1], X[:, 2], X[:, 3], X[:, 4] = X[:, 0], 1 - X[:, 0], 0, 1
        kind = "mixed"
    signal = X[:, :min(p, 8)].sum(axis=1) + rng.normal(0.0, 1.0, n)
    if (n, p) == (257, 1031):          # about one sample in twelve is positive
        kind = "unbalanced"
        y = (signal >= np.sort(signal)[-21]).astype(np.int64)
    else:
        y = (signal > np.median(signal)).astype(np.int64)
    if n == 7:
        y = np.array([0, 1, 0, 1, 0, 1, 0])
    fold = np.zeros(n, dtype=np.int32)
    for f, (_, te) in enumerate(StratifiedKFold(FOLDS).split(X, y)):
        fold[te] = f
    return X, y, fold, kind


out = {"sklearn_version": np.array(sklearn.__version__), "n_designs": np.array(len(SHAPES)), "n_folds": np.array(FOLDS)}
kinds = []
for d, (n, p) in enumerate(SHAPES):
    X, y, fold, kind = design(n, p, 100 + d)
    kinds.append(kind)
    out["shape%d" % d], out["X%d" % d], out["y%d" % d], out["fold%d" % d] = np.array([n, p]), np.packbits(X, axis=1), y, fold
    Xf = X.astype(np.float64)
    for k, held in enumerate([-1] + list(range(FOLDS))):
        tr = fold != held
        assert len(set(y[tr])) == 2
        m = BernoulliNB().fit(Xf[tr], y[tr])
        jll = m._joint_log_likelihood(Xf)
        tol = R.jll_tolerance(X != 0, m.feature_log_prob_, m.class_log_prior_)
        inside = np.abs(jll[:, 0] - jll[:, 1]) <= tol.sum(axis=1)
        assert inside.mean() <= 0.01, (n, p, held, inside.sum())
        print("design %d (%d x %d, %s) held-out %2d: %d samples inside the rounding band" % (d, n, p, kind, held, inside.sum()))
        tag = "_%d_%d" % (d, k)
        out["fc" + tag], out["cc" + tag] = m.feature_count_.astype(np.int32), m.class_count_.astype(np.int32)
        assert np.array_equal(out["fc" + tag], m.feature_count_) and np.array_equal(out["cc" + tag], m.class_count_)
        out["flp" + tag], out["clp" + tag] = m.feature_log_prob_, m.class_log_prior_
        out["jll" + tag], out["pred" + tag], out["proba" + tag] = jll, m.predict(Xf).astype(np.int8), m.predict_proba(Xf)
out["kind"] = np.array(kinds)
path = os.path.join(ROOT, "tests", "golden", "nb_kat.npz")
np.savez_compressed(path, **out)
size = os.path.getsize(path)
assert size < 1 << 20, size
print("wrote %s: %d bytes, scikit-learn %s" % (path, size, sklearn.__version__))
