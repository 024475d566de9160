#!/usr/bin/env python3
"""Records tests/golden/pca_kat.npz from scikit-learn's StandardScaler() and PCA() (the file notes the version; 1.7.2 is the
contract of `--pca`): the known answers of psk_pca_fit / psk_pca_transform and of model_pca.

Designs (seeded; every third column copies one of three latent sample groups with 10 % noise, the others are Bernoulli(0.35);
column 1 duplicates column 0 and column 2 is its complement, so equal |loadings| of opposite sign exist and the rank drops by
two):
  A  24 x 40    n below one 64-sample word and no multiple of 16; p > n: rank n - 1, the last lambda ~ 0
  B  96 x 300   the common case, p > n
  C  130 x 64   counts 0 .. 4 (--real_counts), n > p, three words; the last column is constant (scale 1)
  D  200 x 15   scikit-learn takes covariance_eigh; p below one MFMA tile.  The duplicate only, no complement: three copies of
                one column among 15 always carry the largest loading of the first component, with both signs, and
                scikit-learn's svd_flip then decides that component's sign by the last bits of LAPACK's result (its argmax
                fell on column 0, 1 or 2 depending on the seed): condition 3 below cannot hold for any seed
  E  65 x 700   n one past a word; p >> n and no multiple of a tile
Per design: StandardScaler().fit, PCA().fit, the transformed scores, the resolved _fit_svd_solver, the mask explained_variance_
> 0.9, and per component of that mask oracle.ttest_row (roles swapped: presence = (y == 1), pheno = the scores of the component)
for the recorded labels and non-uniform weights, and PCs_to_keep (p < 0.01).  Component rows and score columns are stored down
to the rank floor.

The generator asserts, of scikit-learn alone (tests/pca_restated.py derives the bounds):
  1. scikit-learn's values lie within every bound of the restatement;
  2. tol_v[i] <= 1e-6 for every component with explained variance > 0.9 of every design;
  3. scikit-learn's own sign decision on those components is not made inside its rounding noise: the largest |loading| of a row
     exceeds the largest |loading| of the opposite sign by more than 2 tol_v[i].  (Column 2 against columns 0 and 1 is such a
     tie by construction; where it is the largest loading of a row, svd_flip decides by the last bits of LAPACK's result and no
     second implementation can be held to it.  The seeds below are the first for which no kept component is decided so.)
usage: tools/gen_pca_golden.py"""
import os
import sys

import numpy as np
import sklearn
from sklearn.decomposition import PCA
from sklearn.preprocessing import StandardScaler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pca_restated as R  # noqa: E402
from oracle import oracle  # noqa: E402

SEEDS = {"A": 701, "B": 700, "C": 703, "D": 700, "E": 700}
SHAPES = [("A", 24, 40), ("B", 96, 300), ("C", 130, 64), ("D", 200, 15), ("E", 65, 700)]


def design(name, n, p, seed):
    rng = np.random.default_rng(seed)
    group = rng.integers(0, 3, n)
    X = (rng.random((n, p)) < 0.35).astype(np.int64)
    for j in range(0, p, 3):
        X[:, j] = (group == (j // 3) % 3) ^ (rng.random(n) < 0.10)
    top = 1
    if name == "C":                               # counts: a present k-mer is seen 1 .. 4 times
        X = X * rng.integers(1, 5, (n, p))
        top = 4
        X[:, p - 1] = 1                               # constant over the samples
    X[:, 1] = X[:, 0]
    if name != "D":
        X[:, 2] = top - X[:, 0]
    y = ((group == 0) ^ (rng.random(n) < 0.15)).astype(np.int64)
    w = rng.uniform(0.5, 2.0, n)
    return X, y, w


out = {"sklearn_version": np.array(sklearn.__version__), "names": np.array([s[0] for s in SHAPES])}
for d, (name, n, p) in enumerate(SHAPES):
    X, y, w = design(name, n, p, SEEDS[name])
    Xf = X.astype(np.float64)
    scaler = StandardScaler().fit(Xf)
    Zs = scaler.transform(Xf)
    pca = PCA().fit(Zs)
    scores = pca.transform(Zs)
    lam_sk = pca.singular_values_ ** 2
    keep_ev = pca.explained_variance_ > 0.9
    assert keep_ev.any() and np.array_equal(keep_ev, np.arange(len(keep_ev)) < keep_ev.sum())      # a prefix

    r = R.fit(Xf)
    Z, lam = r["Z"], r["lambda"]
    tol_lam = R.lambda_tolerance(Z, lam[0])
    tol_v = R.vector_tolerance(lam, tol_lam)
    # 1. scikit-learn inside the restatement's bounds
    assert np.array_equal(scaler.mean_, r["mean"]), name
    assert np.all(np.abs(scaler.var_ - r["var"]) <= R.var_tolerance(n, r["mean"], r["var"])), name
    assert np.array_equal(scaler.scale_ == 1.0, r["var"] == 0.0) and (name != "C" or scaler.var_[-1] == 0.0), name
    assert np.all(np.abs(lam_sk - lam) <= tol_lam), (name, np.abs(lam_sk - lam).max() / tol_lam)
    assert np.array_equal(keep_ev, R.kept_prefix(lam, n)), name
    k = int(keep_ev.sum())
    # 3. before the comparison of the vectors: the signs are scikit-learn's to decide, not its rounding's
    for c in range(k):
        v = pca.components_[c]
        top = np.argmax(np.abs(v))
        other = np.abs(v[np.sign(v) != np.sign(v[top])])
        assert abs(v[top]) - (other.max() if len(other) else 0.0) > 2 * tol_v[c], (name, c, "sign decided by rounding")
    dv = np.linalg.norm(pca.components_[:k] - r["components"][:k], axis=1)
    assert np.all(dv <= tol_v[:k]), (name, (dv / tol_v[:k]).max())
    ds = np.linalg.norm(scores[:, :k] - r["scores"][:, :k], axis=0)
    tol_s = np.sqrt(lam[0]) * tol_v[:k] + np.sqrt(n) * R.fit_score_tolerance(Z, r["components"][:k], lam, tol_lam).max(axis=0)
    assert np.all(ds <= tol_s), (name, (ds / tol_s).max())
    # 2. the comparison of the kept components is not vacuous
    assert np.all(tol_v[:k] <= 1e-6), (name, tol_v[:k].max())

    stored = int(np.count_nonzero(lam_sk > R.rank_floor(n, p, lam_sk[0])))
    tt = np.array([oracle.ttest_row(y == 1, scores[:, c], w, 0, n) for c in range(k)], dtype=np.float64)
    keep = np.zeros(min(n, p), dtype=bool)
    keep[:k] = tt[:, 1] < 0.01
    assert keep.any(), name
    print("design %s (%d x %d, %s): K = %.2f, lambda within %.3f of its bound, kept components within %.3g of tol_v (largest tol_v %.2g, "
          "smallest gap %.2g lambda_1), %d of %d components > 0.9, %d kept by the t-test, %d stored"
          % (name, n, p, pca._fit_svd_solver, R.rho(Z, lam[0]) + R.K_FIXED, np.abs(lam_sk - lam).max() / tol_lam, (dv / tol_v[:k]).max(),
             tol_v[:k].max(), R.gaps(lam)[:k].min() / lam[0], k, min(n, p), keep.sum(), stored))
    for key, val in (("X", X.astype(np.uint8)), ("y", y.astype(np.int8)), ("w", w), ("solver", np.array(pca._fit_svd_solver)),
                     ("mean", scaler.mean_), ("var", scaler.var_), ("scale", scaler.scale_), ("ev", pca.explained_variance_),
                     ("evr", pca.explained_variance_ratio_), ("sv", pca.singular_values_), ("components", pca.components_[:stored]),
                     ("scores", scores[:, :stored]), ("keep_ev", keep_ev), ("ttest", tt), ("keep", keep)):
        out["%s_%s" % (name, key)] = val
path = os.path.join(ROOT, "tests", "golden", "pca_kat.npz")
np.savez_compressed(path, **out)
size = os.path.getsize(path)
assert size < 1 << 20, size
print("wrote %s: %d bytes, scikit-learn %s" % (path, size, sklearn.__version__))
