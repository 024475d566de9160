#!/usr/bin/env python
"""Writes tests/golden/svm_kat.npz: scikit-learn's own SVC fits on a family of gene-block 0/1 designs, the known answers
of tests/test_svm_host.py and tests/test_gpu_svm.py.  Needs scikit-learn (build machine only); the tests read the file.

Per fit (design x kernel x C x {all samples | one held-out fold of cv.stratified_kfold(y, 5)}) two records, in libsvm's
sign (class 0 positive: dual = -dual_coef_, rho = intercept_, dec = -decision_function):
  off  SVC(shrinking=False): the path psk_svc_fit walks -- n_iter_, duals at the support vectors, rho, dec on all n samples
  on   SVC(shrinking=True): the reference's actual call; stored in full only where it differs from `off`
Per grid-search design the cv_results_ of GridSearchCV(SVC(kernel='linear', max_iter=1000, tol=1e-4, shrinking=s),
{'C': Cs}, cv=10) for both s.  Measured bounds the GPU tests use (never chosen): the largest |dec_on - dec_off| among
fits both records converged on, and the largest excess of the recomputed stopping quantity Gmax + Gmax2 - tol and of
|y'a| / C on scikit-learn's own converged solutions.
A fit on which the NumPy restatement (tests/svm_restated.py) does not reproduce the `off` record is marked inadmissible
for the exact-path tier; more than 2 % of them and nothing is written."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TOL, MAX_ITER, PATH_RTOL = 1e-4, 1000, 1e-6
CS = [float(1.0 / a) for a in np.logspace(-3, 3, 13)]
# (n, p, flip noise, seed, kernels, all-sample C indices, fold-masked C indices, grid search)
FAMILY = [
    (48, 200, 0.15, 1, ("linear", "rbf"), range(0, 13), (0, 3, 6, 9, 12), False),     # p > n, separable
    (120, 12, 0.30, 3, ("linear", "rbf"), range(0, 13), (0, 3, 6, 9, 12), False),     # p < n: fits stop at the cap
    (96, 40, 0.25, 7, ("linear", "rbf"), range(0, 13, 2), (2, 6, 10), False),
    (200, 100, 0.30, 5, ("linear",), range(0, 13, 2), (), False),
    (256, 1000, 0.42, 2, ("linear",), range(0, 13), (), True),   # two distinct mean scores, on / off records equal
    (150, 300, 0.40, 4, ("linear",), range(0, 13), (), True),    # seven distinct scores, some fits capped, records differ
]
FOLDS, GS_CV = 5, 10


def design(n, p, seed, noise):
    """Gene-like blocks of repeated columns, a share of them tracking the phenotype with per-pattern flip noise."""
    r = np.random.default_rng(seed)
    y = (np.arange(n) % 2).astype(int)
    r.shuffle(y)
    npat = max(4, p // 8)
    pats = []
    for _ in range(npat):
        base = y if r.random() < 0.6 else r.integers(0, 2, n)
        flip = r.random(n) < noise * (0.5 + r.random())
        pats.append(np.where(flip, 1 - base, base))
    pats = np.array(pats).T
    X = pats[:, r.integers(0, npat, p)].astype(float)
    return X, y


def main():
    from sklearn.model_selection import GridSearchCV
    from sklearn.svm import SVC
    import svm_restated as R
    from phenotypeseeker_amd import cv as CV
    warnings.simplefilter("ignore")

    out = {"Cs": np.array(CS), "tol": TOL, "max_iter": MAX_ITER, "n_designs": len(FAMILY)}
    meta = {k: [] for k in ("design", "kernel", "C", "gamma", "fold", "iters_off", "iters_on", "rho_off", "rho_on", "same",
                            "admissible")}
    dec_off, sv_idx, sv_val, sv_ptr = [], [], [], [0]
    on_fit, dec_on, on_sv_idx, on_sv_val, on_sv_ptr = [], [], [], [], [0]
    dec_ptr, on_dec_ptr = [0], [0]
    conv_dev = gap_excess = eq_excess = 0.0
    for d, (n, p, noise, seed, kernels, all_cs, fold_cs, grid) in enumerate(FAMILY):
        X, y = design(n, p, seed, noise)
        folds = CV.stratified_kfold(y, FOLDS)
        out["X%d" % d] = np.packbits(X.astype(np.uint8), axis=1)
        out["y%d" % d], out["shape%d" % d], out["folds%d" % d] = y.astype(np.int8), np.array([n, p]), folds.astype(np.int8)
        for kern in kernels:
            gamma = 1.0 / p if kern == "rbf" else 0.0
            K = R.kernel_matrix(X, kern, gamma)
            jobs = [(ci, -1) for ci in all_cs] + [(ci, f) for ci in fold_cs for f in range(FOLDS)]
            for ci, f in jobs:
                C = CS[ci]
                tr = folds != f
                rec = {}
                for s in (False, True):
                    m = SVC(kernel=kern, gamma=gamma if kern == "rbf" else "scale", C=C, tol=TOL, max_iter=MAX_ITER,
                            shrinking=s).fit(X[tr], y[tr])
                    dual = np.zeros(n)
                    dual[np.nonzero(tr)[0][m.support_]] = -m.dual_coef_[0]
                    rec[s] = (int(m.n_iter_[0]), dual, float(m.intercept_[0]), -m.decision_function(X))
                it0, du0, rho0, de0 = rec[False]
                it1, du1, rho1, de1 = rec[True]
                same = it0 == it1 and np.array_equal(du0, du1) and rho0 == rho1 and np.array_equal(de0, de1)
                rd, rr, rdec, rit = R.fit(X, y, tr, C, kern, gamma, TOL, MAX_ITER)
                scale = max(1.0, np.abs(de0).max())
                adm = (rit == it0 and np.abs(rdec - de0).max() <= PATH_RTOL * scale
                       and np.abs(rd - du0).max() <= PATH_RTOL * max(1.0, np.abs(du0).max())
                       and abs(rr - rho0) <= PATH_RTOL * max(1.0, abs(rho0)))
                if it0 < MAX_ITER and it1 < MAX_ITER:
                    conv_dev = max(conv_dev, float(np.abs(de1 - de0).max()))
                for it, du in ((it0, du0), (it1, du1)):
                    if it < MAX_ITER:
                        gap, eq = R.optimality(K[np.ix_(tr, tr)], y[tr], du[tr], C)
                        gap_excess = max(gap_excess, gap - TOL)
                        eq_excess = max(eq_excess, eq / C)
                for k, v in zip(meta, (d, 0 if kern == "linear" else 1, C, gamma, f, it0, it1, rho0, rho1, same, adm)):
                    meta[k].append(v)
                dec_off.append(de0)
                dec_ptr.append(dec_ptr[-1] + n)
                nz = np.nonzero(du0)[0]
                sv_idx.append(nz)
                sv_val.append(du0[nz])
                sv_ptr.append(sv_ptr[-1] + len(nz))
                if not same:
                    on_fit.append(len(meta["design"]) - 1)
                    dec_on.append(de1)
                    on_dec_ptr.append(on_dec_ptr[-1] + n)
                    nz = np.nonzero(du1)[0]
                    on_sv_idx.append(nz)
                    on_sv_val.append(du1[nz])
                    on_sv_ptr.append(on_sv_ptr[-1] + len(nz))
        if grid:
            res = {}
            for s in (False, True):
                g = GridSearchCV(SVC(kernel="linear", max_iter=MAX_ITER, tol=TOL, shrinking=s), {"C": CS}, cv=GS_CV).fit(X, y)
                r = g.cv_results_
                res[s] = (np.array([r["split%d_test_score" % f] for f in range(GS_CV)]).T, r["mean_test_score"],
                          r["rank_test_score"], g.best_params_["C"])
            # a held-out decision value of the record within the exact-path tolerance of zero would make a score depend on
            # rounding: such a design does not belong in the fixture
            gf = CV.stratified_kfold(y, GS_CV)
            for C in CS:
                for f in range(GS_CV):
                    m = SVC(kernel="linear", max_iter=MAX_ITER, tol=TOL, C=C, shrinking=False).fit(X[gf != f], y[gf != f])
                    de = m.decision_function(X)
                    if np.abs(de[gf == f]).min() <= PATH_RTOL * max(1.0, np.abs(de).max()):
                        raise SystemExit("design %d: a held-out decision value at C=%g, fold %d is within the path tolerance "
                                         "of zero; choose another design" % (d, C, f))
            tag = "gs%d_" % d
            out[tag + "splits_off"], out[tag + "mean_off"], out[tag + "rank_off"], out[tag + "best_C_off"] = res[False]
            out[tag + "splits_on"], out[tag + "mean_on"], out[tag + "rank_on"], out[tag + "best_C_on"] = res[True]
            out[tag + "equal"] = all(np.array_equal(a, b) for a, b in zip(res[False], res[True]))
            print("grid design %d: records equal %s, distinct mean scores %d" % (d, out[tag + "equal"], len(set(res[False][1].tolist()))))
    n_fits = len(meta["design"])
    bad = n_fits - int(np.sum(meta["admissible"]))
    print("%d fits, %d capped (off), %d differ on/off, %d inadmissible; on/off deviation (converged) %.3g, gap excess %.3g, "
          "|y'a|/C %.3g" % (n_fits, int(np.sum(np.array(meta["iters_off"]) >= MAX_ITER)), len(on_fit), bad, conv_dev, gap_excess,
                             eq_excess))
    if bad > 0.02 * n_fits:
        raise SystemExit("more than 2 % of the fits are inadmissible for the exact-path tier: the restatement is wrong")
    for k, v in meta.items():
        out["fit_" + k] = np.array(v)
    out["dec_off"], out["dec_ptr"] = np.concatenate(dec_off), np.array(dec_ptr)
    out["sv_idx"], out["sv_val"], out["sv_ptr"] = np.concatenate(sv_idx).astype(np.int16), np.concatenate(sv_val), np.array(sv_ptr)
    out["on_fit"] = np.array(on_fit, dtype=np.int64)
    out["dec_on"] = np.concatenate(dec_on) if dec_on else np.zeros(0)
    out["on_dec_ptr"] = np.array(on_dec_ptr)
    out["on_sv_idx"] = np.concatenate(on_sv_idx).astype(np.int16) if on_sv_idx else np.zeros(0, np.int16)
    out["on_sv_val"] = np.concatenate(on_sv_val) if on_sv_val else np.zeros(0)
    out["on_sv_ptr"] = np.array(on_sv_ptr)
    out["conv_on_off_dev"], out["cert_gap_excess"], out["cert_eq_excess"] = conv_dev, gap_excess, eq_excess
    path = os.path.join(ROOT, "tests", "golden", "svm_kat.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    if size >= 1 << 20:
        os.remove(path)
        raise SystemExit("the fixture must stay under 1 MiB: trim the family")


if __name__ == "__main__":
    main()
