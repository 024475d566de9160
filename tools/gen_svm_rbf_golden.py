#!/usr/bin/env python
"""Writes tests/golden/svm_rbf_search.npz: what scikit-learn 1.7.2 draws and finds for the reference's rbf branch of `-bc SVM`
(RandomizedSearchCV over {'C': 1 / alphas, 'gamma': 1 / gammas}, modeling.py:1050-1056, :1091-1095), the known answers of
tests/test_svm_rbf_host.py and tests/test_gpu_svm_rbf.py.  Needs scikit-learn (build machine only); the tests read the file.

  draw_<size>_<n_iter>_<seed>   sklearn.utils.random.sample_without_replacement(size, n_iter, random_state=seed): (169, 25) is
                                the rbf default (13 x 13 grid), the others sit on both sides of the two thresholds of
                                method="auto" (n_iter / size 0.01 and 0.99) and on them; (10692, 25) is the forest's default
  X, y, shape                   one 0/1 design of 96 x 40 (the recipe and the third design of tools/gen_svm_golden.py)
  search_*                      RandomizedSearchCV(SVC(kernel='rbf', max_iter=1000, tol=1e-4), grid 13 x 13, n_iter=25, cv=5,
                                random_state=0).fit(X, y): the candidates' C and gamma in order, the split scores
                                [candidate][split], best_index_, and the refit's support_, dual_coef_, intercept_, n_iter_"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TOL, MAX_ITER, N_ITER, CV, SEED = 1e-4, 1000, 25, 5, 0
AXIS = [float(1.0 / a) for a in np.logspace(-3, 3, 13)]
DRAWS = [(169, 25, 0), (169, 25, 1), (169, 25, 7), (169, 1, 0), (169, 2, 0), (169, 167, 0), (169, 168, 0), (169, 169, 0),
         (10692, 25, 0), (100, 1, 0)]
DESIGN = (96, 40, 7, 0.25)      # n, p, seed, flip noise


def main():
    from sklearn.model_selection import RandomizedSearchCV
    from sklearn.svm import SVC
    from sklearn.utils.random import sample_without_replacement
    from gen_svm_golden import design
    warnings.simplefilter("ignore")

    out = {"axis": np.array(AXIS), "tol": TOL, "max_iter": MAX_ITER, "n_iter": N_ITER, "cv": CV, "seed": SEED}
    for size, n_iter, seed in DRAWS:
        out["draw_%d_%d_%d" % (size, n_iter, seed)] = np.asarray(sample_without_replacement(size, n_iter, random_state=seed), dtype=np.int64)
    n, p, dseed, noise = DESIGN
    X, y = design(n, p, dseed, noise)
    out["X"], out["y"], out["shape"] = np.packbits(X.astype(np.uint8), axis=1), y.astype(np.int8), np.array([n, p])
    rs = RandomizedSearchCV(SVC(kernel="rbf", max_iter=MAX_ITER, tol=TOL), {"C": AXIS, "gamma": AXIS}, n_iter=N_ITER, cv=CV,
                            random_state=SEED).fit(X, y)
    r, be = rs.cv_results_, rs.best_estimator_
    out["search_C"] = np.array([q["C"] for q in r["params"]])
    out["search_gamma"] = np.array([q["gamma"] for q in r["params"]])
    out["search_keys"] = np.array(list(r["params"][0]))
    out["search_splits"] = np.array([r["split%d_test_score" % f] for f in range(CV)]).T
    out["search_mean"], out["search_rank"], out["search_best_index"] = r["mean_test_score"], r["rank_test_score"], rs.best_index_
    out["search_support"], out["search_dual_coef"] = be.support_.astype(np.int32), be.dual_coef_
    out["search_intercept"], out["search_refit_iters"] = be.intercept_, be.n_iter_.astype(np.int32)
    path = os.path.join(ROOT, "tests", "golden", "svm_rbf_search.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes; %d distinct mean scores, best candidate %d (C=%g, gamma=%g), refit %d iterations, %d support vectors"
          % (path, os.path.getsize(path), len(set(r["mean_test_score"].tolist())), rs.best_index_, rs.best_params_["C"],
             rs.best_params_["gamma"], int(be.n_iter_[0]), len(be.support_)))


if __name__ == "__main__":
    main()
