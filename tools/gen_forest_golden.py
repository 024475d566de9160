#!/usr/bin/env python
"""Writes tests/golden/forest_kat.npz: scikit-learn's own RandomForestClassifier fits under fixed seeds on 0/1 designs, the
known answers of tests/test_forest_host.py and tests/test_gpu_forest.py.  Needs scikit-learn 1.7.2 (build machine only); the
tests read the file, which records the version.

Designs (default_rng(17)): n in {40, 63, 64, 65, 130} (the 64-sample word boundary from both sides), p in {1, 5, 24, 70}.  The
"mixed" ones carry a duplicated, a complemented, an all-zero and an all-one column, so known constants, constants found in a
node and visit-order ties between equal columns all occur; the "staircase" (X[i][j] = i > j, n = 40, alternating labels)
drives a tree at least 20 levels deep; "search" (60 x 30) carries the recorded RandomizedSearchCV.
Cases: CASES seeded forests of 3-10 trees, their parameters cycling with different periods through every value of criterion,
bootstrap, max_features, min_samples_leaf, min_samples_split and max_depth in {4, 20, None}; per case every tree's arrays,
predict_proba and feature_importances_.  The search: RandomizedSearchCV(RandomForestClassifier(random_state=S), grid,
n_iter=6, cv=3, random_state=S) over a 648-point grid with n_estimators in {5, 10} (6 / 648 < 0.01: the sampler regime of
the reference's default 25 / 10,692).  Draws: the first 25 grid indices of the reference's grid for seeds 0-4."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = 48
RS_SEED, RS_CV, RS_N_ITER = 3, 3, 6
RS_GRID = {"bootstrap": [True, False], "criterion": ["gini", "entropy"], "max_depth": [4, 20, None],
           "max_features": [None, "sqrt", "log2"], "min_samples_leaf": [1, 2, 4], "min_samples_split": [2, 5, 10],
           "n_estimators": [5, 10]}


def designs():
    rng = np.random.default_rng(17)

    def plain(n, p):
        X = (rng.random((n, p)) < rng.uniform(.15, .85, p)).astype(np.float64)
        y = (X[:, :3].sum(axis=1) + rng.normal(0.0, 0.8, n) > 0.5 * min(p, 3)).astype(np.int64)
        y[:2] = [0, 1]
        return X, y

    def mixed(n, p):
        X, y = plain(n, p)
        X[:, 1], X[:, 2], X[:, 3], X[:, 4] = X[:, 0], 1.0 - X[:, 0], 0.0, 1.0
        if p > 10:
            X[:, 9], X[:, 10] = X[:, 8], X[:, 8]
        return X, y

    out = [plain(40, 1) + ("plain",), mixed(63, 5) + ("mixed",), mixed(64, 24) + ("mixed",), mixed(65, 70) + ("mixed",),
           mixed(130, 24) + ("mixed",), plain(130, 70) + ("plain",)]
    S = np.zeros((40, 70))
    S[:, :40] = np.arange(40)[:, None] > np.arange(40)[None, :]
    out.append((S, np.arange(40) % 2, "staircase"))
    out.append(plain(60, 30) + ("search",))
    return out


def case_params(k):
    q = dict(criterion=("gini", "entropy")[k % 2], bootstrap=bool((k // 2) % 2 == 0), max_features=(None, "sqrt", "log2")[k % 3],
             min_samples_leaf=(1, 2, 4)[(k // 3) % 3], min_samples_split=(2, 5, 10)[(k // 5) % 3], max_depth=(None, 4, 20)[(k // 7) % 3],
             n_estimators=3 + k % 8)
    if k in (6, 13):      # the staircase at full depth (k % 7 == 6): no bootstrap, every column, and once capped at 20 levels
        q.update(bootstrap=False, max_features=None, min_samples_leaf=1, min_samples_split=2, max_depth=None if k == 6 else 20)
    return q


def main():
    import sklearn
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import ParameterSampler, RandomizedSearchCV, StratifiedKFold
    import forest_restated as R
    from phenotypeseeker_amd import cv as CV
    if sklearn.__version__ != "1.7.2":
        raise SystemExit("the fixture records scikit-learn 1.7.2, found %s" % sklearn.__version__)

    ds = designs()
    out = {"n_designs": len(ds), "kind": np.array([k for _, _, k in ds]), "sklearn_version": np.array(sklearn.__version__)}
    for d, (X, y, _) in enumerate(ds):
        out["X%d" % d] = np.packbits(X.astype(np.uint8), axis=1)
        out["y%d" % d], out["shape%d" % d] = y.astype(np.int8), np.array(X.shape)
    case = {k: [] for k in ("design", "seed", "params")}
    node = {k: [] for k in ("feature", "left", "right", "n", "counts", "impurity")}
    tree_depth, proba, imps = [], [], []
    node_ptr, tree_ptr, sample_ptr, feat_ptr = [0], [0], [0], [0]
    n_cases_designs = len(ds) - 1            # the search design has no forest case
    for k in range(CASES):
        d = k % n_cases_designs
        X, y, _ = ds[d]
        q = case_params(k)
        m = RandomForestClassifier(random_state=100 + k, **q).fit(X, y)
        case["design"].append(d)
        case["seed"].append(100 + k)
        case["params"].append(R.encode_params(q))
        for e in m.estimators_:
            t = e.tree_
            node["feature"].append(t.feature)
            node["left"].append(t.children_left)
            node["right"].append(t.children_right)
            node["n"].append(t.n_node_samples)
            node["counts"].append(np.rint(t.value[:, 0, :] * t.weighted_n_node_samples[:, None]))
            node["impurity"].append(t.impurity)
            tree_depth.append(t.max_depth)
            node_ptr.append(node_ptr[-1] + t.node_count)
        tree_ptr.append(tree_ptr[-1] + len(m.estimators_))
        proba.append(m.predict_proba(X).ravel())
        sample_ptr.append(sample_ptr[-1] + 2 * X.shape[0])
        imps.append(m.feature_importances_)
        feat_ptr.append(feat_ptr[-1] + X.shape[1])
    P = np.array(case["params"])
    for col, vals in ((0, {0, 1}), (1, {0, 1}), (2, {0, 4, 20}), (3, {0, 1, 2}), (4, {1, 2, 4}), (5, {2, 5, 10})):
        assert set(P[:, col].tolist()) == vals, (col, set(P[:, col].tolist()))
    deep = max(dp for dp, k in zip(tree_depth, np.repeat(np.arange(CASES), np.diff(tree_ptr))) if ds[k % n_cases_designs][2] == "staircase")
    if deep < 20:
        raise SystemExit("the staircase design reached only depth %d" % deep)

    gd = len(ds) - 1
    X, y, _ = ds[gd]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g = RandomizedSearchCV(RandomForestClassifier(random_state=RS_SEED), RS_GRID, n_iter=RS_N_ITER, cv=RS_CV, random_state=RS_SEED).fit(X, y)
    r = g.cv_results_
    folds = CV.stratified_kfold(y, RS_CV)
    sk_folds = np.full(len(y), -1)
    for f, (_, te) in enumerate(StratifiedKFold(RS_CV).split(X, y)):
        sk_folds[te] = f
    if not np.array_equal(sk_folds, folds):
        raise SystemExit("cv.stratified_kfold differs from StratifiedKFold on the search design")
    out["rs_design"], out["rs_cv"], out["rs_seed"], out["rs_n_iter"] = gd, RS_CV, RS_SEED, RS_N_ITER
    for key, vals in RS_GRID.items():
        out["rs_grid_" + key] = np.array([R.encode_params(dict(R.grid_point(RS_GRID, 0), **{key: v}))[sorted(RS_GRID).index(key)] for v in vals])
    out["rs_params"] = np.array([R.encode_params(q) for q in r["params"]])
    out["rs_splits"] = np.array([r["split%d_test_score" % f] for f in range(RS_CV)]).T
    out["rs_mean"], out["rs_std"], out["rs_rank"] = r["mean_test_score"], r["std_test_score"], r["rank_test_score"]
    out["rs_best"] = np.array(R.encode_params(g.best_params_))
    out["rs_proba"], out["rs_importances"] = g.best_estimator_.predict_proba(X), g.best_estimator_.feature_importances_
    print("search: means %s, ranks %s, best %s" % (np.round(r["mean_test_score"], 4), r["rank_test_score"], g.best_params_))

    out["draw_seeds"] = np.arange(5)
    keys = sorted(R.REFERENCE_GRID)
    idx = []
    for s in range(5):
        row = []
        for q in ParameterSampler(R.REFERENCE_GRID, 25, random_state=s):
            i = 0
            for k in keys:
                i = i * len(R.REFERENCE_GRID[k]) + R.REFERENCE_GRID[k].index(q[k])
            row.append(i)
        idx.append(row)
    out["draw_indices"] = np.array(idx)

    out["case_design"], out["case_seed"], out["case_params"] = np.array(case["design"]), np.array(case["seed"]), P
    out["node_feature"] = np.concatenate(node["feature"]).astype(np.int16)
    out["node_left"], out["node_right"] = np.concatenate(node["left"]).astype(np.int16), np.concatenate(node["right"]).astype(np.int16)
    out["node_n"], out["node_counts"] = np.concatenate(node["n"]).astype(np.int16), np.concatenate(node["counts"]).astype(np.int32)
    out["node_impurity"] = np.concatenate(node["impurity"])
    out["tree_max_depth"] = np.array(tree_depth)
    out["proba"], out["importances"] = np.concatenate(proba), np.concatenate(imps)
    out["node_ptr"], out["tree_ptr"], out["sample_ptr"], out["feat_ptr"] = (np.array(v) for v in (node_ptr, tree_ptr, sample_ptr, feat_ptr))
    path = os.path.join(ROOT, "tests", "golden", "forest_kat.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d cases, %d trees (deepest on the staircase %d), %d nodes, %d bytes" % (path, CASES, tree_ptr[-1], deep, node_ptr[-1], size))
    if size >= 1 << 20:
        os.remove(path)
        raise SystemExit("the fixture must stay under 1 MiB: trim the family")


if __name__ == "__main__":
    main()
