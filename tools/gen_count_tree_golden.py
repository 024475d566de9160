#!/usr/bin/env python
"""Writes tests/golden/count_tree_kat.npz: scikit-learn's own DecisionTreeClassifier and RandomForestClassifier fits on
designs of k-mer COUNTS, the known answers of tests/test_count_tree_host.py and tests/test_gpu_count_tree.py.  Needs
scikit-learn 1.7.2 (build machine only); the tests read the file, which records the version.

Designs (default_rng(7)) at (64, 12), (130, 40), (256, 40), (257, 70): column j is Poisson(lambda_j), lambda_j ~ U(0.2, 2.5);
15 % of the columns are replaced by Poisson(30) x Bernoulli(0.7) (an amplified gene that some samples lack); the last but
one column is uniform on 0 .. 999 (more than 64 distinct values where n allows), the last one constant.  Labels: a noisy vote
of count thresholds on three columns, so that good splits lie at thresholds other than 0.5.
DT cases (every design x criterion x max_depth 1..10, all samples): the tree_ arrays with thresholds of
DecisionTreeClassifier(random_state=0) and whether SEEDS values of random_state all gave that tree (the SEED-INVARIANT
cases, as in gen_tree_golden.py).  Asserted: at least 12 seed-invariant cases covering depths 1-3 under both criteria, each
with a split whose threshold is not 0.5.
RF cases: RF_PARAMS x seeds {0, 41} x 10 trees on the (130, 40) and (257, 70) designs, every tree with its thresholds, and
predict_proba.  The search: RandomizedSearchCV(RandomForestClassifier(random_state=7), RS_GRID, n_iter=4, cv=3,
random_state=7) on (130, 40)."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(64, 12), (130, 40), (256, 40), (257, 70)]
DEPTHS = range(1, 11)
SEEDS = 12
CRITERIA = ("gini", "entropy")
RF_DESIGNS, RF_SEEDS = (1, 3), (0, 41)
RF_PARAMS = [dict(bootstrap=True, criterion="gini", max_depth=None, max_features="sqrt", min_samples_leaf=1, min_samples_split=2),
             dict(bootstrap=False, criterion="entropy", max_depth=None, max_features=None, min_samples_leaf=2, min_samples_split=2),
             dict(bootstrap=True, criterion="entropy", max_depth=None, max_features="log2", min_samples_leaf=4, min_samples_split=2),
             dict(bootstrap=False, criterion="gini", max_depth=None, max_features="sqrt", min_samples_leaf=1, min_samples_split=2)]
RS_DESIGN, RS_SEED, RS_CV, RS_N_ITER = 1, 7, 3, 4
RS_GRID = {"bootstrap": [True, False], "criterion": ["gini", "entropy"], "max_depth": [4, 20, None],
           "max_features": [None, "sqrt", "log2"], "min_samples_leaf": [1, 2, 4], "min_samples_split": [2, 5, 10],
           "n_estimators": [5, 10]}


def designs():
    rng = np.random.default_rng(7)
    out = []
    for n, p in SHAPES:
        X = rng.poisson(rng.uniform(0.2, 2.5, p), (n, p)).astype(np.float64)
        heavy = np.nonzero(rng.random(p) < 0.15)[0]
        if len(heavy) == 0:
            heavy = np.array([2])
        X[:, heavy] = rng.poisson(30, (n, len(heavy))) * (rng.random((n, len(heavy))) < 0.7)
        X[:, p - 2] = rng.integers(0, 1000, n)
        X[:, p - 1] = 3.0
        h = int(heavy[0])
        vote = (X[:, 0] >= 2).astype(float) + (X[:, 1] >= 3) + (X[:, h] > 28) + rng.normal(0.0, 0.3, n)
        out.append((X, (vote > 1.2).astype(np.int64)))
    return out


def tree_arrays(t):
    return dict(feature=t.feature, threshold=t.threshold, left=t.children_left, right=t.children_right, n=t.n_node_samples,
                counts=np.rint(t.value[:, 0, :] * t.weighted_n_node_samples[:, None]), impurity=t.impurity)


def same_tree(a, b):
    return (a.node_count == b.node_count and np.array_equal(a.feature, b.feature) and np.array_equal(a.threshold, b.threshold)
            and np.array_equal(a.children_left, b.children_left) and np.array_equal(a.n_node_samples, b.n_node_samples))


class Trees:
    """The node arrays of many trees, concatenated under `prefix`."""

    def __init__(self, prefix):
        self.prefix, self.node, self.ptr, self.depth = prefix, {}, [0], []

    def add(self, t):
        for k, v in tree_arrays(t).items():
            self.node.setdefault(k, []).append(v)
        self.ptr.append(self.ptr[-1] + t.node_count)
        self.depth.append(t.max_depth)

    def into(self, out):
        pre = self.prefix
        kinds = dict(feature=np.int16, left=np.int16, right=np.int16, n=np.int16, counts=np.int16, threshold=np.float64, impurity=np.float64)
        for k, v in self.node.items():
            out[pre + "node_" + k] = np.concatenate(v).astype(kinds[k])
        out[pre + "node_ptr"], out[pre + "tree_max_depth"] = np.array(self.ptr), np.array(self.depth)


def main():
    import sklearn
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import RandomizedSearchCV, StratifiedKFold
    from sklearn.tree import DecisionTreeClassifier
    import forest_restated as R
    from phenotypeseeker_amd import cv as CV
    if sklearn.__version__ != "1.7.2":
        raise SystemExit("the fixture records scikit-learn 1.7.2, found %s" % sklearn.__version__)

    ds = designs()
    out = {"n_designs": len(ds), "sklearn_version": np.array(sklearn.__version__), "seeds": SEEDS}
    for d, (X, y) in enumerate(ds):
        assert X.max() < 65536 and np.all(X[:, -1] == 3.0)
        assert len(np.unique(X[:, -2])) > 64 or X.shape[0] <= 64
        out["X%d" % d] = X.astype(np.uint8 if X.max() < 256 else np.uint16)
        out["y%d" % d] = y.astype(np.int8)
        print("design %d: %s, %d of class 1, up to %d distinct values in a column" % (d, X.shape, int(y.sum()),
                                                                                     max(len(np.unique(X[:, j])) for j in range(X.shape[1]))))

    dt = Trees("dt_")
    case = {k: [] for k in ("design", "criterion", "depth", "invariant")}
    good = set()
    for d, (X, y) in enumerate(ds):
        for ci, crit in enumerate(CRITERIA):
            for depth in DEPTHS:
                fits = [DecisionTreeClassifier(max_depth=depth, criterion=crit, random_state=s).fit(X, y).tree_ for s in range(SEEDS)]
                t = fits[0]
                inv = all(same_tree(t, f) for f in fits[1:])
                for k, v in zip(case, (d, ci, depth, inv)):
                    case[k].append(v)
                dt.add(t)
                if inv and depth <= 3 and np.any((t.feature >= 0) & (t.threshold != 0.5)):
                    good.add((d, ci, depth))
    inv = np.array(case["invariant"])
    print("DT: %d of %d cases seed-invariant; %d at depths 1-3 with a threshold other than 0.5" % (int(inv.sum()), len(inv), len(good)))
    print("  by (criterion, depth): %s" % sorted((c, k, d) for d, c, k in good))
    if len(good) < 12 or {(c, k) for _, c, k in good} != {(c, k) for c in (0, 1) for k in (1, 2, 3)}:
        raise SystemExit("fewer than 12 seed-invariant cases with a count threshold at depths 1-3 under both criteria: choose other designs")
    for k, v in case.items():
        out["dt_" + k] = np.array(v)
    dt.into(out)

    rf = Trees("rf_")
    rcase = {k: [] for k in ("design", "seed", "params")}
    proba, tree_ptr, sample_ptr = [], [0], [0]
    for d in RF_DESIGNS:
        X, y = ds[d]
        for q in RF_PARAMS:
            for seed in RF_SEEDS:
                m = RandomForestClassifier(n_estimators=10, random_state=seed, **q).fit(X, y)
                rcase["design"].append(d)
                rcase["seed"].append(seed)
                rcase["params"].append(R.encode_params(dict(q, n_estimators=10)))
                for e in m.estimators_:
                    rf.add(e.tree_)
                tree_ptr.append(tree_ptr[-1] + len(m.estimators_))
                proba.append(m.predict_proba(X).ravel())
                sample_ptr.append(sample_ptr[-1] + 2 * X.shape[0])
    for k, v in rcase.items():
        out["rf_" + k] = np.array(v)
    rf.into(out)
    out["rf_tree_ptr"], out["rf_sample_ptr"], out["rf_proba"] = np.array(tree_ptr), np.array(sample_ptr), np.concatenate(proba)
    thr = out["rf_node_threshold"][out["rf_node_feature"] >= 0]
    print("RF: %d forests, %d trees, %d nodes; %d of %d split thresholds are not 0.5" % (len(rcase["seed"]), tree_ptr[-1], rf.ptr[-1],
                                                                                       int((thr != 0.5).sum()), len(thr)))

    X, y = ds[RS_DESIGN]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g = RandomizedSearchCV(RandomForestClassifier(random_state=RS_SEED), RS_GRID, n_iter=RS_N_ITER, cv=RS_CV, random_state=RS_SEED).fit(X, y)
    r = g.cv_results_
    sk_folds = np.full(len(y), -1)
    for f, (_, te) in enumerate(StratifiedKFold(RS_CV).split(X, y)):
        sk_folds[te] = f
    if not np.array_equal(sk_folds, CV.stratified_kfold(y, RS_CV)):
        raise SystemExit("cv.stratified_kfold differs from StratifiedKFold on the search design")
    out["rs_design"], out["rs_cv"], out["rs_seed"], out["rs_n_iter"] = RS_DESIGN, RS_CV, RS_SEED, RS_N_ITER
    for key, vals in RS_GRID.items():
        out["rs_grid_" + key] = np.array([R.encode_params(dict(R.grid_point(RS_GRID, 0), **{key: v}))[sorted(RS_GRID).index(key)] for v in vals])
    out["rs_params"] = np.array([R.encode_params(q) for q in r["params"]])
    out["rs_splits"] = np.array([r["split%d_test_score" % f] for f in range(RS_CV)]).T
    out["rs_mean"], out["rs_rank"] = r["mean_test_score"], r["rank_test_score"]
    out["rs_best"] = np.array(R.encode_params(g.best_params_))
    out["rs_proba"] = g.best_estimator_.predict_proba(X)
    print("search: means %s, ranks %s, best %s" % (np.round(r["mean_test_score"], 4), r["rank_test_score"], g.best_params_))

    path = os.path.join(ROOT, "tests", "golden", "count_tree_kat.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    if size >= 1 << 20:
        os.remove(path)
        raise SystemExit("the fixture must stay under 1 MiB: trim the family")


if __name__ == "__main__":
    main()
