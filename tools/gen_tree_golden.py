#!/usr/bin/env python
"""Writes tests/golden/tree_kat.npz: scikit-learn's own DecisionTreeClassifier fits on 0/1 designs, the known answers of
tests/test_tree_host.py and tests/test_gpu_tree.py.  Needs scikit-learn 1.7.2 (build machine only); the tests read the file.

Designs: rng.random((n, p)) < rng.uniform(.1, .9, p) from default_rng(7) at (256, 40), (256, 200), (1024, 200), labels a
noisy threshold of six columns; then the first design with every column duplicated, and with complemented duplicates.
Per case (design x criterion x max_depth 1..10, all samples): the tree_ arrays, predict_proba and feature_importances_ of
DecisionTreeClassifier(random_state=0), and whether the fits under SEEDS values of random_state all gave that same tree:
the SEED-INVARIANT cases, the ones where scikit-learn's unseeded tie rule does not matter and the recorded tree is THE
answer.  The generator asserts that the duplicate-free designs give at least 18 such cases covering depths 1-3 under both
criteria.  The grid-search record is GridSearchCV(DecisionTreeClassifier(random_state=0), {'max_depth': 1..3, 'criterion':
['gini', 'entropy']}, cv=5) on a design where every fold fit is seed-invariant (checked here as well)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(256, 40), (256, 200), (1024, 200)]
DEPTHS = range(1, 11)
SEEDS = 12
GS_DEPTHS, GS_CV, FOLDS = [1, 2, 3], 5, 5
CRITERIA = ("gini", "entropy")


def designs():
    rng = np.random.default_rng(7)
    out = []
    for n, p in SHAPES:
        X = (rng.random((n, p)) < rng.uniform(.1, .9, p)).astype(np.float64)
        y = (X[:, :6].sum(axis=1) + rng.normal(0.0, 1.0, n) > 3).astype(np.int64)   # three of the first six columns, noisy
        out.append((X, y, "plain"))
    X, y, _ = out[0]
    out.append((np.repeat(X, 2, axis=1), y, "duplicated"))
    out.append((np.hstack([X, 1.0 - X]), y, "complemented"))
    return out


def same_tree(a, b):
    return (a.node_count == b.node_count and np.array_equal(a.feature, b.feature) and np.array_equal(a.children_left, b.children_left)
            and np.array_equal(a.children_right, b.children_right) and np.array_equal(a.n_node_samples, b.n_node_samples))


def main():
    import sklearn
    from sklearn.model_selection import GridSearchCV, StratifiedKFold
    from sklearn.tree import DecisionTreeClassifier
    from phenotypeseeker_amd import cv as CV
    if sklearn.__version__ != "1.7.2":
        raise SystemExit("the fixture records scikit-learn 1.7.2, found %s" % sklearn.__version__)

    ds = designs()
    out = {"n_designs": len(ds), "kind": np.array([k for _, _, k in ds]), "seeds": SEEDS}
    case = {k: [] for k in ("design", "criterion", "depth", "invariant", "max_depth")}
    node = {k: [] for k in ("feature", "left", "right", "n", "impurity", "value")}
    proba, imps, node_ptr, sample_ptr, feat_ptr = [], [], [0], [0], [0]
    for d, (X, y, kind) in enumerate(ds):
        n, p = X.shape
        out["X%d" % d] = np.packbits(X.astype(np.uint8), axis=1)
        out["y%d" % d], out["shape%d" % d] = y.astype(np.int8), np.array([n, p])
        out["folds%d" % d] = CV.stratified_kfold(y, FOLDS).astype(np.int8)
        for ci, crit in enumerate(CRITERIA):
            for depth in DEPTHS:
                fits = [DecisionTreeClassifier(max_depth=depth, criterion=crit, random_state=s).fit(X, y) for s in range(SEEDS)]
                m, t = fits[0], fits[0].tree_
                inv = all(same_tree(t, f.tree_) for f in fits[1:])
                for k, v in zip(case, (d, ci, depth, inv, t.max_depth)):
                    case[k].append(v)
                node["feature"].append(t.feature)
                node["left"].append(t.children_left)
                node["right"].append(t.children_right)
                node["n"].append(t.n_node_samples)
                node["impurity"].append(t.impurity)
                node["value"].append(t.value[:, 0, :])
                node_ptr.append(node_ptr[-1] + t.node_count)
                proba.append(m.predict_proba(X).ravel())
                sample_ptr.append(sample_ptr[-1] + 2 * n)
                imps.append(m.feature_importances_)
                feat_ptr.append(feat_ptr[-1] + p)
    inv = np.array(case["invariant"])
    des, dep, cri = np.array(case["design"]), np.array(case["depth"]), np.array(case["criterion"])
    plain = np.array([k == "plain" for _, _, k in ds])[des]
    for kind in ("plain", "duplicated", "complemented"):
        sel = np.array([k == kind for _, _, k in ds])[des]
        print("%-12s designs: %d of %d cases seed-invariant; by depth %s" % (
            kind, int(inv[sel].sum()), int(sel.sum()), {int(k): int(inv[sel & (dep == k)].sum()) for k in DEPTHS}))
    shallow = plain & (dep <= 3)
    if int(inv[shallow].sum()) < 18 or {(int(c), int(k)) for c, k in zip(cri[shallow & inv], dep[shallow & inv])} != {
            (c, k) for c in (0, 1) for k in (1, 2, 3)}:
        raise SystemExit("fewer than 18 seed-invariant cases at depths 1-3 on the duplicate-free designs: choose other designs")

    # the grid search: every fold fit must be seed-invariant, or the recorded scores are one draw of several; the first
    # duplicate-free design (largest first) on which that holds carries the record
    def folds_invariant(X, y, folds):
        for crit in CRITERIA:
            for depth in GS_DEPTHS:
                for f in list(range(GS_CV)) + [-1]:
                    tr = folds != f
                    fits = [DecisionTreeClassifier(max_depth=depth, criterion=crit, random_state=s).fit(X[tr], y[tr]).tree_
                            for s in range(SEEDS)]
                    if not all(same_tree(fits[0], t) for t in fits[1:]):
                        print("grid design %d: the fit at %s, depth %d, fold %d depends on random_state" % (gd, crit, depth, f))
                        return False
        return True
    for gd in sorted((d for d, (_, _, k) in enumerate(ds) if k == "plain"), key=lambda d: -ds[d][0].shape[0]):
        X, y, _ = ds[gd]
        folds = CV.stratified_kfold(y, GS_CV)
        if folds_invariant(X, y, folds):
            break
    else:
        raise SystemExit("no duplicate-free design has seed-invariant fold fits at depths %s" % GS_DEPTHS)
    g = GridSearchCV(DecisionTreeClassifier(random_state=0), {"max_depth": GS_DEPTHS, "criterion": list(CRITERIA)}, cv=GS_CV).fit(X, y)
    r = g.cv_results_
    sk_folds = np.full(len(y), -1)
    for f, (_, te) in enumerate(StratifiedKFold(GS_CV).split(X, y)):
        sk_folds[te] = f
    if not np.array_equal(sk_folds, folds):
        raise SystemExit("cv.stratified_kfold differs from StratifiedKFold on the grid design")
    out["gs_design"], out["gs_cv"], out["gs_depths"] = gd, GS_CV, np.array(GS_DEPTHS)
    out["gs_params"] = np.array([[CRITERIA.index(q["criterion"]), q["max_depth"]] for q in r["params"]])
    out["gs_splits"] = np.array([r["split%d_test_score" % f] for f in range(GS_CV)]).T
    out["gs_mean"], out["gs_std"], out["gs_rank"] = r["mean_test_score"], r["std_test_score"], r["rank_test_score"]
    out["gs_best"] = np.array([CRITERIA.index(g.best_params_["criterion"]), g.best_params_["max_depth"]])
    print("grid search on design %d: means %s, ranks %s, best %s" % (gd, np.round(r["mean_test_score"], 4), r["rank_test_score"],
                                                                     g.best_params_))

    for k, v in case.items():
        out["case_" + k] = np.array(v)
    out["node_feature"] = np.concatenate(node["feature"]).astype(np.int16)
    out["node_left"], out["node_right"] = np.concatenate(node["left"]).astype(np.int16), np.concatenate(node["right"]).astype(np.int16)
    out["node_n"], out["node_impurity"] = np.concatenate(node["n"]).astype(np.int16), np.concatenate(node["impurity"])
    out["node_value"] = np.concatenate(node["value"])
    out["proba"], out["importances"] = np.concatenate(proba), np.concatenate(imps)
    out["node_ptr"], out["sample_ptr"], out["feat_ptr"] = np.array(node_ptr), np.array(sample_ptr), np.array(feat_ptr)
    path = os.path.join(ROOT, "tests", "golden", "tree_kat.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d cases, %d nodes, %d bytes" % (path, len(inv), node_ptr[-1], size))
    if size >= 1 << 20:
        os.remove(path)
        raise SystemExit("the fixture must stay under 1 MiB: trim the family")


if __name__ == "__main__":
    main()
