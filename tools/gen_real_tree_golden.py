#!/usr/bin/env python
"""Writes tests/golden/real_tree_kat.npz: scikit-learn's own DecisionTreeClassifier and RandomForestClassifier fits on
REAL-VALUED float32 designs, the known answers of tests/test_real_tree_host.py and tests/test_gpu_real_tree.py.  Needs
scikit-learn 1.7.2 (build machine only); the tests read the file, which records the version.

Designs (default_rng(11)), all float32:
  0, 1  65 x 5 and 257 x 9 Gaussian columns with a planted signal (one 64-sample word / one 256-thread trip crossed); the last
        column of design 1 holds only 0.75 and the float32 next to it, in noisy agreement with the label
  2     130 x 40 PCA-like: the scores of a 0/1 matrix with repeated rows through StandardScaler + PCA, rounded to float32 (many
        tied values), then a column of zeros and a column holding -0.0 and +0.0
  3     96 x 1,100 Gaussian columns in steps of 2^-10: more columns than a workgroup has threads and than stay in LDS
Probes: four one-column designs whose root split shows that scikit-learn 1.7.2 as built separates ANY two different float32
values (the FEATURE_THRESHOLD of its source is not in effect); recorded with the threshold it chose.
DT cases: every design x criterion x max_depth (1, 3, 10): the tree of random_state=0 and whether SEEDS values of
random_state all gave it (SEED-INVARIANT).  Deep cases: DecisionTreeClassifier(random_state=s) at depth None, 4 seeds per
design (gini for two, entropy for two).  RF cases: 12 parameter sets of the reference's grid, 10 or 20 trees each, with
predict_proba.  Asserted here: at least 10 seed-invariant single trees, 4 of them with three or more splits; a recorded
threshold whose two neighbours are adjacent float32 values; every probe split where the rules say."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gen_count_tree_golden import Trees, same_tree  # noqa: E402

DEPTHS = (1, 3, 10)
SEEDS = 8
DEEP_SEEDS = ((0, "gini"), (1, "gini"), (2, "entropy"), (3, "entropy"))
CRITERIA = ("gini", "entropy")


def _q(bootstrap, criterion, max_depth, max_features, msl, mss, n_estimators):
    return dict(bootstrap=bootstrap, criterion=criterion, max_depth=max_depth, max_features=max_features, min_samples_leaf=msl,
                min_samples_split=mss, n_estimators=n_estimators)


# (design, seed, parameters), every value from the reference's grid
RF_CASES = [(1, 0, _q(True, "gini", None, "sqrt", 1, 2, 10)), (1, 41, _q(False, "entropy", None, None, 4, 2, 10)),
            (1, 0, _q(True, "entropy", 20, "log2", 1, 10, 20)), (1, 41, _q(False, "gini", 6, "sqrt", 2, 5, 10)),
            (1, 0, _q(True, "gini", None, None, 1, 2, 10)),
            (2, 41, _q(True, "entropy", None, "sqrt", 1, 2, 10)), (2, 0, _q(False, "gini", None, "log2", 4, 2, 10)),
            (2, 41, _q(True, "gini", 4, None, 2, 10, 10)), (2, 0, _q(False, "entropy", 100, "sqrt", 1, 5, 20)),
            (3, 0, _q(True, "gini", None, "sqrt", 1, 2, 10)), (3, 41, _q(False, "entropy", 10, "log2", 4, 10, 10)),
            (3, 0, _q(True, "entropy", None, None, 2, 2, 10))]


def designs():
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    rng = np.random.default_rng(11)
    out = []
    for n, p in ((65, 5), (257, 9)):
        X = rng.normal(0.0, 1.0, (n, p)).astype(np.float32)
        y = (2.0 * X[:, 0] + np.where(X[:, 1] > 0.3, 1.5, -1.5) + rng.normal(0.0, 0.4, n) > 0).astype(np.int64)
        if p == 9:
            agree = rng.random(n) < 0.8
            X[:, 8] = np.where((y == 1) == agree, np.nextafter(np.float32(0.75), np.float32(1)), np.float32(0.75))
        out.append((X, y))
    base = (rng.random((45, 60)) < 0.4).astype(np.float64)
    B = base[rng.integers(0, 45, 130)]                              # repeated rows: tied scores
    S = PCA(n_components=38, svd_solver="full").fit_transform(StandardScaler().fit_transform(B)).astype(np.float32)
    X = np.zeros((130, 40), dtype=np.float32)
    X[:, :38] = S
    X[:, 39] = np.where(rng.random(130) < 0.5, np.float32(-0.0), np.float32(0.0))
    y = (S[:, 0] + 0.7 * S[:, 2] + rng.normal(0.0, 0.5, 130) > 0).astype(np.int64)
    out.append((X, y))
    X = (np.rint(rng.normal(0.0, 1.0, (96, 1100)) * 1024.0) / 1024.0).astype(np.float32)
    y = (X[:, 1050] + np.where(X[:, 300] > -0.2, 0.8, -0.8) + rng.normal(0.0, 0.3, 96) > 0).astype(np.int64)
    out.append((X, y))
    return out


def probes():
    """(x, y, the threshold the rules give) of the four measurements; u = 2^-25."""
    f, u = np.float32, 2.0 ** -25
    a, b, c = f(0.25), f(0.25 + 3 * u), f(0.25 + 6 * u)
    nxt = np.nextafter(f(1.0), f(2.0))
    return [(np.array([a, b] * 4, dtype=f), np.array([0, 1] * 4), float(a) / 2.0 + float(b) / 2.0),
            (np.array([f(1.0), nxt] * 4, dtype=f), np.array([0, 1] * 4), float(f(1.0)) / 2.0 + float(nxt) / 2.0),
            (np.array([a, b, c] * 4, dtype=f), np.array([0, 1, 1] * 4), float(a) / 2.0 + float(b) / 2.0),
            (np.array([a, b, c] * 4, dtype=f), np.array([0, 0, 1] * 4), float(b) / 2.0 + float(c) / 2.0)]


def adjacent_thresholds(X, feature, threshold):
    """How many of a tree's split thresholds lie between two ADJACENT float32 values of their column."""
    k = 0
    for j, t in zip(feature, threshold):
        if j >= 0:
            col = X[:, j]
            lo, hi = col[col <= t].max(), col[col > t].min()
            k += bool(np.nextafter(np.float32(lo), np.float32(np.inf)) == np.float32(hi))
    return k


def main():
    import sklearn
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier
    import forest_restated as R
    if sklearn.__version__ != "1.7.2":
        raise SystemExit("the fixture records scikit-learn 1.7.2, found %s" % sklearn.__version__)

    ds = designs()
    out = {"n_designs": len(ds), "sklearn_version": np.array(sklearn.__version__), "seeds": SEEDS}
    for d, (X, y) in enumerate(ds):
        assert X.dtype == np.float32 and np.all(np.isfinite(X))
        out["X%d" % d], out["y%d" % d] = X, y.astype(np.int8)
        print("design %d: %s, %d of class 1, %d to %d distinct values in a column" % (
            d, X.shape, int(y.sum()), min(len(np.unique(X[:, j])) for j in range(X.shape[1])),
            max(len(np.unique(X[:, j])) for j in range(X.shape[1]))))
    X2 = ds[2][0]
    assert np.all(X2[:, 38] == 0) and len(np.unique(np.signbit(X2[:, 39]))) == 2 and np.all(X2[:, 39] == 0)
    assert min(len(np.unique(X2[:, j])) for j in range(38)) < 60           # tied scores

    px, py, pthr, pptr = [], [], [], [0]
    for x, y, want in probes():
        t = DecisionTreeClassifier(random_state=0).fit(x.reshape(-1, 1), y).tree_
        if t.node_count != 3 or t.threshold[0] != want:
            raise SystemExit("a probe was not split where the rules say: %r gave %d nodes, threshold %r, expected %r"
                             % (x[:3], t.node_count, t.threshold[0], want))
        px.append(x)
        py.append(y)
        pthr.append(t.threshold[0])
        pptr.append(pptr[-1] + len(x))
    out["probe_x"], out["probe_y"] = np.concatenate(px).astype(np.float32), np.concatenate(py).astype(np.int8)
    out["probe_threshold"], out["probe_ptr"] = np.array(pthr), np.array(pptr)
    n_adjacent = 1                                                         # the second probe: 1.0 and the float32 next to it

    dt = Trees("dt_")
    case = {k: [] for k in ("design", "criterion", "depth", "invariant")}
    n_inv = n_inv3 = 0
    for d, (X, y) in enumerate(ds):
        for ci, crit in enumerate(CRITERIA):
            for depth in DEPTHS:
                fits = [DecisionTreeClassifier(max_depth=depth, criterion=crit, random_state=s).fit(X, y).tree_ for s in range(SEEDS)]
                t = fits[0]
                inv = all(same_tree(t, f) for f in fits[1:])
                for k, v in zip(case, (d, ci, depth, inv)):
                    case[k].append(v)
                dt.add(t)
                n_inv += inv
                n_inv3 += inv and int((t.feature >= 0).sum()) >= 3
                if inv:
                    n_adjacent += adjacent_thresholds(X, t.feature, t.threshold)
    print("DT: %d of %d cases seed-invariant, %d of them with three or more splits" % (n_inv, len(case["design"]), n_inv3))
    if n_inv < 10 or n_inv3 < 4:
        raise SystemExit("fewer than 10 seed-invariant single trees, or fewer than 4 of them with three splits: strengthen the signal")
    for k, v in case.items():
        out["dt_" + k] = np.array(v)
    dt.into(out)
    out["n_invariant"], out["n_invariant_3_splits"] = n_inv, n_inv3

    deep = Trees("deep_")
    dcase = {k: [] for k in ("design", "seed", "criterion")}
    for d, (X, y) in enumerate(ds):
        for seed, crit in DEEP_SEEDS:
            t = DecisionTreeClassifier(criterion=crit, random_state=seed).fit(X, y).tree_
            for k, v in zip(dcase, (d, seed, CRITERIA.index(crit))):
                dcase[k].append(v)
            deep.add(t)
            n_adjacent += adjacent_thresholds(X, t.feature, t.threshold)
    for k, v in dcase.items():
        out["deep_" + k] = np.array(v)
    deep.into(out)
    print("deep: %d seeded trees, %d nodes" % (len(dcase["seed"]), deep.ptr[-1]))

    rf = Trees("rf_")
    rcase = {k: [] for k in ("design", "seed", "params")}
    proba, tree_ptr, sample_ptr = [], [0], [0]
    for d, seed, q in RF_CASES:
        X, y = ds[d]
        m = RandomForestClassifier(random_state=seed, **q).fit(X, y)
        rcase["design"].append(d)
        rcase["seed"].append(seed)
        rcase["params"].append(R.encode_params(q))
        for e in m.estimators_:
            rf.add(e.tree_)
            n_adjacent += adjacent_thresholds(X, e.tree_.feature, e.tree_.threshold)
        tree_ptr.append(tree_ptr[-1] + len(m.estimators_))
        proba.append(m.predict_proba(X).ravel())
        sample_ptr.append(sample_ptr[-1] + 2 * X.shape[0])
    for k, v in rcase.items():
        out["rf_" + k] = np.array(v)
    rf.into(out)
    out["rf_tree_ptr"], out["rf_sample_ptr"], out["rf_proba"] = np.array(tree_ptr), np.array(sample_ptr), np.concatenate(proba)
    print("RF: %d forests, %d trees, %d nodes" % (len(RF_CASES), tree_ptr[-1], rf.ptr[-1]))
    covered = {k: {q[k] for _, _, q in RF_CASES} for k in ("bootstrap", "max_features", "min_samples_leaf", "min_samples_split")}
    assert covered["bootstrap"] == {True, False} and covered["max_features"] == {None, "sqrt", "log2"}
    assert 4 in covered["min_samples_leaf"] and 10 in covered["min_samples_split"] and len(RF_CASES) >= 12

    out["n_adjacent_thresholds"] = n_adjacent
    print("%d recorded thresholds lie between adjacent float32 values" % n_adjacent)
    path = os.path.join(ROOT, "tests", "golden", "real_tree_kat.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    if size >= 1 << 20:
        os.remove(path)
        raise SystemExit("the fixture must stay under 1 MiB: trim the family")


if __name__ == "__main__":
    main()
