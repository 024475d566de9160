"""CPU tests (-m "not gpu") of the tree estimators on k-mer counts (`--real_counts` with -bc DT / -bc RF behind
PSK_TREE_COUNTS): the NumPy restatement (tests/count_tree_restated.py) against scikit-learn's recorded fits
(tests/golden/count_tree_kat.npz, tools/gen_count_tree_golden.py), model.Tree with thresholds, the scikit-learn .pkl of
trees that carry them, the option handling and the value check of the engine's count calls.  Where an estimator has to be
fitted without a GPU the engine call is served by the restatement (count_tree_restated.Engine).

Every compared figure here is ==: integer counts, thresholds that are exactly representable midpoints of two integers, and
impurities computed by the same Python-float expressions over the same C library that scikit-learn's Cython uses."""
import os

import numpy as np
import pytest

import count_tree_restated as C

NODE_KEYS = ("feature", "threshold", "left", "right", "n_node_samples", "counts", "impurity")


@pytest.fixture(scope="module")
def fx():
    return C.Fixture()


def assert_equal_tree(got, want, where):
    assert got["node_count"] == want["node_count"] and got["max_depth"] == want["max_depth"], where
    for k in NODE_KEYS:
        assert np.array_equal(got[k], want[k]), (where, k)


def test_fixture_holds_what_the_tests_need(fx):
    assert fx.sklearn_version == "1.7.2"
    assert [(D["n"], D["p"]) for D in fx.designs] == [(64, 12), (130, 40), (256, 40), (257, 70)]
    for D in fx.designs:
        distinct = [len(np.unique(D["X"][:, j])) for j in range(D["p"])]
        assert distinct[-1] == 1 and (max(distinct) > 64 or D["n"] <= 64) and D["X"].max() > 255
    inv = [c for c in fx.dt if c["invariant"] and c["depth"] <= 3
           and np.any((c["tree"]["feature"] >= 0) & (c["tree"]["threshold"] != 0.5))]
    assert len(inv) >= 12 and {(c["criterion"], c["depth"]) for c in inv} == {(cr, d) for cr in C.CRITERIA for d in (1, 2, 3)}
    assert len(fx.dt) == 80 and len(fx.rf) == 16 and sum(len(c["trees"]) for c in fx.rf) == 160


def test_restatement_equals_scikit_learn(fx):
    """Every tree of every recorded forest and every seed-invariant single tree: nodes, thresholds and impurities ==."""
    n = 0
    for k, c in enumerate(fx.dt):
        if c["invariant"]:
            D = fx.designs[c["design"]]
            assert_equal_tree(C.fit(D["X"], D["y"], np.ones(D["n"], dtype=bool), c["depth"], c["criterion"]), c["tree"], ("dt", k))
            n += 1
    assert n >= 22
    for k, c in enumerate(fx.rf):
        D, q = fx.designs[c["design"]], c["params"]
        s0, s1 = np.zeros(D["n"]), np.zeros(D["n"])
        for t, (seed, want) in enumerate(zip(C.tree_seeds(c["seed"], q["n_estimators"]), c["trees"])):
            w, state = C.tree_draws(seed, np.arange(D["n"]), D["n"], q["bootstrap"])
            got = C.fit_tree(D["X"], D["y"], w, state, q["criterion"], q["max_depth"], C.n_max_features(q["max_features"], D["p"]),
                             q["min_samples_leaf"], q["min_samples_split"])
            assert_equal_tree(got, want, ("rf", k, t))
            assert np.array_equal(got["leaf"], C.apply(want, D["X"])), ("rf", k, t)      # weight-0 samples by the thresholds
            s0 += got["frac0"]
            s1 += got["frac1"]
        assert float(np.abs(np.column_stack([s0, s1]) / q["n_estimators"] - c["proba"]).max()) <= 1e-15, k


def test_a_0_1_design_is_a_count_design(fx):
    import forest_restated as FR
    import tree_restated as TR
    D = fx.designs[1]
    X = (D["X"] > 1).astype(np.float64)
    tr = np.arange(D["n"]) % 3 != 0
    a, b = C.fit(X, D["y"], tr, 6, "entropy"), TR.fit(X, D["y"], tr, 6, "entropy")
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["threshold"], np.where(a["feature"] >= 0, 0.5, -2.0))
    w, state = C.tree_draws(5, np.nonzero(tr)[0], D["n"], True)
    a, b = C.fit_tree(X, D["y"], w, state, "gini", None, 6, 2, 2), FR.fit_tree(X, D["y"], w, state, "gini", None, 6, 2, 2)
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["threshold"], np.where(a["feature"] >= 0, 0.5, -2.0))


def test_tree_applies_its_thresholds(fx):
    from phenotypeseeker_amd import model as M
    D = fx.designs[2]
    m = M.DecisionTree(max_depth=4, counts=True).fit(D["X"], D["y"], C.Engine())
    want = C.fit(D["X"], D["y"], np.ones(D["n"], dtype=bool), 4, "gini")
    assert np.array_equal(m.tree_.threshold, want["threshold"]) and np.any(m.tree_.threshold > 0.5)
    assert np.array_equal(m.tree_.apply(D["X"]), want["leaf"])
    rng = np.random.default_rng(5)
    Xn = rng.poisson(1.5, (40, D["p"])).astype(np.float64)
    assert np.array_equal(m.tree_.apply(Xn), C.apply(want, Xn))
    assert np.array_equal(m.predict_proba(D["X"])[:, 1], want["frac"])
    # the switch is the engine's: neither the repr nor the exported parameters show it, and a clone keeps it
    assert repr(m) == "DecisionTreeClassifier(max_depth=4)" and "counts" not in m._sklearn_params()
    assert m._clone(max_depth=2).counts is True and M.DecisionTree().counts is False
    f = M.RandomForest(n_estimators=3, random_state=1, counts=True)
    assert "counts" not in repr(f) and "counts" not in f.get_params() and f._clone(n_estimators=2).counts is True
    f.fit(D["X"], D["y"], C.Engine())
    assert all(e.counts and np.any(e.tree_.threshold > 0.5) for e in f.estimators_) and "counts" not in f.estimators_[0]._sklearn_params()
    # without thresholds a Tree is the 0/1 tree it was
    t = M.Tree(3, [0, -2, -2], [1, -1, -1], [2, -1, -1], [4, 2, 2], [[2, 2], [2, 0], [0, 2]], [0.5, 0.0, 0.0], 1)
    assert list(t.threshold) == [0.5, -2.0, -2.0]


def test_the_recorded_search_and_its_model_file(tmp_path, fx):
    """model.RandomizedSearch over RandomForest(counts=True), served by the restatement, reproduces scikit-learn's recorded
    cv_results_; its .pkl loads with joblib into scikit-learn's own classes, thresholds included."""
    from phenotypeseeker_amd import model as M, skpickle
    g = fx.search
    D = fx.designs[g["design"]]
    rs = M.RandomizedSearch(M.RandomForest(random_state=g["seed"], counts=True), g["grid"], g["n_iter"], g["cv"],
                            random_state=g["seed"]).fit(D["X"], D["y"], C.Engine())
    r = rs.cv_results_
    assert r["params"] == g["params"] and rs.best_params_ == g["best"]
    for f in range(g["cv"]):
        assert np.array_equal(r["split%d_test_score" % f], g["splits"][:, f]), f
    assert np.array_equal(r["mean_test_score"], g["mean"]) and np.array_equal(r["rank_test_score"], g["rank"])
    assert float(np.abs(rs.predict_proba(D["X"]) - g["proba"]).max()) <= 1e-15
    pytest.importorskip("sklearn")
    joblib = pytest.importorskip("joblib")
    import warnings
    rng = np.random.default_rng(9)
    Xn = np.vstack([D["X"], rng.poisson(2.0, (30, D["p"])).astype(np.float64)])
    dt = M.GridSearch(M.DecisionTree(counts=True), {"max_depth": [3], "criterion": ["gini"]}, cv=3).fit(D["X"], D["y"], C.Engine())
    for name, search in (("rf", rs), ("dt", dt)):
        shell = search.to_sklearn_shell()
        assert shell is not None, "no template for the installed scikit-learn: run tools/make_sklearn_shells.py"
        path = os.path.join(tmp_path, name + ".pkl")
        with open(path, "wb") as f:
            f.write(skpickle.dumps({"model": shell, "kmers": np.array(["ACGT"] * D["p"], dtype=object), "pca": False, "pred_scale": "binary"}))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            sk = joblib.load(path)["model"]
            be = sk.best_estimator_
            ours = search.best_estimator_
            pairs = zip(be.estimators_, ours.estimators_) if name == "rf" else [(be, ours)]
            for a, b in pairs:
                assert type(a.tree_).__module__ == "sklearn.tree._tree"
                assert np.array_equal(a.tree_.threshold, b.tree_.threshold) and np.any(a.tree_.threshold > 0.5)
                assert not np.any(a.tree_.missing_go_to_left)
            assert "counts" not in be.get_params()
            assert np.array_equal(sk.predict_proba(Xn), search.predict_proba(Xn)) and np.array_equal(sk.predict(Xn), search.predict(Xn))
        fast = skpickle.load_linear_package(path)                 # what `phenotypeseeker prediction` reads the file with
        assert fast is not None and np.array_equal(fast["model"].predict_proba(Xn), search.predict_proba(Xn))


DT_OFF = "The decision tree on the GPU engine takes the 0/1 presence matrix only: --real_counts is not supported with -bc DT."
RF_OFF = "The random forest on the GPU engine takes the 0/1 presence matrix only: --real_counts is not supported with -bc RF."


def test_real_counts_sits_behind_the_knob(tmp_path, monkeypatch):
    from test_host_modeling import _setup
    monkeypatch.setenv("PSK_DT", "1")
    monkeypatch.setenv("PSK_RF", "1")
    for flag in (None, "0"):                                      # off: both refusals as they were
        if flag is None:
            monkeypatch.delenv("PSK_TREE_COUNTS", raising=False)
        else:
            monkeypatch.setenv("PSK_TREE_COUNTS", flag)
        for bc, msg in (("DT", DT_OFF), ("RF", RF_OFF)):
            with pytest.raises(SystemExit) as e:
                _setup(tmp_path, "ds_bonf", ["-bc", bc, "--real_counts"])
            assert str(e.value) == msg
    monkeypatch.setenv("PSK_TREE_COUNTS", "1")
    for bc, cls, text in (("DT", "DecisionTree", "DecisionTreeClassifier()"), ("RF", "RandomForest", "RandomForestClassifier(random_state=0)")):
        M, _ = _setup(tmp_path, "ds_bonf", ["-bc", bc, "--real_counts"])
        assert M.phenotypes.binary_classifier == bc and M.phenotypes.real_counts
        est = M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()[0]
        assert type(est).__name__ == cls and est.counts is True and repr(est) == text
        M, _ = _setup(tmp_path, "ds_bonf", ["-bc", bc])           # without --real_counts the estimator is the 0/1 one
        assert M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()[0].counts is False
        for extra in (["--pca"], ["--pca", "--real_counts"]):
            with pytest.raises(SystemExit) as e:
                _setup(tmp_path, "ds_bonf", ["-bc", bc] + extra)
            assert "--pca is not supported with -bc %s" % bc in str(e.value)
    monkeypatch.delenv("PSK_DT")                                  # the knob opens nothing by itself
    with pytest.raises(SystemExit) as e:
        _setup(tmp_path, "ds_bonf", ["-bc", "DT", "--real_counts"])
    assert "outside the accelerated path" in str(e.value)


def test_the_engine_checks_the_values_before_the_cast():
    from phenotypeseeker_amd.engine import PskContext
    ok = PskContext._count_design(np.array([[0.0, 3.0], [float(1 << 24), 255.0]]), "tree_fit_counts")
    assert ok.dtype == np.float32 and ok.flags["C_CONTIGUOUS"] and ok[1, 0] == 16777216.0
    for bad in (-1.0, 0.5, np.nan, np.inf, float((1 << 24) + 1)):       # (2^24 + 1 rounds to 2^24 as a float32)
        with pytest.raises(ValueError) as e:
            PskContext._count_design(np.array([[0.0, 1.0], [bad, 2.0]]), "forest_fit_counts")
        assert "forest_fit_counts" in str(e.value) and "2^24" in str(e.value)
        with pytest.raises(ValueError):
            C.Engine().tree_fit_counts(np.array([[0.0, 1.0], [bad, 2.0]]), [0, 1], [0, 0], [1], ["gini"], [-1])


def test_abi_names_the_count_entry_points():
    from phenotypeseeker_amd import _lib
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psk.h")) as f:
        header = f.read()
    assert "---- f9:" in header and "---- f10:" in header and "#define PSK_TREE_PLANE_CAP 1048576" in header
    for name, base in (("psk_tree_fit_counts", "psk_tree_fit"), ("psk_forest_fit_counts", "psk_forest_fit")):
        assert name in _lib.exported_names()
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib._SIGNATURES[name][1]) == len(_lib._SIGNATURES[base][1]) + 1, name
        assert decl.rstrip().endswith("double *threshold_out")
