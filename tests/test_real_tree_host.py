"""CPU tests (-m "not gpu") of the tree estimators on real-valued designs (`--pca` with -bc DT / -bc RF behind PSK_TREE_PCA):
the NumPy restatement (tests/real_tree_restated.py) against scikit-learn's recorded fits (tests/golden/real_tree_kat.npz,
tools/gen_real_tree_golden.py), the four probes of what scikit-learn 1.7.2 takes for equal values, the restatement against
count_tree_restated on the recorded count designs, the model layer's third engine route and its .pkl, the knob, and the
engine's value check.  Where an estimator has to be fitted without a GPU the engine call is served by the restatement.

Every compared figure is ==: integer counts, thresholds that are one f64 expression of two float32 values, and impurities
computed by the same Python-float expressions over the same C library that scikit-learn's Cython uses."""
import os

import numpy as np
import pytest

import count_tree_restated as C
import real_tree_restated as R

NODE_KEYS = ("feature", "threshold", "left", "right", "n_node_samples", "counts", "impurity")


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


def assert_equal_tree(got, want, where):
    assert got["node_count"] == want["node_count"] and got["max_depth"] == want["max_depth"], where
    for k in NODE_KEYS:
        assert np.array_equal(got[k], want[k]), (where, k)


def test_fixture_holds_what_the_tests_need(fx):
    assert fx.sklearn_version == "1.7.2"
    assert [(D["n"], D["p"]) for D in fx.designs] == [(65, 5), (257, 9), (130, 40), (96, 1100)]
    X = fx.designs[2]["X32"]
    assert np.all(X[:, 38] == 0) and np.all(X[:, 39] == 0) and set(np.signbit(X[:, 39]).tolist()) == {True, False}
    assert min(len(np.unique(X[:, j])) for j in range(38)) < 60                       # tied scores
    assert len(fx.probes) == 4 and len(fx.dt) == 24 and len(fx.deep) == 16 and len(fx.rf) >= 12
    inv = [c for c in fx.dt if c["invariant"]]
    assert len(inv) == fx.n_invariant >= 10
    assert sum(int((c["tree"]["feature"] >= 0).sum()) >= 3 for c in inv) == fx.n_invariant_3_splits >= 4
    assert fx.n_adjacent_thresholds >= 1
    q = [c["params"] for c in fx.rf]
    assert {v["bootstrap"] for v in q} == {True, False} and {v["max_features"] for v in q} == {None, "sqrt", "log2"}
    assert any(v["min_samples_leaf"] == 4 for v in q) and any(v["min_samples_split"] == 10 for v in q)
    assert all(v["n_estimators"] <= 20 for v in q)
    from phenotypeseeker_amd.modeling import RF_GRID
    assert all(v[k] in RF_GRID[k] for v in q for k in RF_GRID)


def test_restatement_equals_scikit_learn(fx):
    """Every seed-invariant single tree, every seeded deep tree (through the forest builder with one all-ones tree and
    max_features = p) and every tree of every recorded forest: nodes, thresholds and impurities ==."""
    n_dt = n_rf = 0
    for k, c in enumerate(fx.dt):
        if c["invariant"]:
            D = fx.designs[c["design"]]
            assert_equal_tree(R.fit(D["X"], D["y"], np.ones(D["n"], dtype=bool), c["depth"], c["criterion"]), c["tree"], ("dt", k))
            n_dt += 1
    assert n_dt == fx.n_invariant
    for k, c in enumerate(fx.deep):
        D = fx.designs[c["design"]]
        got = R.seeded_tree(D["X"], D["y"], c["seed"], c["criterion"])
        assert_equal_tree(got, c["tree"], ("deep", k))
        assert np.array_equal(got["leaf"], R.apply(c["tree"], D["X"])), ("deep", k)
    adjacent = 0
    for k, c in enumerate(fx.rf):
        D, q = fx.designs[c["design"]], c["params"]
        s0, s1 = np.zeros(D["n"]), np.zeros(D["n"])
        for t, (seed, want) in enumerate(zip(R.tree_seeds(c["seed"], q["n_estimators"]), c["trees"])):
            w, state = R.tree_draws(seed, np.arange(D["n"]), D["n"], q["bootstrap"])
            got = R.fit_tree(D["X"], D["y"], w, state, q["criterion"], q["max_depth"], R.n_max_features(q["max_features"], D["p"]),
                             q["min_samples_leaf"], q["min_samples_split"])
            assert_equal_tree(got, want, ("rf", k, t))
            assert np.array_equal(got["leaf"], R.apply(want, D["X"])), ("rf", k, t)      # weight-0 samples by the thresholds
            s0 += got["frac0"]
            s1 += got["frac1"]
            n_rf += 1
            for j, thr in zip(got["feature"], got["threshold"]):
                if j >= 0:
                    col = D["X32"][:, j]
                    adjacent += bool(np.nextafter(col[col <= thr].max(), np.float32(np.inf)) == col[col > thr].min())
        assert float(np.abs(np.column_stack([s0, s1]) / q["n_estimators"] - c["proba"]).max()) <= 1e-15, k
    assert n_rf == sum(len(c["trees"]) for c in fx.rf) >= 120
    assert adjacent >= 1                         # a threshold between two adjacent float32 values was reproduced


def test_the_probes_split_where_scikit_learn_split(fx):
    """Two values 8.9e-8 apart, 1.0 and the float32 next to it, and the first / second gap of three values 3 x 2^-25 apart:
    scikit-learn 1.7.2 as built splits all four (the FEATURE_THRESHOLD of its source is not in effect), and so do the rules."""
    u = 2.0 ** -25
    a = float(np.float32(0.25))
    want = [a / 2.0 + float(np.float32(0.25 + 3 * u)) / 2.0, 1.0 / 2.0 + float(np.nextafter(np.float32(1.0), np.float32(2.0))) / 2.0,
            a / 2.0 + float(np.float32(0.25 + 3 * u)) / 2.0, float(np.float32(0.25 + 3 * u)) / 2.0 + float(np.float32(0.25 + 6 * u)) / 2.0]
    for k, (pr, thr) in enumerate(zip(fx.probes, want)):
        assert pr["threshold"] == thr, k                                            # what scikit-learn recorded
        x = pr["x"].reshape(-1, 1)
        for crit in R.CRITERIA:
            t = R.fit(x, pr["y"], np.ones(len(x), dtype=bool), 3, crit)
            assert t["node_count"] == 3 and t["threshold"][0] == thr, (k, crit)
            f = R.fit_tree(x, pr["y"], np.ones(len(x), dtype=int), 5, crit, None, 1, 1, 2)
            assert f["node_count"] == 3 and f["threshold"][0] == thr, (k, crit)
    assert abs(fx.probes[0]["threshold"] - (0.25 + 4.47e-8)) < 1e-10
    # -0.0 and +0.0 are one value; the midpoint that rounds to hi is replaced by lo
    z = np.array([-0.0, 0.0] * 4, dtype=np.float32).reshape(-1, 1)
    assert R.fit(z, [0, 1] * 4, np.ones(8, dtype=bool), 3, "gini")["node_count"] == 1
    tiny = float(np.float32(1e-45))
    assert R.threshold(0.0, 5e-324) == 0.0 and R.threshold(0.0, tiny) == tiny / 2.0 and R.threshold(-1.0, 1.0) == 0.0


def test_on_a_count_design_it_is_the_count_restatement():
    cf = C.Fixture()
    for d, D in enumerate(cf.designs):
        tr = np.arange(D["n"]) % 3 != 0
        for crit, depth in (("gini", 3), ("entropy", 10)):
            a, b = R.fit(D["X"], D["y"], tr, depth, crit), C.fit(D["X"], D["y"], tr, depth, crit)
            assert set(a) == set(b)
            for k in b:
                assert np.array_equal(a[k], b[k]), (d, crit, k)
        w, state = C.tree_draws(5 + d, np.nonzero(tr)[0], D["n"], True)
        a = R.fit_tree(D["X"], D["y"], w, state, "entropy", None, 6, 2, 5)
        b = C.fit_tree(D["X"], D["y"], w, state, "entropy", None, 6, 2, 5)
        for k in b:
            assert np.array_equal(a[k], b[k]), (d, k)


def test_the_third_engine_route_and_its_model_file(tmp_path, fx):
    """DecisionTree / RandomForest with real=True call tree_fit_real / forest_fit_real; the switch shows nowhere; the .pkl of
    such a search loads with joblib into scikit-learn's own classes and predicts what the package predicts."""
    from phenotypeseeker_amd import model as M, skpickle
    D = fx.designs[1]
    m = M.DecisionTree(max_depth=4, real=True).fit(D["X"], D["y"], R.Engine())
    want = R.fit(D["X"], D["y"], np.ones(D["n"], dtype=bool), 4, "gini")
    assert np.array_equal(m.tree_.threshold, want["threshold"]) and np.array_equal(m.tree_.apply(D["X"]), want["leaf"])
    assert np.array_equal(m.predict_proba(D["X"])[:, 1], want["frac"])
    assert repr(m) == "DecisionTreeClassifier(max_depth=4)" and "real" not in m._sklearn_params()
    assert m._clone(max_depth=2).real is True and M.DecisionTree().real is False and M.DecisionTree(counts=True).real is False
    f = M.RandomForest(n_estimators=3, random_state=1, real=True)
    assert "real" not in repr(f) and "real" not in f.get_params() and f._clone(n_estimators=2).real is True
    f.fit(D["X"], D["y"], R.Engine())
    assert all(e.real and not e.counts for e in f.estimators_) and "real" not in f.estimators_[0]._sklearn_params()
    pytest.importorskip("sklearn")
    joblib = pytest.importorskip("joblib")
    import warnings
    from phenotypeseeker_amd.modeling import RF_GRID
    rs = M.RandomizedSearch(M.RandomForest(random_state=3, real=True), dict(RF_GRID, n_estimators=[10, 20]), 2, 3,
                            random_state=3).fit(D["X"], D["y"], R.Engine())
    dt = M.GridSearch(M.DecisionTree(real=True), {"max_depth": [3, 6], "criterion": ["gini", "entropy"]}, cv=3).fit(D["X"], D["y"], R.Engine())
    rng = np.random.default_rng(9)
    Xn = np.vstack([D["X"], rng.normal(0.0, 1.0, (30, D["p"])).astype(np.float32).astype(np.float64)])
    for name, search in (("rf", rs), ("dt", dt)):
        shell = search.to_sklearn_shell()
        assert shell is not None, "no template for the installed scikit-learn: run tools/make_sklearn_shells.py"
        path = os.path.join(tmp_path, name + ".pkl")
        with open(path, "wb") as fh:
            fh.write(skpickle.dumps({"model": shell, "kmers": np.array(["ACGT"] * D["p"], dtype=object), "pca": False, "pred_scale": "binary"}))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            sk = joblib.load(path)["model"]
            be, ours = sk.best_estimator_, search.best_estimator_
            pairs = zip(be.estimators_, ours.estimators_) if name == "rf" else [(be, ours)]
            for a, b in pairs:
                assert type(a.tree_).__module__ == "sklearn.tree._tree"
                assert np.array_equal(a.tree_.threshold, b.tree_.threshold) and np.any(a.tree_.threshold[a.tree_.feature >= 0] != 0.5)
            assert "real" not in be.get_params()
            assert np.array_equal(sk.predict_proba(Xn), search.predict_proba(Xn)) and np.array_equal(sk.predict(Xn), search.predict(Xn))
        fast = skpickle.load_linear_package(path)                 # what `phenotypeseeker prediction` reads the file with
        assert fast is not None and np.array_equal(fast["model"].predict_proba(Xn), search.predict_proba(Xn))


DT_OFF = "The decision tree on the GPU engine takes the 0/1 presence matrix only: --pca is not supported with -bc DT."
RF_OFF = "The random forest on the GPU engine takes the 0/1 presence matrix only: --pca is not supported with -bc RF."
NB_OFF = "The naive Bayes classifier on the GPU engine takes the k-mer presence matrix only: --pca is not supported with -bc NB."


def test_pca_with_the_trees_sits_behind_the_knob(tmp_path, monkeypatch):
    from test_host_modeling import _setup
    for knob in ("PSK_DT", "PSK_RF", "PSK_NB", "PSK_PCA"):
        monkeypatch.setenv(knob, "1")
    monkeypatch.delenv("PSK_TREE_COUNTS", raising=False)
    for flag in (None, "0"):                                      # off: both refusals as they were, word for word
        if flag is None:
            monkeypatch.delenv("PSK_TREE_PCA", raising=False)
        else:
            monkeypatch.setenv("PSK_TREE_PCA", flag)
        for bc, msg in (("DT", DT_OFF), ("RF", RF_OFF)):
            with pytest.raises(SystemExit) as e:
                _setup(tmp_path, "ds_bonf", ["-bc", bc, "--pca"])
            assert str(e.value) == msg
    monkeypatch.setenv("PSK_TREE_PCA", "1")
    for bc, cls, text in (("DT", "DecisionTree", "DecisionTreeClassifier()"), ("RF", "RandomForest", "RandomForestClassifier(random_state=0)")):
        for extra in ([], ["--real_counts"]):                     # the PCA may be of the counts: the trees see scores either way
            M, _ = _setup(tmp_path, "ds_bonf", ["-bc", bc, "--pca"] + extra)
            assert M.phenotypes.binary_classifier == bc and M.phenotypes.pca is True
            est = M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()[0]
            assert type(est).__name__ == cls and est.real is True and est.counts is False and repr(est) == text
        M, _ = _setup(tmp_path, "ds_bonf", ["-bc", bc])           # without --pca the estimator is the 0/1 one
        est = M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()[0]
        assert est.real is False and est.counts is False
        with pytest.raises(SystemExit) as e:                      # the knob opens --real_counts only together with --pca
            _setup(tmp_path, "ds_bonf", ["-bc", bc, "--real_counts"])
        assert "--real_counts is not supported with -bc %s" % bc in str(e.value)
    with pytest.raises(SystemExit) as e:                          # refusals that stay
        _setup(tmp_path, "ds_bonf", ["-bc", "NB", "--pca"])
    assert str(e.value) == NB_OFF
    monkeypatch.setenv("PSK_PCA", "0")                            # the knob does not stand in for PSK_PCA
    with pytest.raises(SystemExit) as e:
        _setup(tmp_path, "ds_bonf", ["-bc", "DT", "--pca"])
    assert str(e.value) == "--pca is outside the accelerated path."
    monkeypatch.setenv("PSK_PCA", "1")
    monkeypatch.delenv("PSK_DT")                                  # ... nor for the estimator's
    with pytest.raises(SystemExit) as e:
        _setup(tmp_path, "ds_bonf", ["-bc", "DT", "--pca"])
    assert "outside the accelerated path" in str(e.value)


def test_the_engine_checks_the_values_after_the_cast():
    from phenotypeseeker_amd.engine import PskContext
    ok = PskContext._real_design(np.array([[-0.0, 3.5], [1e-40, -255.25]]), "tree_fit_real")
    assert ok.dtype == np.float32 and ok.flags["C_CONTIGUOUS"] and ok[1, 1] == -255.25
    for bad in (np.nan, np.inf, -np.inf, 1e39):                   # (1e39 is an infinity as a float32)
        with np.errstate(over="ignore"):
            with pytest.raises(ValueError) as e:
                PskContext._real_design(np.array([[0.0, 1.0], [bad, 2.0]]), "forest_fit_real")
            assert "forest_fit_real" in str(e.value) and "finite" in str(e.value)
            with pytest.raises(ValueError):
                R.Engine().tree_fit_real(np.array([[0.0, 1.0], [bad, 2.0]]), [0, 1], [0, 0], [1], ["gini"], [-1])


def test_abi_names_the_real_entry_points():
    from phenotypeseeker_amd import _lib
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psk.h")) as f:
        header = f.read()
    assert "---- f13:" in header and "6 n p bytes" in header
    for name, base in (("psk_tree_fit_real", "psk_tree_fit_counts"), ("psk_forest_fit_real", "psk_forest_fit_counts")):
        assert name in _lib.exported_names()
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib._SIGNATURES[name][1]) == len(_lib._SIGNATURES[base][1]), name
        assert decl.rstrip().endswith("double *threshold_out")
