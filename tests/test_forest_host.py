"""CPU tests (-m "not gpu") of the random forest's host side: the NumPy restatement of scikit-learn's seeded forest
(tests/forest_restated.py) against scikit-learn's recorded fits (tests/golden/forest_kat.npz, tools/gen_forest_golden.py) on
EVERY case, the randomized search and its candidate draws, the scikit-learn .pkl of a fitted search and the `-bc RF` option
handling.  Where an estimator has to be fitted without a GPU, the engine call is served by the restatement
(forest_restated.Engine): the host code under test is the package's own.

Tolerance: as in test_tree_host.py -- impurities, probabilities and importances are f64 functions of small integers with
results bounded by 1, a handful of roundings apart between two correct evaluations: 1e-12 absolute.  Integers are ==."""
import os

import numpy as np
import pytest

import forest_restated as R

ATOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


def assert_same_tree(got, want, where):
    """Integers ==, node order included (counts: the weighted class counts, so weighted_n_node_samples too); impurities
    within ATOL."""
    assert got["node_count"] == want["node_count"] and got["max_depth"] == want["max_depth"], where
    for k in ("feature", "left", "right", "n_node_samples", "counts"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert float(np.abs(got["impurity"] - want["impurity"]).max()) <= ATOL, where


def restated(D, c):
    q = c["params"]
    return R.fit_forest(D["X"], D["y"], c["seed"], **q)


def test_fixture_holds_what_the_tests_need(fx):
    assert fx.sklearn_version == "1.7.2"
    shapes = {(D["n"], D["p"]) for D in fx.designs if D["kind"] != "search"}
    assert {n for n, _ in shapes} == {40, 63, 64, 65, 130} and {p for _, p in shapes} == {1, 5, 24, 70}
    assert {D["kind"] for D in fx.designs} == {"plain", "mixed", "staircase", "search"}
    for D in fx.designs:
        if D["kind"] == "mixed":      # a duplicated, a complemented, an all-zero and an all-one column
            X = D["X"]
            assert np.array_equal(X[:, 1], X[:, 0]) and np.array_equal(X[:, 2], 1 - X[:, 0]) and not X[:, 3].any() and X[:, 4].all()
    assert len(fx.cases) >= 40 and all(3 <= len(c["trees"]) <= 10 for c in fx.cases)
    for key, vals in (("criterion", {"gini", "entropy"}), ("bootstrap", {True, False}), ("max_features", {None, "sqrt", "log2"}),
                      ("min_samples_leaf", {1, 2, 4}), ("min_samples_split", {2, 5, 10}), ("max_depth", {4, 20, None})):
        assert {c["params"][key] for c in fx.cases} == vals, key
    stair = [c for c in fx.cases if fx.designs[c["design"]]["kind"] == "staircase"]
    assert max(t["max_depth"] for c in stair for t in c["trees"]) >= 20
    assert any(t["max_depth"] == 20 and c["params"]["max_depth"] == 20 for c in stair for t in c["trees"])     # stopped by the cap
    # bootstrap trees: weighted counts above the distinct ones
    assert any(np.any(t["counts"].sum(axis=1) > t["n_node_samples"]) for c in fx.cases if c["params"]["bootstrap"] for t in c["trees"])
    g = fx.search
    D = fx.designs[g["design"]]
    assert (D["n"], D["p"], g["cv"], g["n_iter"], len(g["params"])) == (60, 30, 3, 6, 6) and g["grid"]["n_estimators"] == [5, 10]
    assert R.grid_size(g["grid"]) == 648 and g["splits"].shape == (6, 3)
    assert sorted(fx.draws) == [0, 1, 2, 3, 4] and all(len(v) == 25 for v in fx.draws.values())
    assert R.grid_size(R.REFERENCE_GRID) == 10692
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forest_kat.npz")) < 1 << 20


def test_restatement_equals_scikit_learn_on_every_case(fx):
    n = n_trees = 0
    for k, c in enumerate(fx.cases):
        D = fx.designs[c["design"]]
        r = restated(D, c)
        assert len(r["trees"]) == len(c["trees"]) == c["params"]["n_estimators"], k
        for t, (got, want) in enumerate(zip(r["trees"], c["trees"])):
            assert_same_tree(got, want, (k, t))
            assert np.all(got["leaf"] >= 0) and np.all(got["left"][got["leaf"]] == -1), (k, t)
            n_trees += 1
        assert float(np.abs(r["proba"] - c["proba"]).max()) <= ATOL, k
        assert float(np.abs(R.forest_importances(r["trees"], D["p"]) - c["importances"]).max()) <= ATOL, k
        n += 1
    assert n == len(fx.cases) and n_trees == sum(len(c["trees"]) for c in fx.cases)


def test_live_agreement_with_scikit_learn_on_fresh_seeds(fx):
    pytest.importorskip("sklearn")
    from sklearn.ensemble import RandomForestClassifier
    rng = np.random.default_rng(2024)
    for k in range(6):
        D = fx.designs[(1, 3, 4)[k % 3]]
        q = dict(criterion=R.CRITERIA[k % 2], bootstrap=k % 3 != 0, max_features=R.MAX_FEATURES[k % 3], min_samples_leaf=(1, 2, 4)[k % 3],
                 min_samples_split=(2, 5, 10)[(k // 2) % 3], max_depth=(None, 4, 20)[k % 3], n_estimators=4)
        seed = int(rng.integers(0, 2 ** 31))
        m = RandomForestClassifier(random_state=seed, **q).fit(D["X"], D["y"])
        r = R.fit_forest(D["X"], D["y"], seed, **q)
        for e, got in zip(m.estimators_, r["trees"]):
            t = e.tree_
            assert np.array_equal(t.feature, got["feature"]) and np.array_equal(t.children_left, got["left"]), (k, seed)
            assert np.array_equal(t.children_right, got["right"]) and np.array_equal(t.n_node_samples, got["n_node_samples"]), (k, seed)
            assert np.array_equal(t.weighted_n_node_samples, got["counts"].sum(axis=1)), (k, seed)
            assert float(np.abs(t.impurity - got["impurity"]).max()) <= ATOL
        assert float(np.abs(m.predict_proba(D["X"]) - r["proba"]).max()) <= ATOL
        assert float(np.abs(m.feature_importances_ - R.forest_importances(r["trees"], D["p"])).max()) <= ATOL


def test_weight_zero_samples_are_routed_and_masking_equals_subsetting(fx):
    D = fx.designs[4]
    rows = np.nonzero(np.arange(D["n"]) % 3 != 1)[0]
    full = R.fit_forest(D["X"], D["y"], 5, rows=rows, n_estimators=3, max_depth=6)
    sub = R.fit_forest(D["X"][rows], D["y"][rows], 5, n_estimators=3, max_depth=6)
    for a, b in zip(full["trees"], sub["trees"]):
        assert_same_tree(a, b, "masking == sub-setting")
        assert np.all(a["leaf"] >= 0) and np.array_equal(a["leaf"][rows], b["leaf"])
    assert np.array_equal(full["proba"][rows], sub["proba"])


def test_candidate_draws_of_the_full_grid_equal_the_record(fx):
    from phenotypeseeker_amd import model as M
    from phenotypeseeker_amd.modeling import RF_GRID
    assert RF_GRID == R.REFERENCE_GRID and list(RF_GRID) == list(R.REFERENCE_GRID)
    for seed, want in fx.draws.items():
        assert R.sampled_indices(R.REFERENCE_GRID, 25, seed) == want, seed
        rs = M.RandomizedSearch(M.RandomForest(random_state=seed), RF_GRID, 25, 10, random_state=seed)
        assert rs.sampled_indices() == want, seed
        assert rs.candidates() == [R.grid_point(R.REFERENCE_GRID, i) for i in want]
        assert list(rs.candidates()[0]) == sorted(RF_GRID, reverse=True)         # ParameterGrid's key order
    assert M.RandomizedSearch.max_n_iter(10692) == 106
    for n_iter in (0, 107, 5000, 20000):                      # outside the restated regime (20000: capped to the grid, then pool)
        with pytest.raises(ValueError) as e:
            M.RandomizedSearch(M.RandomForest(), RF_GRID, n_iter, 10).candidates()
        assert "1..106" in str(e.value)
    assert len(M.RandomizedSearch(M.RandomForest(), RF_GRID, 106, 10).candidates()) == 106


@pytest.fixture(scope="module")
def searched(fx):
    from phenotypeseeker_amd import model as M
    g = fx.search
    D = fx.designs[g["design"]]
    return M.RandomizedSearch(M.RandomForest(random_state=g["seed"]), g["grid"], g["n_iter"], g["cv"], random_state=g["seed"]).fit(
        D["X"], D["y"], R.Engine())


def test_randomized_search_over_the_restatement_equals_the_record(fx, searched):
    from phenotypeseeker_amd import model as M
    g, rs = fx.search, searched
    D = fx.designs[g["design"]]
    r = rs.cv_results_
    assert r["params"] == g["params"]
    for f in range(g["cv"]):
        assert np.array_equal(r["split%d_test_score" % f], g["splits"][:, f]), f
    assert np.array_equal(r["mean_test_score"], g["mean"]) and np.allclose(r["std_test_score"], g["std"], rtol=0, atol=1e-15)
    assert np.array_equal(r["rank_test_score"], g["rank"])
    assert rs.best_params_ == g["best"] and rs.best_index_ == int(np.argmin(g["rank"]))
    assert set(r) == set(M.GridSearch(M.DecisionTree(), {"max_depth": [1], "criterion": ["gini"]}, cv=3).fit(
        D["X"], D["y"], __import__("tree_restated").Engine()).cv_results_)
    be = rs.best_estimator_
    assert isinstance(be, M.RandomForest) and be.get_params() == g["best"] and len(be.estimators_) == g["best"]["n_estimators"]
    assert float(np.abs(rs.predict_proba(D["X"]) - g["proba"]).max()) <= ATOL
    assert float(np.abs(be.feature_importances_ - g["importances"]).max()) <= ATOL
    assert np.array_equal(rs.predict(D["X"]), np.argmax(g["proba"], axis=1))
    assert rs.score(D["X"], D["y"]) == np.mean(np.argmax(g["proba"], axis=1) == D["y"])
    assert repr(rs.estimator) == "RandomForestClassifier(random_state=%d)" % g["seed"]


def test_estimator_protocol(fx):
    from phenotypeseeker_amd import model as M
    c = [c for c in fx.cases if c["params"]["bootstrap"] and fx.designs[c["design"]]["kind"] == "mixed"][0]
    D, q = fx.designs[c["design"]], c["params"]
    m = M.RandomForest(random_state=c["seed"], **q).fit(D["X"], D["y"], R.Engine())
    assert len(m.estimators_) == q["n_estimators"]
    for e, want in zip(m.estimators_, c["trees"]):
        t = e.tree_
        assert isinstance(e, M.DecisionTree) and isinstance(t, M.Tree)
        assert np.array_equal(t.feature, want["feature"]) and np.array_equal(t.children_left, want["left"])
        assert np.array_equal(t.children_right, want["right"]) and np.array_equal(t.n_node_samples, want["n_node_samples"])
        assert np.array_equal(t.weighted_n_node_samples, want["counts"].sum(axis=1).astype(np.float64))
        assert t.value.shape == (t.node_count, 1, 2) and float(np.abs(t.value.sum(axis=2) - 1.0).max()) <= ATOL
    assert [e.random_state for e in m.estimators_] == R.tree_seeds(c["seed"], q["n_estimators"])
    assert float(np.abs(m.predict_proba(D["X"]) - c["proba"]).max()) <= ATOL
    assert float(np.abs(m.feature_importances_ - c["importances"]).max()) <= ATOL
    assert np.array_equal(m.predict(D["X"]), np.argmax(c["proba"], axis=1))
    tie = M.RandomForest(n_estimators=2, bootstrap=False, max_features=None).fit(np.array([[0.0], [0.0], [1.0], [1.0]]), np.array([0, 1, 0, 1]), R.Engine())
    assert list(tie.predict(np.array([[0.0], [1.0]]))) == [0, 0]         # equal probabilities: class 0
    dt = M.DecisionTree(max_depth=2).fit(D["X"], D["y"], __import__("tree_restated").Engine())    # DT's tree is what it was
    assert np.array_equal(dt.tree_.weighted_n_node_samples, dt.tree_.n_node_samples.astype(np.float64))
    for bad in (dict(criterion="log_loss"), dict(max_features=0.5), dict(n_estimators=0), dict(min_samples_split=1)):
        with pytest.raises(ValueError):
            M.RandomForest(**bad)
    with pytest.raises(ValueError):
        M.RandomForest(random_state=None).fit(D["X"], D["y"], R.Engine())


def test_repr_is_scikit_learns():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import RandomForestClassifier
    from phenotypeseeker_amd import model as M
    for kw in (dict(random_state=0), dict(random_state=7, n_estimators=10), dict(random_state=3, bootstrap=False, criterion="entropy",
               max_features="log2", min_samples_leaf=4, n_estimators=10), dict(random_state=4294967295, bootstrap=False, criterion="entropy",
               max_depth=100, max_features=None, min_samples_leaf=2, min_samples_split=10, n_estimators=200)):
        assert repr(M.RandomForest(**kw)) == repr(RandomForestClassifier(**kw)), kw


def test_forest_model_file_loads_under_scikit_learn(tmp_path, fx, searched):
    """A shell-written RF package loads with joblib.load into a real RandomizedSearchCV over a real RandomForestClassifier
    whose predict_proba and feature_importances_ equal ours; the reader that does not import scikit-learn agrees."""
    pytest.importorskip("sklearn")
    import warnings

    import joblib
    from phenotypeseeker_amd import model as M, skpickle
    g, rs = fx.search, searched
    D = fx.designs[g["design"]]
    shell = rs.to_sklearn_shell()
    assert shell is not None, "no template for the installed scikit-learn: run tools/make_sklearn_shells.py"
    path = os.path.join(tmp_path, "rf.pkl")
    with open(path, "wb") as f:
        f.write(skpickle.dumps({"model": shell, "kmers": np.array(["ACGT"] * D["p"], dtype=object), "pca": False, "pred_scale": "binary"}))
    rng = np.random.default_rng(3)
    Xn = np.vstack([D["X"], (rng.random((50, D["p"])) < 0.5).astype(np.float64)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = joblib.load(path)["model"]
        assert type(m).__module__ == "sklearn.model_selection._search" and type(m).__name__ == "RandomizedSearchCV"
        sk = m.best_estimator_
        assert type(sk).__module__ == "sklearn.ensemble._forest" and type(sk).__name__ == "RandomForestClassifier"
        assert all(type(e).__module__ == "sklearn.tree._classes" and type(e.tree_).__module__ == "sklearn.tree._tree" for e in sk.estimators_)
        assert repr(sk) == repr(rs.best_estimator_) and sk.get_params()["random_state"] == g["seed"]
        assert m.get_params()["n_iter"] == g["n_iter"] and m.best_params_ == g["best"]
        sk_pred, sk_proba, sk_imp = m.predict(Xn), m.predict_proba(Xn), sk.feature_importances_
    assert float(np.abs(sk_proba[:D["n"]] - g["proba"]).max()) <= ATOL
    assert np.array_equal(sk_proba, rs.predict_proba(Xn)) and np.array_equal(sk_pred, rs.predict(Xn))
    assert float(np.abs(sk_imp - rs.best_estimator_.feature_importances_).max()) <= ATOL
    assert float(np.abs(sk_imp - g["importances"]).max()) <= ATOL
    real = rs.to_sklearn()                                    # the same objects through the real constructors
    assert np.array_equal(real.predict(Xn), sk_pred) and np.array_equal(real.predict_proba(Xn), sk_proba)
    fast = skpickle.load_linear_package(path)                 # what `phenotypeseeker prediction` reads the file with
    assert fast is not None and isinstance(fast["model"], M.RandomForest)
    assert np.array_equal(fast["model"].predict(Xn), sk_pred) and np.array_equal(fast["model"].predict_proba(Xn), sk_proba)


def test_bc_rf_sits_behind_the_knob(tmp_path, monkeypatch):
    from test_host_modeling import _setup
    monkeypatch.delenv("PSK_RF", raising=False)
    monkeypatch.delenv("PSK_RF_SEED", raising=False)
    for flag in (None, "0"):
        if flag is not None:
            monkeypatch.setenv("PSK_RF", flag)
        with pytest.raises(SystemExit) as e:
            _setup(tmp_path, "ds_bonf", ["-bc", "RF"])
        assert str(e.value) == ("Only the logistic-regression classifier runs on the GPU engine, got 'RF' "
                                "(SVM/RF/DT/NB are outside the accelerated path).")
    monkeypatch.setenv("PSK_RF", "1")
    M, _ = _setup(tmp_path, "ds_bonf", ["-bc", "RF"])
    assert (M.phenotypes.model_name_long, M.phenotypes.model_name_short) == ("random forest", "RF")
    assert M.phenotypes.binary_classifier == "RF" and M.phenotypes.n_iter == 25 and M.phenotypes.rf_seed == 0
    est, grid, none = M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()
    assert repr(est) == "RandomForestClassifier(random_state=0)" and none is None and grid == R.REFERENCE_GRID
    monkeypatch.setenv("PSK_RF_SEED", "41")
    M, _ = _setup(tmp_path, "ds_bonf", ["-bc", "RF", "--n_iter", "4"])
    assert M.phenotypes.n_iter == 4 and M.phenotypes.rf_seed == 41
    assert repr(M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()[0]) == "RandomForestClassifier(random_state=41)"
    for seed in ("-1", "4294967296", "x"):
        monkeypatch.setenv("PSK_RF_SEED", seed)
        with pytest.raises(SystemExit) as e:
            _setup(tmp_path, "ds_bonf", ["-bc", "RF"])
        assert "PSK_RF_SEED" in str(e.value)
    monkeypatch.delenv("PSK_RF_SEED")
    for extra in (["--real_counts"], ["--pca"]):
        with pytest.raises(SystemExit) as e:
            _setup(tmp_path, "ds_bonf", ["-bc", "RF"] + extra)
        assert extra[0] in str(e.value) and "-bc RF" in str(e.value)
    for n_iter in ("0", "107", "20000"):                      # outside the sampler regime that is pinned against scikit-learn
        with pytest.raises(SystemExit) as e:
            _setup(tmp_path, "ds_bonf", ["-bc", "RF", "--n_iter", n_iter])
        assert "--n_iter must be 1..106" in str(e.value)
    for other in ("DT", "NB"):                                # the knob opens RF alone
        with pytest.raises(SystemExit):
            _setup(tmp_path, "ds_bonf", ["-bc", other])
    M, _ = _setup(tmp_path, "ds_bonf", [])                    # the default classifier is untouched by the knob
    assert M.phenotypes.model_name_short == "log_reg" and M.phenotypes.binary_classifier == "log"


def test_abi_names_the_forest_entry_point():
    from phenotypeseeker_amd import _lib
    assert "psk_forest_fit" in _lib.exported_names()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psk.h")) as f:
        header = f.read()
    assert "int psk_forest_fit(psk_ctx *ctx" in header and "---- f7:" in header
    decl = header.split("int psk_forest_fit(")[1].split(");")[0]
    assert decl.count(",") + 1 == len(_lib._SIGNATURES["psk_forest_fit"][1])
