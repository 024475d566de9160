"""CPU tests (-m "not gpu") of the decision tree's host side: the NumPy restatement of scikit-learn's builder
(tests/tree_restated.py) against scikit-learn's recorded fits (tests/golden/tree_kat.npz, tools/gen_tree_golden.py), the
two-key grid search, the scikit-learn .pkl of a fitted tree and the `-bc DT` option handling.  Where an estimator has to be
fitted without a GPU, the engine call is served by the restatement (tree_restated.Engine): the host code under test is the
package's own.

Tolerance: impurities, node values and importances are f64 functions of integers below 4096 with results bounded by 1; a
handful of roundings (and one logarithm whose library may differ in the last place) put two correct evaluations within a few
1e-16 of each other, so 1e-12 absolute is derived, not measured."""
import os

import numpy as np
import pytest

import tree_restated as R

ATOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


def _all(D):
    return np.ones(D["n"], dtype=bool)


def assert_same_tree(got, want, where):
    """Integers ==, node order included; impurities within ATOL."""
    assert got["node_count"] == want["node_count"] and got["max_depth"] == want["max_depth"], where
    for k in ("feature", "left", "right", "n_node_samples", "counts"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert float(np.abs(got["impurity"] - want["impurity"]).max()) <= ATOL, where


def test_fixture_holds_what_the_tests_need(fx):
    shapes = {(D["n"], D["p"]) for D in fx.designs if D["kind"] == "plain"}
    assert {(256, 40), (256, 200), (1024, 200)} <= shapes
    assert {D["kind"] for D in fx.designs} == {"plain", "duplicated", "complemented"}
    assert int(fx.z["seeds"]) >= 12
    assert len(fx.cases) == len(fx.designs) * 2 * 10
    inv = [c for c in fx.cases if c["invariant"]]
    shallow = {(c["design"], c["criterion"], c["depth"]) for c in inv if c["depth"] <= 3 and fx.designs[c["design"]]["kind"] == "plain"}
    assert len(shallow) >= 18 and {(cr, d) for _, cr, d in shallow} == {(cr, d) for cr in R.CRITERIA for d in (1, 2, 3)}
    assert not any(c["invariant"] for c in fx.cases if fx.designs[c["design"]]["kind"] != "plain")   # copies tie by construction
    assert any(c["tree"]["node_count"] > 100 for c in fx.cases)
    assert fx.designs[fx.gs["design"]]["kind"] == "plain" and len(fx.gs["params"]) == 6
    assert len(set(fx.gs["rank"].tolist())) < len(fx.gs["rank"])     # the record holds tied candidates: min rank is exercised
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_kat.npz")) < 1 << 20


def test_restatement_equals_scikit_learn_where_the_seed_does_not_matter(fx):
    n = 0
    for c in fx.cases:
        if not c["invariant"]:
            continue
        D = fx.designs[c["design"]]
        where = (c["design"], c["criterion"], c["depth"])
        t = R.fit(D["X"], D["y"], _all(D), c["depth"], c["criterion"])
        assert_same_tree(t, c["tree"], where)
        assert float(np.abs(R.values(t) - c["value"]).max()) <= ATOL, where
        assert float(np.abs(R.importances(t, D["p"]) - c["importances"]).max()) <= ATOL, where
        assert float(np.abs(np.column_stack([1.0 - t["frac"], t["frac"]]) - c["proba"]).max()) <= ATOL, where
        assert np.array_equal(R.apply(t, D["X"]), t["leaf"]), where
        n += 1
    assert n >= 18


def node_sets(t, X):
    """{frozen sample set: node} of a tree's split nodes over the rows of X (all of them trained on)."""
    Xb = np.asarray(X) != 0
    out, stack = {}, [(0, np.ones(Xb.shape[0], dtype=bool))]
    while stack:
        k, members = stack.pop()
        if t["feature"][k] >= 0:
            out[members.tobytes()] = k
            stack.append((int(t["right"][k]), members & Xb[:, t["feature"][k]]))
            stack.append((int(t["left"][k]), members & ~Xb[:, t["feature"][k]]))
    return out


def test_certificate_on_the_seed_dependent_cases(fx):
    """Where scikit-learn's tree depends on random_state its recorded tree is one of several correct ones, and so is the
    restatement's.  What both must satisfy: at the root, and at every node whose sample set the two trees share, the chosen
    column's proxy IS the maximum over all columns (bit-equal: both pick among the maxima), the restatement's being the
    lowest such column."""
    checked = shared = differing = 0
    for c in fx.cases:
        if c["invariant"]:
            continue
        D = fx.designs[c["design"]]
        Xb = D["X"] != 0
        t, s = R.fit(D["X"], D["y"], _all(D), c["depth"], c["criterion"]), c["tree"]
        mine, theirs = node_sets(t, D["X"]), node_sets(s, D["X"])
        assert _all(D).tobytes() in mine and _all(D).tobytes() in theirs     # the root splits in both
        assert t["node_count"] % 2 == 1 and np.all((t["left"] == -1) == (t["feature"] == -2))
        differing += not np.array_equal(t["feature"], s["feature"])
        for key, k in theirs.items():
            if key not in mine:
                continue
            members = np.frombuffer(key, dtype=bool)
            pr, _, _, _, _ = R.node_proxies(Xb, D["y"], members, c["criterion"])
            best = pr.max()
            assert pr[s["feature"][k]] == best, ("scikit-learn", c["design"], c["criterion"], c["depth"], k)
            j = t["feature"][mine[key]]
            assert pr[j] == best and j == int(np.argmax(pr)), ("restatement", c["design"], c["criterion"], c["depth"], k)
            shared += 1
        checked += 1
    print("certificate: %d seed-dependent cases (%d with another tree than the record), %d shared split nodes" % (checked, differing, shared))
    assert checked >= 60 and differing >= 20 and shared > 1000


def test_fold_masked_fit_routes_the_held_out_samples(fx):
    D = fx.designs[1]
    tr = D["folds"] != 2
    t = R.fit(D["X"], D["y"], tr, 4, "gini")
    assert t["n_node_samples"][0] == tr.sum() and np.all(t["leaf"] >= 0)
    assert np.array_equal(R.apply(t, D["X"]), t["leaf"])                 # held-out rows walk the same nodes
    only = R.fit(D["X"][tr], D["y"][tr], np.ones(int(tr.sum()), dtype=bool), 4, "gini")
    assert_same_tree(t, only, "masking == sub-setting")
    assert np.array_equal(t["frac"], (t["counts"][:, 1] / t["n_node_samples"])[t["leaf"]])


def test_edges_of_the_builder():
    X = np.array([[0, 0], [0, 1], [1, 0], [1, 1]] * 2, dtype=np.float64)
    y = np.array([0, 1, 1, 0] * 2)
    t = R.fit(X, y, np.ones(8, dtype=bool), 2, "gini")      # XOR: every first split improves nothing and is taken all the same
    assert list(t["feature"]) == [0, 1, -2, -2, 1, -2, -2] and np.all(t["impurity"][[2, 3, 5, 6]] == 0.0)
    one = R.fit(X, np.zeros(8, dtype=int), np.ones(8, dtype=bool), 3, "entropy")
    assert one["node_count"] == 1 and one["feature"][0] == -2 and np.all(one["frac"] == 0.0)
    const = R.fit(np.ones((6, 3)), np.array([0, 1, 0, 1, 0, 1]), np.ones(6, dtype=bool), 3, "gini")
    assert const["node_count"] == 1 and const["impurity"][0] == 0.5     # no non-constant column: a leaf that is not pure


def test_grid_search_over_two_keys_equals_the_record(fx):
    """ParameterGrid order (keys sorted, the last fastest: criterion outer, max_depth inner), split scores, means, stds, min
    ranks with ties and best_params_ equal GridSearchCV's recorded cv_results_; the fold fits come from the restatement."""
    from phenotypeseeker_amd import model as M
    g = fx.gs
    D = fx.designs[g["design"]]
    gs = M.GridSearch(M.DecisionTree(), {"max_depth": g["depths"], "criterion": ["gini", "entropy"]}, cv=g["cv"])
    gs.fit(D["X"], D["y"], R.Engine())
    r = gs.cv_results_
    assert r["params"] == g["params"] and [list(q) for q in r["params"]] == [["criterion", "max_depth"]] * 6
    for f in range(g["cv"]):
        assert np.array_equal(r["split%d_test_score" % f], g["splits"][:, f]), f
    assert np.array_equal(r["mean_test_score"], g["mean"]) and np.allclose(r["std_test_score"], g["std"], rtol=0, atol=1e-15)
    assert np.array_equal(r["rank_test_score"], g["rank"])
    assert gs.best_params_ == g["best"] and gs.best_index_ == int(np.argmin(g["rank"]))
    be = gs.best_estimator_
    assert isinstance(be, M.DecisionTree) and (be.criterion, be.max_depth) == (g["best"]["criterion"], g["best"]["max_depth"])
    assert repr(gs.estimator) == "DecisionTreeClassifier()"
    want = (["criterion='entropy'"] if be.criterion == "entropy" else []) + ["max_depth=%d" % be.max_depth]
    assert repr(be) == "DecisionTreeClassifier(%s)" % ", ".join(want)
    # the single-parameter constructor is untouched
    one = M.GridSearch(M.L1LogisticRegression(), "C", [0.1, 1.0], 3)
    assert one.param_name == "C" and one.param_grid == {"C": [0.1, 1.0]} and one.candidates() == [{"C": 0.1}, {"C": 1.0}]


def test_estimator_protocol_and_importances(fx):
    from phenotypeseeker_amd import model as M
    c = [c for c in fx.cases if c["invariant"] and c["depth"] == 3 and c["criterion"] == "entropy"][0]
    D = fx.designs[c["design"]]
    m = M.DecisionTree(criterion="entropy", max_depth=3).fit(D["X"], D["y"], R.Engine())
    t = m.tree_
    assert np.array_equal(t.feature, c["tree"]["feature"]) and np.array_equal(t.children_left, c["tree"]["left"])
    assert np.array_equal(t.children_right, c["tree"]["right"]) and np.array_equal(t.n_node_samples, c["tree"]["n_node_samples"])
    assert t.node_count == c["tree"]["node_count"] and t.max_depth == c["tree"]["max_depth"] and t.value.shape == (t.node_count, 1, 2)
    assert np.array_equal(t.threshold, np.where(t.feature >= 0, 0.5, -2.0))
    assert float(np.abs(t.value - c["value"]).max()) <= ATOL and float(np.abs(t.impurity - c["tree"]["impurity"]).max()) <= ATOL
    assert float(np.abs(m.feature_importances_ - c["importances"]).max()) <= ATOL
    assert float(np.abs(m.predict_proba(D["X"]) - c["proba"]).max()) <= ATOL
    assert np.array_equal(m.predict(D["X"]), np.argmax(c["proba"], axis=1))
    assert m.score(D["X"], D["y"]) == np.mean(np.argmax(c["proba"], axis=1) == D["y"])
    tie = M.DecisionTree(max_depth=1).fit(np.array([[0.0], [0.0], [1.0], [1.0]]), np.array([0, 1, 0, 1]), R.Engine())
    assert list(tie.predict(np.array([[0.0], [1.0]]))) == [0, 0]         # equal fractions: class 0, as np.argmax
    with pytest.raises(ValueError):
        M.DecisionTree().fit(D["X"], D["y"], R.Engine())                  # max_depth=None is not offered by the engine
    with pytest.raises(ValueError):
        M.DecisionTree(criterion="log_loss")


def test_tree_model_file_loads_under_scikit_learn(tmp_path, fx):
    """A shell-written DT package loads with joblib.load into a real GridSearchCV over a real DecisionTreeClassifier whose
    predict / predict_proba equal the recorded ones; the reader that does not import scikit-learn agrees."""
    pytest.importorskip("sklearn")
    import warnings

    import joblib
    from phenotypeseeker_amd import model as M, skpickle
    c = [c for c in fx.cases if c["invariant"] and c["depth"] == 3 and c["criterion"] == "gini" and c["design"] == fx.gs["design"]][0]
    D = fx.designs[c["design"]]
    gs = M.GridSearch(M.DecisionTree(), {"max_depth": [3], "criterion": ["gini"]}, cv=3).fit(D["X"], D["y"], R.Engine())
    shell = gs.to_sklearn_shell()
    assert shell is not None, "no template for the installed scikit-learn: run tools/make_sklearn_shells.py"
    path = os.path.join(tmp_path, "dt.pkl")
    with open(path, "wb") as f:
        f.write(skpickle.dumps({"model": shell, "kmers": np.array(["ACGT"] * D["p"], dtype=object), "pca": False, "pred_scale": "binary"}))
    rng = np.random.default_rng(3)
    Xn = np.vstack([D["X"], (rng.random((50, D["p"])) < 0.5).astype(np.float64)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pkg = joblib.load(path)
        m = pkg["model"]
        assert type(m).__module__ == "sklearn.model_selection._search"
        sk = m.best_estimator_
        assert type(sk).__module__ == "sklearn.tree._classes" and type(sk).__name__ == "DecisionTreeClassifier"
        assert type(sk.tree_).__module__ == "sklearn.tree._tree"
        assert repr(sk) == "DecisionTreeClassifier(max_depth=3)" and sk.get_params()["criterion"] == "gini"
        assert "param_grid={'criterion': ['gini'], 'max_depth': [3]}" in repr(m).replace("\n", " ").replace("  ", "")
        sk_pred, sk_proba, sk_imp = m.predict(Xn), m.predict_proba(Xn), sk.feature_importances_
        assert sk.tree_.node_count == c["tree"]["node_count"] and np.array_equal(sk.tree_.feature, c["tree"]["feature"])
    assert np.array_equal(sk_proba[:D["n"]], c["proba"]) or float(np.abs(sk_proba[:D["n"]] - c["proba"]).max()) <= ATOL
    assert np.array_equal(sk_pred[:D["n"]], np.argmax(c["proba"], axis=1))
    assert np.array_equal(sk_pred, gs.predict(Xn)) and np.array_equal(sk_proba, gs.predict_proba(Xn))
    assert float(np.abs(sk_imp - c["importances"]).max()) <= ATOL
    real = gs.to_sklearn()                                    # the same objects through the real constructors
    assert np.array_equal(real.predict(Xn), sk_pred) and np.array_equal(real.predict_proba(Xn), sk_proba)
    fast = skpickle.load_linear_package(path)                 # what `phenotypeseeker prediction` reads the file with
    assert fast is not None and isinstance(fast["model"], M.DecisionTree)
    assert np.array_equal(fast["model"].predict(Xn), sk_pred) and np.array_equal(fast["model"].predict_proba(Xn), sk_proba)


def test_bc_dt_sits_behind_the_knob(tmp_path, monkeypatch):
    from test_host_modeling import _setup
    monkeypatch.delenv("PSK_DT", raising=False)
    for flag in (None, "0"):
        if flag is not None:
            monkeypatch.setenv("PSK_DT", flag)
        with pytest.raises(SystemExit) as e:
            _setup(tmp_path, "ds_bonf", ["-bc", "DT"])
        assert str(e.value) == ("Only the logistic-regression classifier runs on the GPU engine, got 'DT' "
                                "(SVM/RF/DT/NB are outside the accelerated path).")
    monkeypatch.setenv("PSK_DT", "1")
    M, _ = _setup(tmp_path, "ds_bonf", ["-bc", "DT"])
    assert (M.phenotypes.model_name_long, M.phenotypes.model_name_short) == ("decision tree", "DT")
    assert M.phenotypes.binary_classifier == "DT"
    est, grid, none = M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()
    assert repr(est) == "DecisionTreeClassifier()" and none is None
    assert grid == {"max_depth": [1, 2, 3, 4, 5, 6, 7, 8, 9, 10], "criterion": ["gini", "entropy"]}
    for extra in (["--real_counts"], ["--pca"]):
        with pytest.raises(SystemExit) as e:
            _setup(tmp_path, "ds_bonf", ["-bc", "DT"] + extra)
        assert extra[0] in str(e.value) and "-bc DT" in str(e.value)
    for other in ("RF", "NB"):                                # the knob opens DT alone
        with pytest.raises(SystemExit):
            _setup(tmp_path, "ds_bonf", ["-bc", other])
    M, _ = _setup(tmp_path, "ds_bonf", [])                    # the default classifier is untouched by the knob
    assert M.phenotypes.model_name_short == "log_reg" and M.phenotypes.binary_classifier == "log"
    assert len(M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()) == 3


def test_abi_names_the_tree_entry_point():
    from phenotypeseeker_amd import _lib
    assert "psk_tree_fit" in _lib.exported_names()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psk.h")) as f:
        header = f.read()
    assert "int psk_tree_fit(psk_ctx *ctx" in header and "#define PSK_TREE_NODE_CAP 2047" in header
    decl = header.split("int psk_tree_fit(")[1].split(");")[0]
    assert decl.count(",") + 1 == len(_lib._SIGNATURES["psk_tree_fit"][1])
    from phenotypeseeker_amd.engine import PskContext
    assert PskContext.TREE_NODE_CAP == 2047
