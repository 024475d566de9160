"""CPU tests (-m "not gpu") of `-bc XGBC` / `-reg XGBR` under `--real_counts`: the NumPy restatement of the count contract
(gb_count_restated.py, what psk_gb_fit_counts computes bit for bit) against scikit-learn's record on count designs
(tests/golden/gb_count_kat.npz, tools/gen_gb_count_golden.py) within the recorded bounds; the 0/1 design as a count design; the
routing of a held-out value inside a gap; model.GradientBoosting(counts=True) over a stand-in engine and its model file; the
PSK_GB_COUNTS knob; the ABI."""
import os

import numpy as np
import pytest

import gb_count_restated as C
import gb_restated as R
from helpers import GOLDEN, ROOT

MARGIN, MIN_IMPURITY = 1e-9, 1e-12       # the decisive-input condition of tools/gen_gb_count_golden.py
LOSS_NAME = {0: "squared_error", 1: "log_loss"}


class Fixture:
    """The golden record and, per case, the restatement's fit of it (with the decisive-input diagnostic), computed once."""

    def __init__(self):
        g = np.load(os.path.join(GOLDEN, "gb_count_kat.npz"))
        self.g, self.rate = g, float(g["learning_rate"])
        self.designs = [dict(X=g["X_%d" % d].astype(np.float64), y=g["y_%d" % d], fold=g["fold_%d" % d]) for d in range(6)]
        self.cases = []
        for k in range(len(g["case_design"])):
            c = dict(k=k, design=int(g["case_design"][k]), fit_fold=int(g["case_fit_fold"][k]), loss=int(g["case_loss"][k]),
                     stages=int(g["case_stages"][k]), depth=int(g["case_depth"][k]))
            for name in ("staged", "predict", "proba", "init", "train_score", "d_ref", "bound", "thresholds"):
                c[name] = g["%s_%d" % (name, k)]
            D = self.designs[c["design"]]
            c["in_bag"] = D["fold"] != c["fit_fold"]
            c["init_raw"] = R.init_raw(D["y"], c["in_bag"], c["loss"])
            c["fit"] = C.fit_one(D["X"], D["y"], c["in_bag"], c["loss"], c["stages"], self.rate, c["depth"], c["init_raw"], diagnose=True)
            self.cases.append(c)


_FX = []


def fixture():
    """One Fixture per process: test_gpu_gb_count.py shares it."""
    if not _FX:
        _FX.append(Fixture())
    return _FX[0]


@pytest.fixture(scope="module")
def fx():
    return fixture()


def test_the_fixture_holds_what_the_tests_need(fx):
    g = fx.g
    assert str(g["sklearn_version"]) == "1.7.2" and fx.rate == 0.1
    assert len(fx.cases) == 26 and [c["loss"] for c in fx.cases].count(1) == 13
    assert {(c["stages"], c["depth"]) for c in fx.cases} == {(30, 3), (10, 1), (10, 4)}
    for loss in (0, 1):
        kept, skipped = list(g["seeds_kept_%d" % loss]), list(g["seeds_skipped_%d" % loss])
        assert len(kept) == 3 and max(kept) < 64 and sorted(kept + skipped) == list(range(max(kept) + 1))
    for D in fx.designs:
        X = D["X"]
        assert X.shape == (96, 40) and np.array_equal(X, np.floor(X)) and X.min() == 0 and X.max() > 1
        assert set(np.unique(X[:, 7::8])) == {0.0, 1.0} and set(np.unique(D["fold"])) == {0, 1, 2}
    for c in fx.cases:
        nb = int(c["in_bag"].sum())
        assert c["staged"].shape == (c["stages"], nb) and c["predict"].shape == (nb,) and c["train_score"].shape == (c["stages"],)
        # the bound is made of scikit-learn's own spread and the format's precision, never of the code under test
        assert float(c["bound"]) == 8.0 * max(float(c["d_ref"]), 2.0 ** -52 * float(np.abs(c["staged"]).max()))
        assert float(c["bound"]) < 1e-13
    # scikit-learn split between counts, not only between absence and presence
    assert max(float(c["thresholds"].max()) for c in fx.cases) > 1.0
    assert any(np.any(c["thresholds"] != np.floor(c["thresholds"]) + 0.5) for c in fx.cases)


def test_every_golden_case_is_decisive(fx):
    for c in fx.cases:
        assert c["fit"]["margin"] >= MARGIN and c["fit"]["min_impurity"] >= MIN_IMPURITY, (c["k"], c["fit"]["margin"], c["fit"]["min_impurity"])


def test_restatement_is_within_the_bound_of_scikit_learn(fx):
    from phenotypeseeker_amd.model_gb import expit
    for c in fx.cases:
        f, tr, bound = c["fit"], c["in_bag"], float(c["bound"])
        assert abs(c["init_raw"] - float(c["init"])) <= bound, c["k"]
        err = float(np.abs(f["staged"][:, tr] - c["staged"]).max())
        assert err <= bound, (c["k"], err, bound)
        raw = f["raw"][tr]
        if c["loss"] == 0:
            assert np.all(np.abs(raw - c["predict"]) <= bound), c["k"]
        else:
            assert np.all(np.abs(np.column_stack([1 - expit(raw), expit(raw)]) - c["proba"]) <= bound), c["k"]
            assert np.all(np.abs(raw) > bound) and np.array_equal((raw >= 0).astype(np.int64), c["predict"].astype(np.int64)), c["k"]
        # midpoints between counts, above 0.5 too, as scikit-learn's are.  (Not the same SET: a column and its double give one
        # partition at two thresholds, a tie that scikit-learn's random_state decides and the lowest column decides here.)
        used = np.unique(np.concatenate([f["threshold"][t, :k][f["nodes"][t, :k, 0] >= 0] for t, k in enumerate(f["node_count"])]))
        assert np.array_equal(2.0 * used, np.floor(2.0 * used)) and used.min() == 0.5 and used.max() > 1.0, (c["k"], used)
        assert c["thresholds"].min() == 0.5 and c["thresholds"].max() > 1.0
        assert np.all(f["threshold"][f["nodes"][:, :, 1] <= 0] == -2.0)


@pytest.mark.parametrize("loss", [0, 1])
def test_a_presence_design_is_a_count_design(loss):
    """On a 0/1 design the count restatement is gb_restated's with ==, every split at 0.5."""
    g = np.load(os.path.join(GOLDEN, "gb_kat.npz"))
    d = 3 * loss
    X, y, fold = g["X_%d" % d].astype(np.float64), g["y_%d" % d], g["fold_%d" % d]
    for ff in (-1, 1):
        init = R.init_raw(y, fold != ff, loss)
        want = R.fit_one(X, y, fold != ff, loss, 12, 0.1, 3, init)
        got = C.fit_one(X, y, fold != ff, loss, 12, 0.1, 3, init)
        for key in ("node_count", "nodes", "value", "impurity", "staged", "raw"):
            assert np.array_equal(got[key], want[key]), (loss, ff, key)
        split = got["nodes"][:, :, 1] > 0
        assert split.any() and np.all(got["threshold"][split] == 0.5) and np.all(got["threshold"][~split] == -2.0)
        args = (got["node_count"], got["nodes"], got["value"])
        assert np.array_equal(C.decision(X, *args, got["threshold"], init, 0.1, 3), R.decision(X, *args, init, 0.1, 3))


def gap_design():
    """Column 0 holds {0, 3} among the in-bag samples and a held-out 1; column 1 is noise that never wins."""
    n = 70
    X = np.zeros((n, 2))
    X[::2, 0] = 3.0
    X[5, 0] = 1.0
    X[:, 1] = np.arange(n) % 3 == 0
    y = np.where(X[:, 0] == 3.0, 2.0, -1.0) + 0.01 * (np.arange(n) % 5)
    fold = np.zeros(n, dtype=np.int32)
    fold[5] = 1
    return X, y, fold


def test_a_held_out_value_inside_the_gap_goes_by_the_threshold():
    X, y, fold = gap_design()
    f = C.fit_one(X, y, fold != 1, 0, 3, 0.1, 2, R.init_raw(y, fold != 1, 0))
    assert f["nodes"][0, 0, 0] == 0 and f["threshold"][0, 0] == 1.5          # between the in-bag 0 and 3, not 0.5 or 2.0
    left = f["nodes"][0, 0, 1]
    same_side = f["staged"][0] == f["staged"][0][1]                            # sample 1 holds 0: the left side
    assert left == 1 and same_side[5] and not same_side[0]
    raw = C.decision(X, f["node_count"], f["nodes"], f["value"], f["threshold"], R.init_raw(y, fold != 1, 0), 0.1, 2)
    assert np.array_equal(raw, f["raw"])
    # with the sample in bag the gaps are 0-1 and 1-3: another threshold
    g = C.fit_one(X, y, fold != 7, 0, 1, 0.1, 2, R.init_raw(y, fold != 7, 0))
    assert g["threshold"][0, 0] in (0.5, 2.0)


def _estimator(fx, k):
    from phenotypeseeker_amd import model as M
    c = fx.cases[k]
    D = fx.designs[c["design"]]
    y = D["y"] if c["loss"] == 0 else D["y"].astype(np.int64)
    m = M.GradientBoosting(LOSS_NAME[c["loss"]], n_estimators=c["stages"], max_depth=c["depth"], counts=True).fit(D["X"], y, C.Engine())
    return c, D, y, m


@pytest.mark.parametrize("k", [0, 13])
def test_counts_estimator_over_the_stand_in_engine(tmp_path, fx, k):
    """The all-sample cases: the estimator's arrays are the restatement's; raw on the host is decision; the exported object is a
    real scikit-learn estimator that predicts what the model predicts, and from_sklearn gives the model back."""
    pytest.importorskip("sklearn")
    import joblib
    from phenotypeseeker_amd import model as M, model_gb
    c, D, y, m = _estimator(fx, k)
    assert c["fit_fold"] == -1
    f, X, bound = c["fit"], D["X"], float(c["bound"])
    assert m.counts and m.init_raw_ == c["init_raw"] and repr(m) == repr(M.GradientBoosting(LOSS_NAME[c["loss"]], n_estimators=c["stages"]))
    assert np.array_equal(m.node_count_, f["node_count"]) and np.array_equal(m.nodes_, f["nodes"])
    assert np.array_equal(m.value_, f["value"]) and np.array_equal(m.impurity_, f["impurity"]) and np.array_equal(m.threshold_, f["threshold"])
    want = C.decision(X, f["node_count"], f["nodes"], f["value"], f["threshold"], c["init_raw"], fx.rate, c["depth"])
    assert np.array_equal(m.raw(X), want) and np.array_equal(m.raw(X, C.Engine()), want) and np.array_equal(want, f["raw"])
    assert np.array_equal(m.staged_raw(X), f["staged"])
    assert np.abs(m.train_score_ - c["train_score"]).max() <= 1e-12
    assert m._clone().counts and m.estimators_[0].threshold[0] == f["threshold"][0, 0]
    Xn = np.random.default_rng(k).integers(0, 12, (50, 40)).astype(np.float64)          # values absent from training
    assert np.array_equal(m.raw(Xn), m.raw(Xn, C.Engine()))
    path = os.path.join(tmp_path, "gb.pkl")
    joblib.dump({"model": m.to_sklearn()}, path)
    sk = joblib.load(path)["model"]
    assert type(sk).__module__ == "sklearn.ensemble._gb" and type(sk.estimators_[0, 0]).__name__ == "DecisionTreeRegressor"
    assert sk.estimators_[0, 0].tree_.threshold[0] == f["threshold"][0, 0]
    for Z in (X, Xn):
        raw = sk.decision_function(Z) if c["loss"] else sk.predict(Z)
        assert np.abs(raw - m.raw(Z)).max() <= bound
        if c["loss"]:
            assert np.array_equal(sk.predict(Z), m.predict(Z))
    back = model_gb.from_sklearn(sk)
    assert isinstance(back, M.GradientBoosting) and back.counts
    for name in ("node_count_", "nodes_", "value_", "impurity_", "threshold_"):
        assert np.array_equal(getattr(back, name), getattr(m, name)), name
    assert np.array_equal(back.raw(Xn), m.raw(Xn)) and np.array_equal(back.raw(Xn, C.Engine()), m.raw(Xn))


def test_a_presence_model_stays_on_the_presence_path(fx):
    """from_sklearn of a model whose every threshold is 0.5 is what it was: counts off, no thresholds kept."""
    pytest.importorskip("sklearn")
    from phenotypeseeker_amd import model as M, model_gb
    D = fx.designs[0]
    X = (D["X"] > 0).astype(np.float64)
    m = M.GradientBoosting("squared_error", n_estimators=5).fit(X, D["y"], C.Engine())
    back = model_gb.from_sklearn(m.to_sklearn())
    assert not m.counts and m.threshold_ is None and not back.counts and back.threshold_ is None
    assert np.array_equal(back.raw(X), m.raw(X))


def test_the_engine_layer_checks_the_values_before_the_cast():
    from phenotypeseeker_amd.engine import PskContext
    assert PskContext._count_design(np.array([[0.0, 2.0 ** 24]]), "gb_fit_counts").dtype == np.float32
    for bad in (1.5, -1.0, 2.0 ** 24 + 1, np.nan):
        with pytest.raises(ValueError) as e:
            PskContext._count_design(np.array([[0.0, bad]]), "gb_fit_counts")
        assert "gb_fit_counts takes a count design" in str(e.value)
    assert np.float32(2.0 ** 24 + 1) == np.float32(2.0 ** 24)          # what the cast would have hidden


def test_real_counts_sits_behind_its_own_knob(tmp_path, monkeypatch):
    from test_gb_host import _input_args
    for knob in ("PSK_GB", "PSK_GB_COUNTS", "PSK_NB", "PSK_SVM", "PSK_DT", "PSK_RF", "PSK_PCA", "PSK_ENET", "PSK_TREE_COUNTS"):
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("PSK_GB", "1")
    today = "The gradient boosting %s on the GPU engine takes the 0/1 presence matrix only: --real_counts is not supported with %s."
    cases = ((["-bc", "XGBC"], True, "classifier", "-bc XGBC"), (["-reg", "XGBR"], False, "regressor", "-reg XGBR"))
    for flag in (None, "0"):
        if flag is not None:
            monkeypatch.setenv("PSK_GB_COUNTS", flag)
        for extra, binary, kind, name in cases:
            with pytest.raises(SystemExit) as e:
                _input_args(tmp_path, extra + ["--real_counts"], binary)
            assert str(e.value) == today % (kind, name)
    monkeypatch.setenv("PSK_TREE_COUNTS", "1")                          # the count trees' knob does not open it
    with pytest.raises(SystemExit):
        _input_args(tmp_path, ["-bc", "XGBC", "--real_counts"], True)
    monkeypatch.setenv("PSK_GB_COUNTS", "1")
    for extra, binary, kind, name in cases:
        M = _input_args(tmp_path, extra + ["--real_counts"], binary)
        est, pname, grid = M.Input.phenotypes_to_analyse["MIC"]._new_estimator()
        assert M.phenotypes.gradient_boosting and est.counts and pname is None and grid is None
        assert repr(est) == ("GradientBoostingClassifier()" if binary else "GradientBoostingRegressor()")
        M = _input_args(tmp_path, extra, binary)
        assert not M.Input.phenotypes_to_analyse["MIC"]._new_estimator()[0].counts
        for more in (["--pca"], ["--pca", "--real_counts"]):
            with pytest.raises(SystemExit) as e:
                _input_args(tmp_path, extra + more, binary)
            assert str(e.value) == today.replace("--real_counts", "--pca") % (kind, name)
    monkeypatch.delenv("PSK_GB")                                        # and it opens nothing by itself
    with pytest.raises(SystemExit) as e:
        _input_args(tmp_path, ["-bc", "XGBC", "--real_counts"], True)
    assert "got 'XGBC'" in str(e.value)


def test_abi_names_the_count_entry_points():
    from phenotypeseeker_amd import _lib
    with open(os.path.join(ROOT, "include", "psk.h")) as f:
        header = f.read()
    assert "psk_gb_fit_counts: psk_gb_fit on a COUNT design" in header
    for name in ("psk_gb_fit_counts", "psk_gb_decision_counts"):
        assert name in _lib.exported_names()
        assert "int %s(psk_ctx *ctx" % name in header
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib._SIGNATURES[name][1]), name
    assert hasattr(_lib.load(), "psk_gb_fit_counts") and hasattr(_lib.load(), "psk_gb_decision_counts")
