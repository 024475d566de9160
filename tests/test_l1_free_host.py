"""CPU tests of the free-intercept L1 logistic path (`--penalty L1 --logreg_solver saga` behind PSK_L1_SAGA): the yardstick of
tests/test_gpu_l1_free.py certified here -- l1_free_restated.free_arbiter on every fit the device tests use, against
scikit-learn where it is installed, and against liblinear's optimum --, the option of `modeling`, and
model.L1LogisticRegression(solver='saga') (repr, scikit-learn twin, model file, column copies)."""
import os
import pickle

import numpy as np
import pytest

import l1_float_cases as L
import l1_free_restated as F

np.seterr(over="ignore")

BITS = [(n, p) for n in (40, 130, 700) for p in (250, 40)]


def _certificate(X, y, fold, fp, ff, arbs):
    assert not F.one_class_fits(y, fold, ff)
    worst = 0.0
    for C, h, a in zip(fp, ff, arbs):
        assert a["kkt"] < F.KKT_MAX, (C, h, a["kkt"])
        worst = max(worst, a["kkt"])
        tr = fold != h
        g = F.const_group(X[tr].astype(np.float64), a)
        assert g is None or a["w_groups"][g] == 0.0, (C, h)          # the intercept's twin stays at exactly 0
        w = L.expand(a, X.shape[1])
        assert a["objective"] == pytest.approx(F.free_objective(X[tr], y[tr], w, a["b"], float(C)), rel=1e-13)
    return worst


@pytest.mark.parametrize("name", F.FLOAT_CASES + (F.SEAM_CASE,))
def test_the_arbiter_certifies_every_fit_of_the_cases(name):
    """Every fit the device tests judge: KKT residual below 1e-10 within 400 rounds from the zero hint, two classes in every
    training fold, the constant column's pattern at exactly 0.  (Three fits of A-tail-7x3 run at another C: C_CHANGED.)"""
    X, y, fold, fp, ff = F.case_data(name)
    assert X.shape[1] <= 9 or np.all(X[:, L.CONST_COL] == 1)
    worst = _certificate(X, y, fold, fp, ff, F.certified(name))
    print("%s: %d fits, largest KKT residual %.3g" % (name, len(fp), worst))


@pytest.mark.parametrize("n,p", BITS, ids=["%dx%d" % b for b in BITS])
def test_the_arbiter_certifies_the_bit_packed_designs(n, p):
    X, y, fold, fp, ff = F.bits_design(n, p)
    worst = _certificate(X, y, fold, fp, ff, F.bits_certified(n, p))
    print("%dx%d: largest KKT residual %.3g" % (n, p, worst))


def test_c_changed_names_fits_of_the_cases():
    for name, m in F.C_CHANGED.items():
        fp0, ff = L.case_data(name)[3:]
        fp = F.case_data(name)[3]
        have = {(float(C), int(h)) for C, h in zip(fp0, ff)}
        assert set(m) <= have
        assert sum(a != b for a, b in zip(fp0, fp)) == len(m)


@pytest.mark.parametrize("n,p", [(40, 40), (130, 40)], ids=["40x40", "130x40"])
def test_the_arbiter_is_not_above_scikit_learn(n, p):
    """One-sided: the arbiter's objective <= (1 + 1e-12) x that of LogisticRegression(penalty='l1', solver='saga', tol=1e-10,
    max_iter=300000, random_state=0), and of solver='liblinear', intercept_scaling=1e7, tol=1e-12 (a penalty of |b| / 1e7: the
    free intercept to seven digits).  Measured with scikit-learn 1.7.2, objective / the arbiter's - 1 per fit: where the
    optimum has non-zero coefficients (C = 1: 5 of 40 patterns at 40 rows, 16 and 17 at 130) saga ends after 353 .. 780 epochs
    on the arbiter's objective to the last bit (0, 0, 0, 0, -2.2e-16) and liblinear 3.9e-11 .. 2.1e-10 above it; where the
    optimum is w = 0 (C = 0.01 and 0.1) saga stops after 1 .. 9 epochs with the intercept where it then is, 6.7e-8 .. 1.3 %
    above, and liblinear 6.7e-16 .. 1.7e-11 above."""
    lm = pytest.importorskip("sklearn.linear_model")
    import warnings
    X, y, fold, fp, ff = F.bits_design(n, p)
    arbs = F.bits_certified(n, p)
    worst = {"saga": -1.0, "liblinear": -1.0}
    for C, h, a in zip(fp, ff, arbs):
        tr = fold != h
        Xt, yt = X[tr].astype(np.float64), y[tr]
        for solver, extra in (("saga", dict(tol=1e-10, max_iter=300000, random_state=0)), ("liblinear", dict(intercept_scaling=1e7, tol=1e-12))):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sk = lm.LogisticRegression(penalty="l1", solver=solver, C=float(C), **extra).fit(Xt, yt)
            obj = F.free_objective(Xt, yt, sk.coef_[0], float(sk.intercept_[0]), float(C))
            assert a["objective"] <= (1 + 1e-12) * obj, (solver, C, h, a["objective"] / obj - 1)
            worst[solver] = max(worst[solver], obj / a["objective"] - 1)
    print("%dx%d: scikit-learn's objective / the arbiter's - 1, the largest: saga %.3g, liblinear (intercept_scaling 1e7) %.3g"
          % (n, p, worst["saga"], worst["liblinear"]))


@pytest.mark.parametrize("name", ["A-tail-64x1", "A-tail-65x3", "A"])
def test_the_free_optimum_lies_strictly_below_liblinears_in_the_free_objective(name):
    """Another model, not another route: liblinear's certified optimum (l1_float_cases.certified), evaluated in the free
    objective (its own minus |b|), lies strictly above the free arbiter's on every fit."""
    assert name not in F.C_CHANGED
    fp, ff = F.case_data(name)[3:]
    gaps = []
    for C, h, free, pen in zip(fp, ff, F.certified(name), L.certified(name)):
        assert pen["kkt"] < L.KKT_MAX
        in_free = pen["objective"] - abs(pen["b"])
        assert free["objective"] < in_free, (C, h)
        gaps.append(in_free / free["objective"] - 1)
    print("%s: liblinear's optimum above the free one by %.3g .. %.3g (relative, in the free objective); intercepts differ by up "
          "to %.3g" % (name, min(gaps), max(gaps), max(abs(a["b"] - b["b"]) for a, b in zip(F.certified(name), L.certified(name)))))


# ---- `modeling --penalty L1 --logreg_solver saga` ------------------------------------------------------------------------------
OFF = "Logistic Regression with L1 penalty on the GPU engine implements the liblinear objective only, got saga."


def _input_args(tmp_path, extra):
    from test_enet_host import _input_args as enet_input_args
    return enet_input_args(tmp_path, extra, binary=True)


def test_the_solver_sits_behind_the_knob(tmp_path, monkeypatch):
    for knob in ("PSK_L1_SAGA", "PSK_PCA"):
        monkeypatch.delenv(knob, raising=False)
    for flag in (None, "0"):
        if flag is not None:
            monkeypatch.setenv("PSK_L1_SAGA", flag)
        for spelling in (["-ls", "saga"], ["--logreg_solver", "saga", "--penalty", "l1"]):
            with pytest.raises(SystemExit) as e:
                _input_args(tmp_path, spelling)
            assert str(e.value) == OFF
    monkeypatch.setenv("PSK_L1_SAGA", "1")
    M = _input_args(tmp_path, ["-ls", "saga"])
    assert M.phenotypes.pred_scale == "binary" and (M.phenotypes.penalty, M.phenotypes.logreg_solver) == ("L1", "saga")
    assert (M.phenotypes.model_name_long, M.phenotypes.model_name_short) == ("logistic regression", "log_reg")     # files named as liblinear's
    est, pname, grid = M.Input.phenotypes_to_analyse["MIC"]._new_estimator()
    assert repr(est) == "LogisticRegression(max_iter=1000, penalty='l1', solver='saga')" and pname == "C"
    assert np.allclose(grid, 1.0 / np.logspace(-3, 3, 13))
    M = _input_args(tmp_path, ["-ls", "saga", "--real_counts"])
    assert M.phenotypes.real_counts and M.phenotypes.logreg_solver == "saga"
    with pytest.raises(SystemExit) as e:                                  # --pca as for liblinear: it needs its own knob
        _input_args(tmp_path, ["-ls", "saga", "--pca"])
    assert str(e.value) == "--pca is outside the accelerated path."
    monkeypatch.setenv("PSK_PCA", "1")
    M = _input_args(tmp_path, ["-ls", "saga", "--pca"])
    assert M.phenotypes.pca and M.phenotypes.logreg_solver == "saga"
    # the knob changes nothing else: the default and the explicit liblinear, other names still refused in today's words
    for extra in ([], ["-ls", "liblinear"]):
        M = _input_args(tmp_path, extra)
        assert M.phenotypes.logreg_solver == "liblinear"
        assert repr(M.Input.phenotypes_to_analyse["MIC"]._new_estimator()[0]) == "LogisticRegression(max_iter=1000, penalty='l1', solver='liblinear')"
    with pytest.raises(SystemExit) as e:
        _input_args(tmp_path, ["-ls", "lbfgs"])
    assert str(e.value) == OFF.replace("saga", "lbfgs")
    M = _input_args(tmp_path, ["-ls", "saga", "--penalty", "L2"])
    assert repr(M.Input.phenotypes_to_analyse["MIC"]._new_estimator()[0]) == "LogisticRegression(max_iter=1000, solver='saga')"


# ---- model.L1LogisticRegression(solver=...) ---------------------------------------------------------------------------------------
PARAM_SETS = [dict(solver="saga", max_iter=1000), dict(solver="saga"), dict(solver="saga", C=0.5, tol=1e-6, max_iter=50),
              dict(solver="liblinear", max_iter=1000), dict(max_iter=1000)]


@pytest.mark.parametrize("params", PARAM_SETS, ids=[str(i) for i in range(len(PARAM_SETS))])
def test_repr_is_scikit_learns(params):
    lm = pytest.importorskip("sklearn.linear_model")
    from phenotypeseeker_amd.model import L1LogisticRegression
    sk = dict(params)
    sk.setdefault("solver", "liblinear")
    sk.setdefault("max_iter", 1000)                      # (this class's own default, scikit-learn's is 100)
    assert repr(L1LogisticRegression(**params)) == repr(lm.LogisticRegression(penalty="l1", **sk))


def test_repr_without_scikit_learn_and_a_solver_that_is_neither():
    from phenotypeseeker_amd.model import L1LogisticRegression
    assert repr(L1LogisticRegression(max_iter=1000, solver="saga")) == "LogisticRegression(max_iter=1000, penalty='l1', solver='saga')"
    assert repr(L1LogisticRegression(max_iter=1000)) == "LogisticRegression(max_iter=1000, penalty='l1', solver='liblinear')"
    with pytest.raises(ValueError):
        L1LogisticRegression(solver="lbfgs")


class _Engine:
    """Stands in for PskContext in CPU tests: the two L1 entry points by their arbiters; `calls` keeps (entry point, shape)."""

    def __init__(self):
        self.calls = []

    def _fits(self, which, X, y, fold, fp, ff):
        from oracle import oracle_model as OM
        X, y, fold = np.asarray(X, dtype=np.float64), np.asarray(y), np.asarray(fold)
        self.calls.append((which, X.shape))
        out = []
        for C, h in zip(fp, ff):
            tr = fold != h
            a = (F.free_arbiter(X[tr], y[tr], float(C)) if which == "free"
                 else OM.logreg_l1_arbiter(X[tr], y[tr], float(C), np.zeros(X.shape[1]), 0.0, max_rounds=F.ARBITER_ROUNDS))
            out.append((L.expand(a, X.shape[1]), a["b"]))
        return np.stack([w for w, _ in out]), np.array([b for _, b in out]), np.ones(len(out), dtype=np.int32)

    def logreg_l1_fit(self, X, y, fold, fp, ff, tol=1e-4, max_iter=1000):
        return self._fits("penalised", X, y, fold, fp, ff)

    def logreg_l1_free_fit(self, X, y, fold, fp, ff, tol=1e-4, max_iter=1000):
        return self._fits("free", X, y, fold, fp, ff)


def _searched(solver):
    from phenotypeseeker_amd.model import GridSearch, L1LogisticRegression
    X, y = F.bits_design(130, 40)[:2]
    X = np.hstack([X, X[:, :5]]).astype(np.float64)                     # five column copies
    eng = _Engine()
    kw = {} if solver is None else {"solver": solver}
    gs = GridSearch(L1LogisticRegression(tol=1e-4, max_iter=1000, **kw), "C", [0.1, 1.0], 3).fit(X, y, eng)
    return gs, eng, X, y


def test_saga_fits_through_the_free_entry_point_and_copies_are_solved_once():
    gs, eng, X, y = _searched("saga")
    assert eng.calls == [("free", (130, 40))] and gs.n_unique_columns_ == 40
    be = gs.best_estimator_
    assert be.solver == "saga" and be.coef_.shape == (1, 45) and np.all(be.coef_[0, 40:] == 0)
    want = "LogisticRegression(%smax_iter=1000, penalty='l1', solver='saga')" % ("" if be.C == 1.0 else "C=%r, " % be.C)
    assert repr(be) == want
    gl, engl, _, _ = _searched(None)
    assert engl.calls == [("penalised", (130, 40))] and gl.best_estimator_.solver == "liblinear"
    assert gl.best_estimator_.intercept_[0] != be.intercept_[0]


class _ParentL1:
    """The twin the class wrote before it had a solver parameter: the parameters in this order, the solver fixed."""

    @staticmethod
    def twin(est, fitted=True):
        from phenotypeseeker_amd.model_search import _Twin
        params = dict(penalty="l1", solver="liblinear", tol=est.tol, max_iter=int(est.max_iter))
        if not fitted:
            return _Twin("LogisticRegression", "sklearn.linear_model", params)
        return _Twin("LogisticRegression", "sklearn.linear_model", dict(params, C=est.C),
                     dict(classes_=np.array([0, 1]), coef_=est.coef_.copy(), intercept_=est.intercept_.copy(),
                          n_iter_=np.array([0], dtype=np.int32), n_features_in_=est.n_features_in_))


def _package(gs):
    from phenotypeseeker_amd import skpickle
    shell = gs.to_sklearn_shell()
    assert shell is not None, "no template for the installed scikit-learn: run tools/make_sklearn_shells.py"
    return skpickle.dumps({"model": shell, "kmers": np.array(["ACGT"] * 45, dtype=object), "pca": False, "pred_scale": "binary"})


def test_the_model_file_round_trip(tmp_path, monkeypatch):
    """solver='saga': the stub reader takes the file as a plain linear package, joblib.load gives scikit-learn's
    LogisticRegression(penalty='l1', solver='saga') with the model's predict_proba.  Default solver: the bytes are those of the
    class as it was before the solver parameter, from the same coefficients."""
    pytest.importorskip("sklearn")
    from phenotypeseeker_amd import skpickle
    from phenotypeseeker_amd.model import L1LogisticRegression
    gs, _, X, y = _searched("saga")
    path = os.path.join(tmp_path, "log_reg_model_Pheno.pkl")
    with open(path, "wb") as f:
        f.write(_package(gs))
    own = skpickle.load_linear_package(path)
    assert own is not None and type(own["model"]).__name__ == "LinearModel" and own["pred_scale"] == "binary"
    assert np.array_equal(own["model"].predict(X), gs.predict(X))
    assert np.allclose(own["model"].predict_proba(X), gs.predict_proba(X), rtol=1e-14)
    with open(path, "rb") as f:
        pkg = pickle.load(f)
    import joblib
    jl = joblib.load(path)["model"]
    for sk in (pkg["model"], jl):
        be = sk.best_estimator_
        assert type(sk).__name__ == "GridSearchCV" and type(be).__module__.startswith("sklearn.linear_model")
        assert type(be).__name__ == "LogisticRegression" and (be.penalty, be.solver) == ("l1", "saga") and sk.estimator.solver == "saga"
        assert repr(be) == repr(gs.best_estimator_)
        assert np.array_equal(sk.predict(X), gs.predict(X))
        assert np.allclose(sk.predict_proba(X), gs.predict_proba(X), rtol=1e-12)
    # the default solver writes what it wrote
    gl, _, _, _ = _searched(None)
    now = _package(gl)
    monkeypatch.setattr(L1LogisticRegression, "_sklearn", lambda self, fitted=True: _ParentL1.twin(self, fitted))
    assert _package(gl) == now
    assert b"saga" not in now
