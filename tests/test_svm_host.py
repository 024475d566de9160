"""CPU tests (-m "not gpu") of the support vector machine's host side: the NumPy restatement of libsvm's solver against
scikit-learn's recorded fits (tests/golden/svm_kat.npz), the Platt sigmoid, the scikit-learn .pkl of a fitted SVC and the
`-bc SVM` option handling.  Where an estimator has to be fitted without a GPU, the engine call is served by the
restatement (RestatedEngine below): the host code under test is the package's own."""
import os

import numpy as np
import pytest

import svm_restated as R

PATH_RTOL = 1e-6   # the project's coefficient tolerance


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


class RestatedEngine:
    """Stands in for PskContext.svc_fit in CPU tests: the same arguments and results, computed by svm_restated.fit."""

    def svc_fit(self, X, y01, fold, fit_C, fit_fold, kernel="linear", fit_gamma=None, tol=1e-3, max_iter=-1):
        X, y01, fold = np.asarray(X, dtype=np.float64), np.asarray(y01), np.asarray(fold)
        nf = len(fit_C)
        gam = np.broadcast_to(np.asarray(0.0 if fit_gamma is None else fit_gamma, dtype=np.float64), (nf,))
        dual, rho, dec, iters = np.zeros((nf, len(y01))), np.zeros(nf), np.zeros((nf, len(y01))), np.zeros(nf, dtype=np.int32)
        for j in range(nf):
            dual[j], rho[j], dec[j], iters[j] = R.fit(X, y01, fold != fit_fold[j], float(fit_C[j]), kernel, float(gam[j]), tol, max_iter)
        return dual, rho, dec, iters


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) <= PATH_RTOL * max(1.0, float(np.abs(want).max()))


def test_fixture_holds_what_the_tiers_need(fx):
    shapes = [(D["n"], D["p"]) for D in fx.designs]
    assert any(p > n for n, p in shapes) and any(p < n for n, p in shapes)
    assert {f["kernel"] for f in fx.fits} == {"linear", "rbf"}
    assert any(f["fold"] >= 0 for f in fx.fits) and any(f["fold"] < 0 for f in fx.fits)
    assert any(f["kernel"] == "linear" and f["off"]["iters"] >= fx.max_iter for f in fx.fits)
    inadmissible = sum(not f["admissible"] for f in fx.fits)
    assert inadmissible <= 0.02 * len(fx.fits)
    gs = [d for d in range(len(fx.designs)) if "gs%d_equal" % d in fx.z]
    assert any(bool(fx.z["gs%d_equal" % d]) and len(set(fx.z["gs%d_mean_off" % d].tolist())) >= 2 for d in gs)
    assert any(not bool(fx.z["gs%d_equal" % d]) for d in gs)
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svm_kat.npz")) < 1 << 20


def test_restatement_walks_scikit_learns_path(fx):
    """n_iter_ equal and duals / rho / decision values within 1e-6 relative of SVC(shrinking=False) on every admissible fit,
    fits stopped at max_iter and fold-masked fits included."""
    checked = capped = 0
    for f in fx.fits:
        if not f["admissible"]:
            continue
        D = fx.designs[f["design"]]
        dual, rho, dec, it = R.fit(D["X"], D["y"], fx.train_mask(f), f["C"], f["kernel"], f["gamma"], fx.tol, fx.max_iter)
        off = f["off"]
        assert it == off["iters"], (f["design"], f["kernel"], f["C"], f["fold"], it, off["iters"])
        assert _close(dual, off["dual"]) and _close(rho, off["rho"]) and _close(dec, off["dec"])
        checked += 1
        capped += it >= fx.max_iter
    assert checked >= 0.98 * len(fx.fits) and capped > 10


def test_platt_pair_is_a_stationary_point(fx):
    """At the returned (A, B) the gradient of libsvm's regularised likelihood is below libsvm's own stopping bound."""
    from phenotypeseeker_amd import model as M
    n = 0
    for f in fx.fits[::7]:
        y = fx.designs[f["design"]]["y"]
        A, B = M.platt_sigmoid_train(f["off"]["dec"], y == 0)
        g1, g2 = R.platt_objective_gradient(f["off"]["dec"], y == 0, A, B)
        assert abs(g1) < 1e-5 and abs(g2) < 1e-5, (f["design"], f["kernel"], f["C"], g1, g2)
        assert A < 0     # a larger decision value speaks for the positive class
        n += 1
    assert n > 20


def test_platt_constant_values_for_a_one_class_part():
    """A sub-fit of the probability split whose training part has one class contributes libsvm's constant decision values."""
    from phenotypeseeker_amd import model as M
    X = np.array([[1, 0], [1, 1], [0, 1], [0, 0], [1, 0], [0, 1]], dtype=np.float64)
    y = np.array([0, 1, 1, 1, 1, 1])   # the only member of class 0 is held out by one fold
    m = M.SVC(C=1.0, kernel="linear", probability=True, tol=1e-4).fit(X, y, RestatedEngine())
    assert len(m.probA_) == 1 and np.isfinite(m.probA_[0]) and np.isfinite(m.probB_[0])
    p = m.predict_proba(X)
    assert np.allclose(p.sum(axis=1), 1.0)


def _fitted_search(fx, kernel="linear"):
    from phenotypeseeker_amd import model as M
    D = fx.designs[2]
    est = M.SVC(kernel=kernel, gamma=0.02, probability=True, tol=fx.tol, max_iter=1000.0)
    return M.GridSearch(est, "C", [0.01, 1.0, 100.0], 3).fit(D["X"], D["y"], RestatedEngine()), D


def test_grid_search_over_svc_scores_folds_from_decision_values(fx):
    from phenotypeseeker_amd import cv, model as M
    gs, D = _fitted_search(fx)
    folds = cv.stratified_kfold(D["y"], 3)
    for gi, C in enumerate([0.01, 1.0, 100.0]):
        for f in range(3):
            _, _, dec, _ = R.fit(D["X"], D["y"], folds != f, C, "linear", 0.0, fx.tol, 1000)
            want = np.mean((dec[folds == f] <= 0).astype(int) == D["y"][folds == f])
            assert gs.cv_results_["split%d_test_score" % f][gi] == want
    be = gs.best_estimator_
    assert isinstance(be, M.SVC) and be.C == gs.best_params_["C"] and be.coef_.shape == (1, D["p"])
    assert list(be.n_support_) == [int(np.sum(D["y"][be.support_] == 0)), int(np.sum(D["y"][be.support_] == 1))]
    assert np.all(np.diff(D["y"][be.support_]) >= 0)                      # class 0's support vectors first
    assert np.allclose(be.decision_function(D["X"]), D["X"] @ be.coef_[0] + be.intercept_[0], rtol=1e-10, atol=1e-10)
    assert repr(gs.estimator) == "SVC(gamma=0.02, kernel='linear', max_iter=1000.0, probability=True, tol=0.0001)"
    assert repr(M.SVC(kernel="linear", probability=True, max_iter=1000.0, tol=1e-4)) == \
        "SVC(kernel='linear', max_iter=1000.0, probability=True, tol=0.0001)"


@pytest.mark.parametrize("kernel", ["linear", "rbf"])
def test_svc_model_file_loads_under_scikit_learn(tmp_path, fx, kernel):
    """A shell-written SVC package loads with joblib.load under the installed scikit-learn; its predict and
    decision_function equal the package's own and predict_proba agrees within 1e-9: both sides run libsvm's
    multiclass_probability iteration in f64, which leaves rounding; the pairwise value alone would be 6.9e-7 off."""
    pytest.importorskip("sklearn")
    import joblib
    from phenotypeseeker_amd import skpickle
    gs, D = _fitted_search(fx, kernel)
    shell = gs.to_sklearn_shell()
    assert shell is not None, "no template for the installed scikit-learn: run tools/make_sklearn_shells.py"
    path = os.path.join(tmp_path, "svm.pkl")
    with open(path, "wb") as f:
        f.write(skpickle.dumps({"model": shell, "kmers": np.array(["ACGT"] * D["p"], dtype=object), "pca": False, "pred_scale": "binary"}))
    rng = np.random.default_rng(3)
    X = np.vstack([D["X"], (rng.random((50, D["p"])) < 0.5).astype(np.float64)])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pkg = joblib.load(path)
        m = pkg["model"]
        assert type(m).__module__ == "sklearn.model_selection._search" and type(m.best_estimator_).__name__ == "SVC"
        repr(m)
        m.best_estimator_.get_params()
        sk_pred, sk_dec, sk_proba = m.predict(X), m.decision_function(X), m.predict_proba(X)
    assert np.array_equal(sk_pred, gs.predict(X))
    own_dec = gs.best_estimator_.decision_function(X)
    if kernel == "linear":
        assert np.array_equal(sk_dec, own_dec)
    else:   # numpy's exp and libm's may differ in the last place
        assert np.allclose(sk_dec, own_dec, rtol=1e-12, atol=1e-12)
    dev = float(np.abs(sk_proba - gs.predict_proba(X)).max())
    print("predict_proba: largest deviation from scikit-learn %.3g" % dev)
    assert dev <= 1e-9
    be, sk = gs.best_estimator_, m.best_estimator_
    assert np.array_equal(sk.support_, be.support_) and np.array_equal(sk.n_support_, be.n_support_)
    assert np.array_equal(sk.dual_coef_, be.dual_coef_) and np.array_equal(sk.intercept_, be.intercept_)
    assert np.array_equal(sk.probA_, be.probA_) and np.array_equal(sk.probB_, be.probB_)
    if kernel == "linear":
        assert np.allclose(sk.coef_, be.coef_, rtol=1e-12, atol=1e-12)
    # the same objects through the real constructors
    real = gs.to_sklearn()
    assert np.array_equal(real.predict(X), sk_pred) and np.array_equal(real.predict_proba(X), sk_proba)
    # `prediction` reads the file without scikit-learn and answers from the Platt pair, not the logistic
    fast = skpickle.load_linear_package(path)
    assert fast is not None and np.array_equal(fast["model"].predict(X), sk_pred)
    assert float(np.abs(fast["model"].predict_proba(X) - sk_proba).max()) <= 1e-9


def test_bc_svm_sits_behind_the_knob(tmp_path, monkeypatch):
    from test_host_modeling import _setup
    monkeypatch.delenv("PSK_SVM", raising=False)
    with pytest.raises(SystemExit) as e:
        _setup(tmp_path, "ds_bonf", ["-bc", "SVM"])
    assert str(e.value) == ("Only the logistic-regression classifier runs on the GPU engine, got 'SVM' "
                            "(SVM/RF/DT/NB are outside the accelerated path).")
    monkeypatch.setenv("PSK_SVM", "1")
    M, _ = _setup(tmp_path, "ds_bonf", ["-bc", "SVM", "--kernel", "linear"])
    assert (M.phenotypes.model_name_long, M.phenotypes.model_name_short) == ("support vector machine", "SVM")
    est, pname, grid = M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()
    assert pname == "C" and np.allclose(grid, 1.0 / np.logspace(-3, 3, 13))
    assert repr(est) == "SVC(kernel='linear', max_iter=1000, probability=True, tol=0.0001)"   # (argparse keeps the int default)
    with pytest.raises(SystemExit):
        _setup(tmp_path, "ds_bonf", ["-bc", "SVM", "--kernel", "rbf"])
    for other in ("RF", "NB", "DT"):
        with pytest.raises(SystemExit):
            _setup(tmp_path, "ds_bonf", ["-bc", other])
    M, _ = _setup(tmp_path, "ds_bonf", [])   # the default classifier is untouched by the knob
    assert M.phenotypes.model_name_short == "log_reg" and M.phenotypes.binary_classifier == "log"
