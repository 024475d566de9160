"""GPU tests (-m gpu) of psk_svc_decision and of the rbf branch of `-bc SVM`: the decision values of new rows against the
fit's own (bit for bit: the operation order is the contract) and against the host loop of model.SVC; RandomizedSearch over
SVC(kernel='rbf') against scikit-learn's recorded search (tests/golden/svm_rbf_search.npz, tools/gen_svm_rbf_golden.py);
`modeling -bc SVM --kernel rbf` and `prediction` end to end behind PSK_SVM=1 PSK_SVM_RBF=1."""
import os

import numpy as np
import pytest

from test_gpu_svm import _close, _run

pytestmark = pytest.mark.gpu

N, P = 70, 130      # three 64-bit words of columns; neither is a multiple of a 16-wide tile


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gz():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svm_rbf_search.npz"))


def _designs():
    """(name, X[70][130], y): a 0/1 design and a count design (0..5), the label following a few columns."""
    rng = np.random.default_rng(11)
    y = (np.arange(N) % 2).astype(np.int64)
    rng.shuffle(y)
    B = (rng.random((N, P)) < 0.4).astype(np.float64)
    B[:, :12] = np.where(rng.random((N, 12)) < 0.2, 1 - y[:, None], y[:, None])
    Cn = rng.integers(0, 6, (N, P)).astype(np.float64)
    Cn[:, :8] = np.clip(Cn[:, :8] + 2 * y[:, None] - 1, 0, 5)
    return [("0/1", B, y), ("counts", Cn, y)]


def _support(dual, y):
    """The solver's order: class 0 first, input order within a class."""
    nz = dual != 0
    return np.concatenate([np.nonzero(nz & (y == 0))[0], np.nonzero(nz & (y == 1))[0]])


@pytest.fixture(scope="module")
def fitted(ctx):
    """One psk_svc_fit call per (design, kernel): {(design, kernel): (X, y, [(gamma, fold, dual, rho, dec)])}."""
    from phenotypeseeker_amd import cv
    out = {}
    for name, X, y in _designs():
        folds = cv.stratified_kfold(y, 5)
        for kern, gammas in (("linear", (0.0,)), ("rbf", (1.0 / P, 0.5))):
            plan = [(g, f) for g in gammas for f in (-1, 0, 1, 2, 3, 4)]
            dual, rho, dec, _ = ctx.svc_fit(X, y, folds, [1.0] * len(plan), [f for _, f in plan], kernel=kern,
                                            fit_gamma=[g for g, _ in plan], tol=1e-3, max_iter=1000)
            out[(name, kern)] = (X, y, [(g, f, dual[k], float(rho[k]), dec[k]) for k, (g, f) in enumerate(plan)])
    return out


def test_decision_equals_the_fits_own_bit_for_bit(ctx, fitted):
    """svc_decision on the fit's support vectors in the solver's order reproduces dec_out of every fit, all 70 samples, the
    held-out ones included: both kernels, both routes, gamma 1/p and 0.5, folds 0..4 and the all-sample fit."""
    checked = 0
    for (name, kern), (X, y, fits) in fitted.items():
        for g, f, dual, rho, dec in fits:
            sup = _support(dual, y)
            assert len(sup) >= 2
            got = ctx.svc_decision(X, X[sup], dual[sup], rho, kernel=kern, gamma=g)
            assert np.array_equal(got, dec), (name, kern, g, f, float(np.abs(got - dec).max()))
            checked += 1
    assert checked == 2 * (6 + 12)


def _model(fitted, name, kern):
    X, y, fits = fitted[(name, kern)]
    g, _, dual, rho, _ = fits[0]
    sup = _support(dual, y)
    return X[sup], dual[sup], rho, g


@pytest.mark.parametrize("kern", ["linear", "rbf"])
def test_a_result_depends_on_its_own_row_only(ctx, fitted, kern):
    """m = 1, 17 and 300 fresh rows (300: several workgroups): a slice of the rows gives the slice of the results, and a row
    with a 2.0 appended to the 0/1 rows -- which moves the call from the packed to the dense route -- leaves them unchanged."""
    rng = np.random.default_rng(5)
    for name in ("0/1", "counts"):
        SV, coef, rho, g = _model(fitted, name, kern)
        fresh = (rng.random((300, P)) < 0.4).astype(np.float64) if name == "0/1" else rng.integers(0, 6, (300, P)).astype(np.float64)
        full = ctx.svc_decision(fresh, SV, coef, rho, kernel=kern, gamma=g)
        assert full.shape == (300,) and np.all(np.isfinite(full)) and len(set(full.tolist())) > 100
        for lo, hi in ((0, 1), (299, 300), (5, 22), (31, 33), (64, 300)):
            part = ctx.svc_decision(fresh[lo:hi], SV, coef, rho, kernel=kern, gamma=g)
            assert np.array_equal(part, full[lo:hi]), (name, lo, hi)
        if name == "0/1":
            odd = fresh[:1].copy()
            odd[0, 77] = 2.0
            for m in (1, 17, 300):
                dense = ctx.svc_decision(np.vstack([fresh[:m], odd]), SV, coef, rho, kernel=kern, gamma=g)
                assert np.array_equal(dense[:m], full[:m]), m
                assert dense[m] != full[0]


def _ascending(X, SV, coef, rho, kern, gamma):
    """The contract written out in NumPy: dot products and norms summed over the columns in ascending order, the support
    vectors added one after the other.  Returns (dec, sum_j |coef_j| K_ij)."""
    d, sa, sb = np.zeros((len(X), len(SV))), np.zeros(len(SV)), np.zeros(len(X))
    for k in range(X.shape[1]):
        d += SV[None, :, k] * X[:, None, k]
        sa += SV[:, k] * SV[:, k]
        sb += X[:, k] * X[:, k]
    K = d if kern == "linear" else np.exp(-gamma * (sa[None, :] + sb[:, None] - 2 * d))
    s = np.zeros(len(X))
    for j in range(len(SV)):
        s += coef[j] * K[:, j]
    return s - rho, np.abs(coef[None, :] * K).sum(axis=1)


def test_device_decision_against_the_host(ctx):
    """model.SVC's host loop is the yardstick.  Linear kernel: equal to the bit on 0/1 and count designs (exact dot products,
    the same order of the sum), and on a float design against the column-ascending restatement.  rbf: the device's exp and
    the host's may each be one unit in the last place off, and the n_sv additions then round independently, so a row may
    differ by (n_sv + 4) 2^-52 (sum_j |coef_j| K_ij + |rho|), computed from the host's values."""
    from phenotypeseeker_amd import model as M
    rng = np.random.default_rng(9)
    F = rng.standard_normal((40, 12)).astype(np.float32).astype(np.float64)
    yF = (F[:, 0] + 0.5 * F[:, 1] + 0.3 * rng.standard_normal(40) > 0).astype(np.int64)
    fresh = {"0/1": (rng.random((90, P)) < 0.4).astype(np.float64), "counts": rng.integers(0, 6, (90, P)).astype(np.float64),
             "float": rng.standard_normal((90, 12)).astype(np.float32).astype(np.float64)}
    worst = 0.0
    for name, X, y in _designs() + [("float", F, yF)]:
        for kern, gamma in (("linear", "scale"), ("rbf", 1.0 / X.shape[1]), ("rbf", "scale")):
            m = M.SVC(C=1.0, kernel=kern, gamma=gamma, tol=1e-3, max_iter=1000).fit(X, y, ctx)
            Xn = np.vstack([X, fresh[name]])
            dev = m._libsvm_decision(Xn, ctx)
            coef, rho = -m.dual_coef_[0], m.intercept_[0]
            assert m._on_device(Xn) and np.array_equal(m.decision_function(Xn, ctx), -dev)
            assert np.array_equal(m.predict(Xn, ctx), (dev <= 0).astype(int))
            if name == "float":
                host, mass = _ascending(Xn, m.support_vectors_, coef, rho, kern, m._gamma)
            else:
                host = m._libsvm_decision(Xn)
                mass = np.abs(coef[None, :] * m._kernel(Xn)).sum(axis=1)
            if kern == "linear":
                assert np.array_equal(dev, host), (name, float(np.abs(dev - host).max()))
                continue
            bound = (len(coef) + 4) * 2.0 ** -52 * (mass + abs(rho))
            ratio = float((np.abs(dev - host) / bound).max())
            worst = max(worst, ratio)
            print("%s rbf gamma=%r: %d support vectors, largest |device - host| / bound = %.3g" % (name, gamma, len(coef), ratio))
            assert np.all(np.abs(dev - host) <= bound), (name, gamma, ratio)
    print("rbf: largest observed ratio to the bound %.3g" % worst)


def test_refusals_leave_the_context_usable(ctx, fitted):
    from phenotypeseeker_amd._lib import PskError
    SV, coef, rho, g = _model(fitted, "0/1", "rbf")
    X = SV[:5]
    good = ctx.svc_decision(X, SV, coef, rho, kernel="rbf", gamma=g)
    bad_sv = SV.copy()
    bad_sv[3, 100] = np.nan
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    Xf, SVf = f32(X), f32(SV)
    out = np.zeros(5)

    def raw(kernel):
        ctx._check(ctx._lib.psk_svc_decision(ctx._h, Xf.ctypes.data, 5, P, SVf.ctypes.data, len(SVf), coef.ctypes.data, float(rho), kernel,
                                             float(g), out.ctypes.data), "psk_svc_decision")
    for what, call in (("gamma", lambda: ctx.svc_decision(X, SV, coef, rho, kernel="rbf", gamma=-1.0)),
                       ("gamma", lambda: ctx.svc_decision(X, SV, coef, rho, kernel="rbf", gamma=np.inf)),
                       ("kernel", lambda: raw(2)),
                       ("finite", lambda: ctx.svc_decision(X, bad_sv, coef, rho, kernel="rbf", gamma=g)),
                       ("finite", lambda: ctx.svc_decision(X, SV, coef, np.nan, kernel="rbf", gamma=g)),
                       ("n_sv", lambda: ctx.svc_decision(X, SV[:0], coef[:0], rho, kernel="rbf", gamma=g))):
        with pytest.raises(PskError) as e:
            call()
        assert e.value.code == -1 and what in str(e.value), (what, str(e.value))
        assert np.array_equal(ctx.svc_decision(X, SV, coef, rho, kernel="rbf", gamma=g), good), what
    raw(1)
    assert np.array_equal(out, good)


def test_randomized_search_equals_scikit_learns(ctx, gz):
    """RandomizedSearch(SVC(rbf)) on the fixture's 96 x 40 design: the recorded candidates in order; split scores, means,
    ranks and the best index equal (the criteria of test_grid_search_scores_equal_scikit_learn); the refit's support_, dual_coef_
    and intercept_ by the exact-path tier's (1e-6 relative)."""
    from phenotypeseeker_amd import model as M
    n, p = (int(v) for v in gz["shape"])
    X, y = np.unpackbits(gz["X"], axis=1)[:, :p].astype(np.float64), gz["y"].astype(np.int64)
    grid = {"C": gz["axis"].tolist(), "gamma": gz["axis"].tolist()}
    rs = M.RandomizedSearch(M.SVC(kernel="rbf", max_iter=1000, tol=1e-4), grid, 25, 5, random_state=0).fit(X, y, ctx)
    r = rs.cv_results_
    assert [q["C"] for q in r["params"]] == gz["search_C"].tolist() and [q["gamma"] for q in r["params"]] == gz["search_gamma"].tolist()
    assert [list(q) for q in r["params"]] == [gz["search_keys"].tolist()] * 25
    for f in range(5):
        assert np.array_equal(r["split%d_test_score" % f], gz["search_splits"][:, f]), f
    assert np.array_equal(r["mean_test_score"], gz["search_mean"]) and np.array_equal(r["rank_test_score"], gz["search_rank"])
    assert rs.best_index_ == int(gz["search_best_index"])
    be = rs.best_estimator_
    print("best candidate %d %r: %d support vectors, %d iterations (scikit-learn %d)"
          % (rs.best_index_, rs.best_params_, len(be.support_), int(be.n_iter_[0]), int(gz["search_refit_iters"][0])))
    assert np.array_equal(be.support_, gz["search_support"])
    assert _close(be.dual_coef_, gz["search_dual_coef"]) and _close(be.intercept_, gz["search_intercept"])
    # the device's decision values of the refit are the model's own
    assert np.array_equal(be.predict(X, ctx), be.predict(X))


def test_cli_end_to_end_rbf(tmp_path, monkeypatch):
    """PSK_SVM=1 PSK_SVM_RBF=1 modeling -bc SVM --kernel rbf --n_iter 5, twice: the same bytes; NA coefficients, both best
    parameters in the summary, a .pkl the package's reader and scikit-learn's both read; `prediction` on the same genomes writes
    the host's classes and probabilities; another PSK_SVM_SEED draws other candidates."""
    from helpers import load_dataset
    from test_host_modeling import _write_dataset
    from phenotypeseeker_amd import model as M, prediction as PR, skpickle
    monkeypatch.setenv("PSK_SVM", "1")
    monkeypatch.setenv("PSK_SVM_RBF", "1")
    monkeypatch.delenv("PSK_SVM_SEED", raising=False)
    ds = load_dataset("ds_omitB")
    names = ["summary_of_SVM_analysis_Pheno.txt", "k-mers_and_coefficients_in_SVM_model_Pheno.txt", "SVM_model_Pheno.pkl"]
    argv = ["modeling", "data.pheno", "-bc", "SVM", "--kernel", "rbf", "--n_iter", "5", "--omit_B_correction", "--n_kmers", "100"]
    runs = []
    for rep, seed in enumerate((None, None, "1")):
        if seed is not None:
            monkeypatch.setenv("PSK_SVM_SEED", seed)
        wd = tmp_path / ("run%d" % rep)
        wd.mkdir()
        _write_dataset(ds, str(wd))
        _run(wd, argv)
        for nm in names:
            assert (wd / nm).exists(), nm
        runs.append(wd)
    monkeypatch.delenv("PSK_SVM_SEED")
    for nm in names:
        assert (runs[0] / nm).read_bytes() == (runs[1] / nm).read_bytes(), "%s differs between two runs" % nm
    wd = runs[0]
    summary = (wd / names[0]).read_text()
    assert "Parameters:\nSVC(max_iter=1000, probability=True, tol=0.0001)\n" in summary        # rbf is the default kernel
    grid_lines = lambda text: [ln for ln in text.splitlines() if " for {'gamma': " in ln and "'C': " in ln]
    assert len(grid_lines(summary)) == 5
    best = summary.split("Best parameters found on development set: \n")[1].splitlines()[:2]
    assert best[0].startswith("gamma : ") and best[1].startswith("C : ")
    other = grid_lines((runs[2] / names[0]).read_text())
    assert len(other) == 5 and [ln.split(" for ")[1] for ln in other] != [ln.split(" for ")[1] for ln in grid_lines(summary)]
    coef_lines = (wd / names[1]).read_text().splitlines()
    assert coef_lines[0] == "K-mer\tcoef._in_SVM_model\tNo._of_samples_with_k-mer\tSamples_with_k-mer" and len(coef_lines) > 1
    assert all(ln.split("\t")[1] == "NA" for ln in coef_lines[1:])
    pkg = skpickle.load_linear_package(str(wd / names[2]))
    assert pkg is not None and isinstance(pkg["model"], M.SVC) and pkg["model"].kernel == "rbf"
    assert (pkg["model"].gamma, pkg["model"].C) == (float(best[0].split(" : ")[1]), float(best[1].split(" : ")[1]))
    os.chdir(wd)
    with open("samples.txt", "w") as f:
        for line in open("data.pheno").read().splitlines()[1:]:
            if line.strip():
                f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    _run(wd, ["prediction", "samples.txt", "phenos.txt"])
    out = open("predictions_Pheno.txt").read().splitlines()
    assert out[0] == "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class"
    ph = PR.Input.phenos["Pheno"]
    assert isinstance(ph.model, M.SVC) and ph.matrix.shape == (len(out) - 1, len(pkg["kmers"]))
    host_pred, host_proba = pkg["model"].predict(ph.matrix), pkg["model"].predict_proba(ph.matrix)
    assert [ln.split("\t")[1] for ln in out[1:]] == [str(v) for v in host_pred]
    assert [ln.split("\t")[2] for ln in out[1:]] == [str(round(pr[1], 2)) for pr in host_proba]
    block = summary.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: ln.split()[2] for ln in block.splitlines()}
    pred = {ln.split("\t")[0]: ln.split("\t")[1] for ln in out[1:]}
    assert {k: pred[k] for k in trained} == trained
    try:
        import sklearn  # noqa: F401
    except ImportError:
        return
    import joblib
    sk = joblib.load(str(wd / names[2]))["model"]
    assert type(sk).__name__ == "RandomizedSearchCV" and sk.best_estimator_.kernel == "rbf" and sk.n_iter == 5 and sk.random_state == 0
    assert np.array_equal(sk.predict(ph.matrix), host_pred)
