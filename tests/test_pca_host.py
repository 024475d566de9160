"""CPU tests (-m "not gpu") of the `--pca` path's host side: the NumPy restatement (tests/pca_restated.py: the Gram route of
psk_pca_fit, the stated order of psk_pca_transform) against scikit-learn's recorded StandardScaler() + PCA() fits
(tests/golden/pca_kat.npz, tools/gen_pca_golden.py) under the bounds pca_restated.py derives, _stats.welch_weighted against
oracle.ttest_row, the model_pca twins in a .pkl three ways, the PSK_PCA knob and the files a host run writes."""
import os

import numpy as np
import pytest

import pca_restated as R

SHAPES = {"A": (24, 40), "B": (96, 300), "C": (130, 64), "D": (200, 15), "E": (65, 700)}
OFF = "--pca is outside the accelerated path."


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


@pytest.fixture(scope="module")
def restated(fx):
    """The restatement's fit of every design; computed once."""
    return {name: R.fit(fx.designs[name]["X"]) for name in fx.names}


def test_fixture_holds_what_the_tests_need(fx):
    assert fx.sklearn_version == "1.7.2" and fx.names == list(SHAPES)
    for name, D in fx.designs.items():
        X, n, p = D["X"], D["n"], D["p"]
        assert (n, p) == SHAPES[name] and np.array_equal(X, np.round(X)) and X.min() == 0 and X.max() == (4 if name == "C" else 1)
        assert np.array_equal(X[:, 1], X[:, 0]) and 0 < np.count_nonzero(X[:, 0]) < n
        if name != "D":       # (tools/gen_pca_golden.py says why D has the duplicate only)
            assert np.array_equal(X[:, 2], X.max() - X[:, 0])
        assert D["solver"] == ("covariance_eigh" if name == "D" else "full")
        assert set(np.unique(D["y"])) == {0, 1} and len(np.unique(D["w"])) > n // 2
        k = int(D["keep_ev"].sum())
        assert k > 0 and np.array_equal(D["keep_ev"], np.arange(min(n, p)) < k) and np.array_equal(D["keep_ev"], D["ev"] > 0.9)
        assert D["ttest"].shape == (k, 5) and np.array_equal(D["keep"][:k], D["ttest"][:, 1] < 0.01) and not D["keep"][k:].any()
        assert D["keep"].any() and D["n_stored"] >= k and D["scores"].shape == (n, D["n_stored"])
    assert fx.designs["C"]["var"][-1] == 0.0 and fx.designs["C"]["scale"][-1] == 1.0
    assert os.path.getsize(fx.path) < 1 << 20


def test_restatement_lies_within_its_bounds_of_scikit_learn(fx, restated):
    for name, D in fx.designs.items():
        r, n, p = restated[name], D["n"], D["p"]
        Z, lam = r["Z"], r["lambda"]
        assert np.array_equal(r["mean"], D["mean"]), name                                     # integer sums: bit for bit
        tol_var = R.var_tolerance(n, r["mean"], r["var"])
        assert np.all(np.abs(r["var"] - D["var"]) <= tol_var), name
        assert np.array_equal(r["scale"], np.where(r["var"] == 0, 1.0, np.sqrt(r["var"]))), name
        tol_lam = R.lambda_tolerance(Z, lam[0])
        assert np.all(np.abs(lam - D["lambda"]) <= tol_lam) and np.all(np.diff(lam) <= 0) and lam.min() >= 0, name
        k = int(D["keep_ev"].sum())
        tol_v = R.vector_tolerance(lam, tol_lam)[:k]
        assert np.all(tol_v <= 1e-6), name                                                    # the comparison is not vacuous
        dv = np.linalg.norm(r["components"][:k] - D["components"][:k], axis=1)
        assert np.all(dv <= tol_v), (name, float((dv / tol_v).max()))
        tol_s = np.sqrt(lam[0]) * tol_v + np.sqrt(n) * R.fit_score_tolerance(Z, r["components"][:k], lam, tol_lam).max(axis=0)
        ds = np.linalg.norm(r["scores"][:, :k] - D["scores"][:, :k], axis=0)
        assert np.all(ds <= tol_s), (name, float((ds / tol_s).max()))
        assert np.array_equal(R.kept_prefix(lam, n), D["keep_ev"]), name
        dead = lam <= R.rank_floor(n, p, lam[0])
        assert dead.sum() == min(n, p) - D["n_stored"] and not r["components"][dead].any() and not r["scores"][:, dead].any(), name
        print("design %s: K = %.2f; shares of the bounds: var %.3g, lambda %.3g, kept components %.3g, scores %.3g"
              % (name, R.rho(Z, lam[0]) + R.K_FIXED, float((np.abs(r["var"] - D["var"]) / np.maximum(tol_var, 1e-300)).max()),
                 float(np.abs(lam - D["lambda"]).max() / tol_lam), float((dv / tol_v).max()), float((ds / tol_s).max())))


def test_the_stated_order_of_the_transform(fx, restated):
    """pca_restated adds column by column, model_pca step by step: the same order, the same bits; a row's scores do not depend
    on the rows around it nor on the other components; scikit-learn's own transform lies within the transform bound."""
    from phenotypeseeker_amd import model_pca
    for name in ("A", "C", "E"):
        D, r = fx.designs[name], restated[name]
        k = int(D["keep_ev"].sum())
        comp = r["components"][:k]
        a = R.transform_in_order(D["X"], r["mean"], r["scale"], comp)
        b = model_pca.scores_in_order(D["X"], r["mean"], r["scale"], comp)
        assert np.array_equal(a, b), name
        hi = min(D["n"], 70)
        assert np.array_equal(model_pca.scores_in_order(D["X"][3:hi], r["mean"], r["scale"], comp), b[3:hi])
        assert np.array_equal(model_pca.scores_in_order(D["X"][-1:], r["mean"], r["scale"], comp[2:3]), b[-1:, 2:3])
        tol = R.transform_tolerance(r["Z"], comp)
        assert np.all(np.abs(b - r["Z"] @ comp.T) <= tol), name
        assert np.all(np.abs(b - r["scores"][:, :k]) <= R.fit_score_tolerance(r["Z"], comp, r["lambda"], R.lambda_tolerance(r["Z"], r["lambda"][0])))


def test_welch_weighted_is_the_reference_t_test(fx, oracle):
    """conduct_t_test's computation with the roles swapped: the groups are the scores of the phenotype == 1 and == 0 samples.
    t and the two means follow the oracle's order of summation (==); the p-value is another evaluation of the same incomplete
    beta function, both converged to 1e-16 relative: 1e-12 relative."""
    from phenotypeseeker_amd import _stats
    n_tests = 0
    for name, D in fx.designs.items():
        y, w = D["y"], D["w"]
        for c in range(int(D["keep_ev"].sum())):
            s = D["scores"][:, c]
            t, p, mx, my = _stats.welch_weighted(s[y == 1], s[y == 0], w[y == 1], w[y == 0])
            want = oracle.ttest_row(y == 1, s, w, 0, D["n"])
            assert tuple(want) == tuple(D["ttest"][c][:4]) + (int(D["ttest"][c][4]),), (name, c)     # the fixture is the oracle's
            assert (t, mx, my) == (want[0], want[2], want[3]), (name, c)
            assert abs(p - want[1]) <= 1e-12 * want[1], (name, c, p, want[1])
            n_tests += 1
    assert n_tests == sum(int(D["keep_ev"].sum()) for D in fx.designs.values())


def test_pca_model_file_round_trips_three_ways(tmp_path, fx, restated):
    """A shell-written package loads with joblib.load into real sklearn objects, without warnings; scikit-learn's own transforms
    of them reproduce the package's scores within the transform bound; the stub reader returns the same model."""
    pytest.importorskip("sklearn")
    import warnings

    import joblib
    from phenotypeseeker_amd import model_pca, skpickle
    D, r = fx.designs["B"], restated["B"]
    scaler, pca, scores = model_pca.fit(R.Engine(), D["X"])
    keep = D["keep"]
    assert np.array_equal(scores, r["scores"]) and pca.n_components_ == 96 and scaler.n_samples_seen_ == 96
    assert np.array_equal(pca.explained_variance_, r["lambda"] / 95) and np.array_equal(pca.singular_values_, np.sqrt(r["lambda"]))
    assert abs(pca.explained_variance_ratio_.sum() - 1.0) < 1e-12 and not pca.mean_.any() and pca.noise_variance_ == 0.0
    shells = {"scaler": scaler.to_sklearn_shell(), "pca_model": pca.to_sklearn_shell()}
    assert all(v is not None for v in shells.values()), "no template for the installed scikit-learn: run tools/make_sklearn_shells.py"
    from phenotypeseeker_amd.model import L1LogisticRegression
    model = L1LogisticRegression()._set(np.ones(int(keep.sum())), 0.25)
    path = os.path.join(tmp_path, "pca.pkl")
    with open(path, "wb") as f:
        f.write(skpickle.dumps(dict(shells, model=model._sklearn().shell(), kmers=np.array(["ACGT"] * D["p"], dtype=object), pca=True,
                                    pred_scale="binary", PCs_to_keep=keep)))
    rng = np.random.default_rng(5)
    Xn = np.vstack([D["X"], (rng.random((40, D["p"])) < 0.4).astype(np.float64)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pkg = joblib.load(path)
        sk_s, sk_p = pkg["scaler"], pkg["pca_model"]
        assert (type(sk_s).__module__, type(sk_s).__name__) == ("sklearn.preprocessing._data", "StandardScaler")
        assert (type(sk_p).__module__, type(sk_p).__name__) == ("sklearn.decomposition._pca", "PCA")
        got = sk_p.transform(sk_s.transform(Xn))[:, pkg["PCs_to_keep"]]
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    ref_s = StandardScaler().fit(D["X"])
    assert sk_s.__dict__.keys() == ref_s.__dict__.keys() and sk_p.__dict__.keys() == PCA().fit(ref_s.transform(D["X"])).__dict__.keys()
    assert sk_s.get_params() == StandardScaler().get_params() and sk_p.get_params() == PCA().get_params()
    assert pkg["pca"] is True and np.array_equal(pkg["PCs_to_keep"], keep) and pkg["PCs_to_keep"].dtype == bool
    mine = model_pca.project(scaler, pca, Xn, keep)
    Zn = R.standardise(Xn, scaler.mean_, scaler.scale_)
    assert np.all(np.abs(got - mine) <= R.transform_tolerance(Zn, pca.components_[keep]))
    assert np.array_equal(mine[:96], model_pca.project(scaler, pca, D["X"], keep)) and np.array_equal(mine, model_pca.project(scaler, pca, Xn, keep, R.Engine()))
    real_s, real_p = scaler.to_sklearn(), pca.to_sklearn()    # the same objects through the real constructors
    assert type(real_s) is type(sk_s) and type(real_p) is type(sk_p)
    assert np.array_equal(real_p.transform(real_s.transform(Xn))[:, keep], got)
    fast = skpickle.load_linear_package(path)                 # what `phenotypeseeker prediction` reads the file with
    assert fast is not None and isinstance(fast["scaler"], model_pca.StandardScaler) and isinstance(fast["pca_model"], model_pca.PCA)
    assert np.array_equal(fast["PCs_to_keep"], keep) and fast["pca"] is True
    assert np.array_equal(model_pca.project(fast["scaler"], fast["pca_model"], Xn, fast["PCs_to_keep"]), mine)
    for k in ("mean_", "var_", "scale_"):
        assert np.array_equal(getattr(fast["scaler"], k), getattr(scaler, k)), k
    for k in ("components_", "explained_variance_", "explained_variance_ratio_", "singular_values_", "mean_"):
        assert np.array_equal(getattr(fast["pca_model"], k), getattr(pca, k)), k
    # both classes' own transform: the NumPy route and the engine's give the same bits
    assert np.array_equal(scaler.transform(Xn), scaler.transform(Xn, R.Engine()))
    assert np.array_equal(pca.transform(Xn[:5]), pca.transform(Xn[:5], R.Engine()))
    # a whitening PCA is left to scikit-learn
    import pickle
    other = os.path.join(tmp_path, "other.pkl")
    with open(other, "wb") as f:
        pickle.dump(dict(pkg, pca_model=PCA(whiten=True).fit(ref_s.transform(D["X"]))), f, protocol=2)
    assert skpickle.load_linear_package(other) is None


def test_pca_sits_behind_the_knob(tmp_path, monkeypatch):
    from test_host_modeling import _setup
    for knob in ("PSK_PCA", "PSK_NB", "PSK_SVM", "PSK_DT", "PSK_RF"):
        monkeypatch.delenv(knob, raising=False)
    for flag in (None, "0"):
        if flag is not None:
            monkeypatch.setenv("PSK_PCA", flag)
        for extra in ([], ["--penalty", "L2"]):
            with pytest.raises(SystemExit) as e:
                _setup(tmp_path, "ds_bonf", ["--pca"] + extra)
            assert str(e.value) == OFF
    monkeypatch.setenv("PSK_PCA", "1")
    for extra in ([], ["--penalty", "L2"]):
        M, _ = _setup(tmp_path, "ds_bonf", ["-bc", "log", "--pca"] + extra)
        assert M.phenotypes.pca is True and M.phenotypes.model_name_short == "log_reg"
    with pytest.raises(SystemExit) as e:                      # the knob of --pca does not open an estimator
        _setup(tmp_path, "ds_bonf", ["-bc", "SVM", "--pca"])
    assert "SVM/RF/DT/NB are outside the accelerated path" in str(e.value)
    monkeypatch.setenv("PSK_SVM", "1")
    M, _ = _setup(tmp_path, "ds_bonf", ["-bc", "SVM", "--pca"])
    assert M.phenotypes.pca is True and M.phenotypes.binary_classifier == "SVM"
    messages = {"DT": "The decision tree on the GPU engine takes the 0/1 presence matrix only: --pca is not supported with -bc DT.",
                "RF": "The random forest on the GPU engine takes the 0/1 presence matrix only: --pca is not supported with -bc RF.",
                "NB": "The naive Bayes classifier on the GPU engine takes the k-mer presence matrix only: --pca is not supported with -bc NB."}
    for bc, text in messages.items():                         # today's messages, with and without PSK_PCA
        monkeypatch.setenv("PSK_" + bc, "1")
        for on in (True, False):
            monkeypatch.setenv("PSK_PCA", "1" if on else "0")
            with pytest.raises(SystemExit) as e:
                _setup(tmp_path, "ds_bonf", ["-bc", bc, "--pca"])
            assert str(e.value) == text
    monkeypatch.setenv("PSK_PCA", "1")
    M, _ = _setup(tmp_path, "ds_bonf", [])                    # without --pca the knob changes nothing
    assert not M.phenotypes.pca


def test_a_continuous_phenotype_is_refused(tmp_path, monkeypatch):
    from test_host_modeling import _args
    from phenotypeseeker_amd import modeling as M
    os.chdir(tmp_path)
    with open("data.pheno", "w") as f:
        f.write("ID\tAddr\tMIC\nA\ta.fa\t0.25\nB\tb.fa\t2\nC\tc.fa\t8\nD\td.fa\t4\n")

    def run():
        a = _args(["--pca"])
        M.Input.reset()
        M.Input.get_input_data(a.inputfile, a.take_logs, a.mpheno)
        assert M.phenotypes.pred_scale == "continuous"
        M.Input.Input_args(a.alphas, a.alpha_min, a.alpha_max, a.n_alphas, a.gammas, a.gamma_min, a.gamma_max, a.n_gammas,
                           a.min, a.max, a.kmer_length, a.cutoff, a.num_threads, a.pvalue, a.n_kmers, a.binary_classifier,
                           a.regressor, a.penalty, a.max_iter, a.tolerance, a.l1_ratio, a.n_splits_cv_outer, a.kernel,
                           a.n_iter, a.n_splits_cv_inner, a.testset_size, a.train_on_whole, a.logreg_solver, a.jump_to,
                           a.pca, a.real_counts, a.omit_B_correction, a.kmerDB)
    monkeypatch.delenv("PSK_PCA", raising=False)
    with pytest.raises(SystemExit) as e:
        run()
    assert str(e.value) == OFF
    monkeypatch.setenv("PSK_PCA", "1")
    with pytest.raises(SystemExit) as e:
        run()
    assert "--pca" in str(e.value) and "binary phenotype" in str(e.value)
    M.phenotypes.pred_scale = "binary"        # (a class attribute: the next test module starts from the default)


class _HostEngine(R.Engine):
    """The PCA calls from the restatement, the logistic fits from scikit-learn's LogisticRegression on the CPU; keeps the
    designs it was handed."""

    def __init__(self):
        self.designs = []

    def logreg_l1_fit(self, X, y, folds, fit_param, fit_fold, tol, max_iter):
        from sklearn.linear_model import LogisticRegression
        self.designs.append(np.array(X))
        coef, icpt = np.zeros((len(fit_param), X.shape[1])), np.zeros(len(fit_param))
        for j, (C, f) in enumerate(zip(fit_param, fit_fold)):
            tr = np.asarray(folds) != f
            m = LogisticRegression(penalty="l1", solver="liblinear", C=C, tol=tol, max_iter=max_iter).fit(X[tr], np.asarray(y)[tr])
            coef[j], icpt[j] = m.coef_[0], m.intercept_[0]
        return coef, icpt, np.ones(len(fit_param), dtype=np.int32)


def test_files_of_a_host_run_with_pca(tmp_path, monkeypatch, fx, restated):
    pytest.importorskip("sklearn")
    import joblib
    from test_host_modeling import _args
    from phenotypeseeker_amd import modeling as M
    D, r = fx.designs["B"], restated["B"]
    n, p = D["n"], D["p"]
    os.chdir(tmp_path)
    names = ["S%04d" % i for i in range(n)]
    kmers = ["".join("ACGT"[(j >> (2 * b)) & 3] for b in range(13)) for j in range(p)]
    with open("data.pheno", "w") as f:
        f.write("ID\tAddresses\tPheno\n" + "".join("%s\t%s.fasta\t%d\n" % (nm, nm, v) for nm, v in zip(names, D["y"])))
    with open("Pheno_MLdf.csv", "w") as f:
        f.write(",".join([""] + kmers + ["weights", "phenotype"]) + "\n")
        for i, nm in enumerate(names):
            f.write(",".join([nm] + [str(int(v)) for v in D["X"][i]] + [repr(float(D["w"][i])), str(int(D["y"][i]))]) + "\n")
    monkeypatch.setenv("PSK_PCA", "1")
    a = _args(["-jt", "modelling", "-bc", "log", "--pca", "--n_kmers", "300"])
    M.Input.reset()
    M.Input.get_input_data(a.inputfile, a.take_logs, a.mpheno)
    M.Input.Input_args(a.alphas, a.alpha_min, a.alpha_max, a.n_alphas, a.gammas, a.gamma_min, a.gamma_max, a.n_gammas,
                       a.min, a.max, a.kmer_length, a.cutoff, a.num_threads, a.pvalue, a.n_kmers, a.binary_classifier,
                       a.regressor, a.penalty, a.max_iter, a.tolerance, a.l1_ratio, a.n_splits_cv_outer, a.kernel,
                       a.n_iter, a.n_splits_cv_inner, a.testset_size, a.train_on_whole, a.logreg_solver, a.jump_to,
                       a.pca, a.real_counts, a.omit_B_correction, a.kmerDB)
    ph = M.Input.phenotypes_to_analyse["Pheno"]
    engine = _HostEngine()
    ph.machine_learning_modelling(engine)
    keep = D["keep"]
    kept = np.nonzero(keep)[0]
    want = r["scores"][:, keep].astype(np.float32).astype(np.float64)
    assert engine.designs and all(np.array_equal(X, want) for X in engine.designs)      # the search saw the kept scores, as float32
    assert not os.path.exists("k-mers_and_coefficients_in_log_reg_model_Pheno.txt")
    lines = open("PCs_and_coefficients_in_log_reg_model_Pheno.txt").read().splitlines()
    assert lines[0] == "PC\tcoef._in_log_reg_model\texplained_variance\texplained_variance_ratio\tt-test_statistic\tt-test_pvalue"
    assert len(lines) == 1 + len(kept)
    coef = ph.model_fitted.best_estimator_.coef_[0]
    ev = r["lambda"] / (n - 1)
    for i, c in enumerate(kept):
        assert lines[1 + i] == f"PC_{c + 1}\t{np.float64(coef[i])}\t{ev[c]}\t{ev[c] / ev.sum()}\t{np.float64(ph.PC['t'][i])}\t{np.float64(ph.PC['p'][i])}", i
        # the fixture's t-test is of scikit-learn's scores, the run's of the restatement's: the two sets of scores agree to 1e-10
        # relative at worst (sqrt(lambda_1) tol_v), and t and log p are smooth in them
        assert abs(ph.PC["t"][i] - D["ttest"][c][0]) <= 1e-8 * abs(D["ttest"][c][0])
        assert abs(ph.PC["p"][i] - D["ttest"][c][1]) <= 1e-6 * D["ttest"][c][1]
    pkg = joblib.load("log_reg_model_Pheno.pkl")
    assert set(pkg) == {"model", "kmers", "pca", "pred_scale", "scaler", "pca_model", "PCs_to_keep"}
    assert pkg["pca"] is True and list(pkg["kmers"]) == kmers and pkg["pred_scale"] == "binary"
    assert np.array_equal(pkg["PCs_to_keep"], keep) and pkg["PCs_to_keep"].dtype == bool and len(pkg["PCs_to_keep"]) == min(n, p)
    assert type(pkg["scaler"]).__name__ == "StandardScaler" and type(pkg["pca_model"]).__name__ == "PCA"
    assert type(pkg["model"]).__name__ == "GridSearchCV" and pkg["model"].best_estimator_.coef_.shape == (1, len(kept))
    with open("Pheno_MLdf.csv") as f:
        assert f.readline().rstrip("\n").split(",")[1:-2] == kmers                      # _MLdf.csv keeps the k-mers
    summary = open("summary_of_log_reg_analysis_Pheno.txt").read()
    block = summary.split("Predicted_phenotype\n")[1].split("\n\n")[0].splitlines()
    assert block == ["%s %s %s" % (nm, y, q) for nm, y, q in zip(names, D["y"], ph.model_fitted.predict(want))]
    # no component survives: the run stops and says so
    monkeypatch.setattr(M._stats, "welch_weighted", lambda *a: (0.0, 1.0, 0.0, 0.0))
    with pytest.raises(SystemExit) as e:
        ph.machine_learning_modelling(_HostEngine())
    assert "no principal component" in str(e.value)


def test_abi_names_the_pca_entry_points():
    from phenotypeseeker_amd import _lib
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psk.h")) as f:
        header = f.read()
    assert "---- f11:" in header
    for name in ("psk_pca_fit", "psk_pca_transform"):
        assert name in _lib.exported_names()
        assert "int %s(psk_ctx *ctx" % name in header
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib._SIGNATURES[name][1]), name
