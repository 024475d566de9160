"""CPU tests (-m "not gpu") of the naive-Bayes path's host side: the NumPy restatement (tests/nb_restated.py: scikit-learn's
expressions, the engine's order of summation) against scikit-learn's recorded fits (tests/golden/nb_kat.npz,
tools/gen_nb_golden.py) on EVERY case, model.BernoulliNB with the engine served by the restatement (nb_restated.Engine: the host
code under test is the package's own), its .pkl three ways, the `-bc NB` option handling and the files a run writes.

Against scikit-learn: integers and the two log attributes ==.  The joint log-likelihood is the same p + 2 terms added in
another order; the bound is derived in nb_restated.py: tol_ic = 2 (p + 2) 2^-53 (sum_j x_ij |delta_cj| + |class_log_prior_c| +
|neg_sum_c|) per element, tol_i0 + tol_i1 for predict_proba, labels compared where |jll_0 - jll_1| > tol_i0 + tol_i1, at most
1 % of a case's samples inside that band."""
import os

import numpy as np
import pytest

import nb_restated as R


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


@pytest.fixture(scope="module")
def restated(fx):
    """Per design and case (fc, cc, flp, clp, jll, tol) of the restatement; computed once."""
    out = []
    for D, cases in zip(fx.designs, fx.cases):
        rows = []
        for c in cases:
            fc, cc = R.counts(D["X"] != 0, D["y"], c["train"])
            flp, clp = R.log_attributes(fc, cc)
            rows.append(dict(fc=fc, cc=cc, flp=flp, clp=clp, jll=R.jll_in_order(D["X"] != 0, flp, clp),
                             tol=R.jll_tolerance(D["X"] != 0, c["flp"], c["clp"])))
        out.append(rows)
    return out


def test_fixture_holds_what_the_tests_need(fx):
    assert fx.sklearn_version == "1.7.2" and fx.n_folds == 3
    assert [(D["n"], D["p"]) for D in fx.designs] == [(7, 3), (64, 1), (65, 67), (130, 300), (257, 1031), (4100, 5)]
    for D, cases in zip(fx.designs, fx.cases):
        X, y = D["X"], D["y"]
        assert X.shape == (D["n"], D["p"]) and set(np.unique(X)) <= {0.0, 1.0} and set(np.unique(y)) == {0, 1}
        if D["p"] >= 5:       # a duplicated, a complemented, an all-zero and an all-one column
            assert np.array_equal(X[:, 1], X[:, 0]) and np.array_equal(X[:, 2], 1 - X[:, 0]) and not X[:, 3].any() and X[:, 4].all()
            assert 0 < X[:, 0].sum() < D["n"]
        assert set(np.unique(D["fold"])) == {0, 1, 2}
        for f in range(3):    # stratified: every fold holds both classes in the design's proportion, to a sample
            assert abs(np.sum(y[D["fold"] == f]) - y.sum() / 3) < 1
        assert [c["held"] for c in cases] == [-1, 0, 1, 2]
        for c in cases:
            assert c["fc"].shape == (2, D["p"]) and c["cc"].shape == (2,) and c["cc"].sum() == c["train"].sum() and c["cc"].min() > 0
            assert c["flp"].shape == (2, D["p"]) and c["jll"].shape == (D["n"], 2) and c["proba"].shape == (D["n"], 2)
            assert c["pred"].shape == (D["n"],) and np.array_equal(c["pred"], np.argmax(c["jll"], axis=1))
    unb = [D for D in fx.designs if D["kind"] == "unbalanced"]
    assert unb and all(D["y"].mean() < 0.1 for D in unb)
    assert os.path.getsize(fx.path) < 1 << 20


def test_restatement_equals_scikit_learn_on_every_case(fx, restated):
    n_cases, worst = 0, 0.0
    for d, (D, cases) in enumerate(zip(fx.designs, fx.cases)):
        for k, (c, r) in enumerate(zip(cases, restated[d])):
            assert np.array_equal(r["fc"], c["fc"]) and np.array_equal(r["cc"], c["cc"]), (d, k)
            assert np.array_equal(r["flp"], c["flp"]) and np.array_equal(r["clp"], c["clp"]), (d, k)      # ==, bit for bit
            err, tol = np.abs(r["jll"] - c["jll"]), r["tol"]
            worst = max(worst, float((err / tol).max()))
            print("design %d case %d: max |jll - sklearn| / bound = %.4f" % (d, k, float((err / tol).max())))
            assert np.all(err <= tol), (d, k, float((err / tol).max()))
            band = tol.sum(axis=1)
            assert np.all(np.abs(R.proba(r["jll"]) - c["proba"]) <= band[:, None]), (d, k)
            clear = np.abs(c["jll"][:, 0] - c["jll"][:, 1]) > band
            assert np.mean(~clear) <= 0.01, (d, k)
            assert np.array_equal(np.argmax(r["jll"], axis=1)[clear], c["pred"][clear]), (d, k)
            n_cases += 1
    print("restatement against scikit-learn: %d cases, worst share of the bound %.4f" % (n_cases, worst))
    assert n_cases == 24


def test_the_stated_order_is_what_the_restatement_adds():
    """A design on which the order shows: one row, columns 0, 64 and 1 set, values that do not add associatively."""
    X = np.zeros((1, 130), dtype=bool)
    X[0, [0, 1, 64]] = True
    delta = np.zeros(130)
    delta[0], delta[64], delta[1] = 1e16, 1.0, -1e16
    # lane 0: (0 + 1e16) + 1.0 = 1e16; lane 1: -1e16; butterfly: 1e16 + -1e16 = 0 -- not the 1.0 of the exact sum
    assert R.sum_in_order(X, delta)[0] == 0.0
    delta[0], delta[64], delta[1] = 1e16, -1e16, 1.0
    assert R.sum_in_order(X, delta)[0] == 1.0
    from phenotypeseeker_amd import model_nb
    for dl in (delta, np.arange(130) * 0.1):
        both = np.stack([dl, -dl])
        got = model_nb.jll_in_order(X, both, np.zeros(2), np.zeros(2))
        assert got[0, 0] == R.sum_in_order(X, dl)[0] and got[0, 1] == R.sum_in_order(X, -dl)[0]


@pytest.fixture(scope="module")
def fitted(fx):
    """model.BernoulliNB fitted over the stand-in engine on all samples of every design."""
    from phenotypeseeker_amd import model as M
    return [M.BernoulliNB().fit(D["X"], D["y"], R.Engine()) for D in fx.designs]


def test_estimator_over_the_stand_in_engine(fx, fitted, restated):
    from phenotypeseeker_amd import model as M
    for d, (D, m) in enumerate(zip(fx.designs, fitted)):
        c, r = fx.cases[d][0], restated[d][0]
        assert repr(m) == "BernoulliNB()" and list(m.classes_) == [0, 1] and m.n_features_in_ == D["p"]
        assert m.feature_count_.dtype == np.float64 and m.class_count_.dtype == np.float64
        assert np.array_equal(m.feature_count_, c["fc"]) and np.array_equal(m.class_count_, c["cc"])
        assert np.array_equal(m.feature_log_prob_, c["flp"]) and np.array_equal(m.class_log_prior_, c["clp"])
        jll = m._joint_log_likelihood(D["X"])
        assert np.array_equal(jll, r["jll"])                                       # the host path IS the stated order
        assert np.array_equal(m._joint_log_likelihood(D["X"], R.Engine()), jll)    # and so is the engine's
        band = r["tol"].sum(axis=1)
        assert np.all(np.abs(m.predict_proba(D["X"]) - c["proba"]) <= band[:, None])
        assert np.array_equal(m.predict(D["X"]), np.argmax(jll, axis=1))
        lp = m.predict_log_proba(D["X"])
        # (lp = jll - logsumexp(jll) carries the rounding of numbers of jll's size: a few ulp of |jll|, absolute, in each exponent)
        assert np.all(np.abs(np.exp(lp).sum(axis=1) - 1.0) <= 4 * np.finfo(float).eps * np.maximum(1.0, np.abs(jll).max(axis=1)))
        assert m.score(D["X"], D["y"]) == np.mean(m.predict(D["X"]) == D["y"]) and isinstance(m.score(D["X"], D["y"]), np.float64)
        # a row alone gives the bits it gives inside the matrix
        assert np.array_equal(m._joint_log_likelihood(D["X"][-1:]), jll[-1:])
    # counts binarize as scikit-learn's binarize=0.0 does: the model of a count design is the model of its presence
    D = fx.designs[3]
    counted = M.BernoulliNB().fit(D["X"] * np.arange(1, D["p"] + 1), D["y"], R.Engine())
    assert np.array_equal(counted.feature_log_prob_, fitted[3].feature_log_prob_)
    assert np.array_equal(counted.predict_proba(D["X"] * 7), fitted[3].predict_proba(D["X"]))
    # equal likelihoods: class 0, probabilities one half each
    tie = M.BernoulliNB().fit(np.array([[0.0], [1.0], [0.0], [1.0]]), np.array([0, 0, 1, 1]), R.Engine())
    assert list(tie.predict(np.array([[0.0], [1.0]]))) == [0, 0] and np.all(np.abs(tie.predict_proba(np.array([[1.0]])) - 0.5) <= 1e-15)
    for bad in (dict(alpha=0.5), dict(force_alpha=False), dict(binarize=None), dict(binarize=1.0), dict(fit_prior=False),
                dict(class_prior=[0.5, 0.5]), dict(alpha=True)):
        with pytest.raises(ValueError):
            M.BernoulliNB(**bad)
    assert repr(M.BernoulliNB(alpha=1, force_alpha=True, binarize=0, fit_prior=True, class_prior=None)) == "BernoulliNB()"
    with pytest.raises(ValueError):
        M.BernoulliNB().fit(D["X"], D["y"] + 1, R.Engine())
    with pytest.raises(ValueError):
        fitted[3]._joint_log_likelihood(D["X"][:, :5])


def test_live_agreement_with_scikit_learn(fx, fitted):
    pytest.importorskip("sklearn")
    from sklearn.naive_bayes import BernoulliNB
    for D, m in zip(fx.designs, fitted):
        sk = BernoulliNB().fit(D["X"], D["y"])
        assert np.array_equal(sk.feature_log_prob_, m.feature_log_prob_) and np.array_equal(sk.class_log_prior_, m.class_log_prior_)
        tol = R.jll_tolerance(D["X"] != 0, sk.feature_log_prob_, sk.class_log_prior_)
        assert np.all(np.abs(sk._joint_log_likelihood(D["X"]) - m._joint_log_likelihood(D["X"])) <= tol)
        assert np.all(np.abs(sk.predict_log_proba(D["X"]) - m.predict_log_proba(D["X"])) <= tol.sum(axis=1)[:, None])


def test_nb_model_file_round_trips_three_ways(tmp_path, fx, fitted):
    """A shell-written NB package loads with joblib.load into a real sklearn.naive_bayes.BernoulliNB; to_sklearn() builds the same
    object; the reader that does not import scikit-learn gives model.BernoulliNB.  Equal predictions all round."""
    pytest.importorskip("sklearn")
    import warnings

    import joblib
    from phenotypeseeker_amd import model as M, skpickle
    D, m = fx.designs[3], fitted[3]
    shell = m.to_sklearn_shell()
    assert shell is not None, "no template for the installed scikit-learn: run tools/make_sklearn_shells.py"
    path = os.path.join(tmp_path, "nb.pkl")
    with open(path, "wb") as f:
        f.write(skpickle.dumps({"model": shell, "kmers": np.array(["ACGT"] * D["p"], dtype=object), "pca": False, "pred_scale": "binary"}))
    rng = np.random.default_rng(3)
    Xn = np.vstack([D["X"], (rng.random((50, D["p"])) < 0.5).astype(np.float64)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        sk = joblib.load(path)["model"]
        assert type(sk).__module__ == "sklearn.naive_bayes" and type(sk).__name__ == "BernoulliNB" and repr(sk) == repr(m)
        assert sk.get_params() == dict(alpha=1.0, force_alpha=True, binarize=0.0, fit_prior=True, class_prior=None)
        sk_pred, sk_proba, sk_jll = sk.predict(Xn), sk.predict_proba(Xn), sk._joint_log_likelihood(Xn)
    assert sk.__dict__.keys() == BernoulliNB_fitted_keys()
    for k in ("class_count_", "feature_count_", "feature_log_prob_", "class_log_prior_", "classes_"):
        assert np.array_equal(getattr(sk, k), getattr(m, k)) and getattr(sk, k).dtype == getattr(m, k).dtype, k
    tol = R.jll_tolerance(Xn != 0, m.feature_log_prob_, m.class_log_prior_)
    band = tol.sum(axis=1)
    assert np.all(np.abs(sk_jll - m._joint_log_likelihood(Xn)) <= tol)
    assert np.all(np.abs(sk_proba - m.predict_proba(Xn)) <= band[:, None])
    clear = np.abs(sk_jll[:, 0] - sk_jll[:, 1]) > band
    assert np.mean(~clear) <= 0.01 and np.array_equal(sk_pred[clear], m.predict(Xn)[clear])
    real = m.to_sklearn()                                     # the same object through the real constructor
    assert type(real) is type(sk)
    assert np.array_equal(real.predict(Xn), sk_pred) and np.array_equal(real.predict_proba(Xn), sk_proba)
    fast = skpickle.load_linear_package(path)                 # what `phenotypeseeker prediction` reads the file with
    assert fast is not None and isinstance(fast["model"], M.BernoulliNB)
    assert np.array_equal(fast["model"].predict(Xn), m.predict(Xn)) and np.array_equal(fast["model"].predict_proba(Xn), m.predict_proba(Xn))
    assert np.array_equal(fast["model"].predict(Xn, R.Engine()), m.predict(Xn))
    assert np.array_equal(fast["model"].predict(Xn)[clear], sk_pred[clear])
    # a BernoulliNB with other parameters is left to scikit-learn
    from sklearn.naive_bayes import BernoulliNB
    other = os.path.join(tmp_path, "other.pkl")
    import pickle
    with open(other, "wb") as f:
        pickle.dump({"model": BernoulliNB(alpha=0.5).fit(D["X"], D["y"]), "kmers": np.array(["ACGT"] * D["p"], dtype=object), "pca": False,
                     "pred_scale": "binary"}, f, protocol=2)
    assert skpickle.load_linear_package(other) is None


def BernoulliNB_fitted_keys():
    from sklearn.naive_bayes import BernoulliNB
    return BernoulliNB().fit(np.array([[0.0], [1.0]]), np.array([0, 1])).__dict__.keys()


OFF = "Only the logistic-regression classifier runs on the GPU engine, got 'NB' (SVM/RF/DT/NB are outside the accelerated path)."


def test_bc_nb_sits_behind_the_knob(tmp_path, monkeypatch):
    from test_host_modeling import _setup
    for knob in ("PSK_NB", "PSK_SVM", "PSK_DT", "PSK_RF"):
        monkeypatch.delenv(knob, raising=False)
    for flag in (None, "0"):
        if flag is not None:
            monkeypatch.setenv("PSK_NB", flag)
        with pytest.raises(SystemExit) as e:
            _setup(tmp_path, "ds_bonf", ["-bc", "NB"])
        assert str(e.value) == OFF
    for other in ("PSK_SVM", "PSK_DT", "PSK_RF"):             # no other knob opens NB
        monkeypatch.setenv(other, "1")
        with pytest.raises(SystemExit) as e:
            _setup(tmp_path, "ds_bonf", ["-bc", "NB"])
        assert str(e.value) == OFF
        monkeypatch.delenv(other)
    monkeypatch.setenv("PSK_NB", "1")
    M, _ = _setup(tmp_path, "ds_bonf", ["-bc", "NB"])
    assert (M.phenotypes.model_name_long, M.phenotypes.model_name_short) == ("Naive Bayes", "NB")
    assert M.phenotypes.binary_classifier == "NB"
    est, pname, grid = M.Input.phenotypes_to_analyse["Pheno"]._new_estimator()
    assert repr(est) == "BernoulliNB()" and pname is None and grid is None
    with pytest.raises(SystemExit) as e:
        _setup(tmp_path, "ds_bonf", ["-bc", "NB", "--pca"])
    assert "--pca" in str(e.value) and "-bc NB" in str(e.value)
    M, _ = _setup(tmp_path, "ds_bonf", ["-bc", "NB", "--real_counts"])
    assert M.phenotypes.binary_classifier == "NB" and M.phenotypes.real_counts
    for other in ("SVM", "DT", "RF"):                         # the knob opens NB alone
        with pytest.raises(SystemExit) as e:
            _setup(tmp_path, "ds_bonf", ["-bc", other])
        assert str(e.value) == OFF.replace("'NB'", "'%s'" % other)
    M, _ = _setup(tmp_path, "ds_bonf", [])                    # the default classifier is untouched by the knob
    assert M.phenotypes.model_name_short == "log_reg" and M.phenotypes.binary_classifier == "log"


def _host_run(tmp, monkeypatch, extra, scale=1):
    """machine_learning_modelling from the recorded Pheno_MLdf.csv of ds_omitB (-jt modelling) with the engine served by the
    restatement; `scale` multiplies the k-mer cells (a --real_counts design).  Returns (modeling module, phenotype, files)."""
    from helpers import GOLDEN
    from test_host_modeling import _args
    from phenotypeseeker_amd import modeling as M
    gd = os.path.join(GOLDEN, "ds_omitB")
    os.makedirs(tmp)
    os.chdir(tmp)
    with open(os.path.join(gd, "data.pheno")) as f, open("data.pheno", "w") as g:
        g.write(f.read())
    with open(os.path.join(gd, "Pheno_MLdf.csv")) as f, open("Pheno_MLdf.csv", "w") as g:
        g.write(f.readline())
        for line in f:
            c = line.rstrip("\n").split(",")
            g.write(",".join([c[0]] + [str(int(float(v)) * scale) for v in c[1:-2]] + c[-2:]) + "\n")
    monkeypatch.setenv("PSK_NB", "1")
    a = _args(["-jt", "modelling", "-bc", "NB", "--omit_B_correction", "--n_kmers", "100"] + extra)
    M.Input.reset()
    M.Input.get_input_data(a.inputfile, a.take_logs, a.mpheno)
    M.Input.Input_args(a.alphas, a.alpha_min, a.alpha_max, a.n_alphas, a.gammas, a.gamma_min, a.gamma_max, a.n_gammas,
                       a.min, a.max, a.kmer_length, a.cutoff, a.num_threads, a.pvalue, a.n_kmers, a.binary_classifier,
                       a.regressor, a.penalty, a.max_iter, a.tolerance, a.l1_ratio, a.n_splits_cv_outer, a.kernel,
                       a.n_iter, a.n_splits_cv_inner, a.testset_size, a.train_on_whole, a.logreg_solver, a.jump_to,
                       a.pca, a.real_counts, a.omit_B_correction, a.kmerDB)
    ph = M.Input.phenotypes_to_analyse["Pheno"]
    ph.machine_learning_modelling(R.Engine())
    names = ["summary_of_NB_analysis_Pheno.txt", "k-mers_and_coefficients_in_NB_model_Pheno.txt", "NB_model_Pheno.pkl"]
    for nm in names:
        assert os.path.exists(nm), nm
    return M, ph, [open(nm, "rb").read() for nm in names]


def test_summary_and_coefficient_files_of_a_host_run(tmp_path, monkeypatch):
    import joblib
    from phenotypeseeker_amd import model as Mo
    M, ph, (summary, coef, pkl) = _host_run(os.path.join(tmp_path, "presence"), monkeypatch, [])
    assert isinstance(ph.model_fitted, Mo.BernoulliNB)                # no search: the fitted estimator itself
    assert not os.path.exists("log_reg_model_Pheno.pkl")
    summary, coef = summary.decode(), coef.decode()
    for absent in ("Parameters:", "Grid scores", "Best parameters"):
        assert absent not in summary
    assert summary.startswith("\nModel predictions on samples:\nSample_ID Acutal_phenotype Predicted_phenotype\n")
    assert "Mean accuracy: " in summary and summary.rstrip("\n").endswith("### Outputting the model to a model file! ###")
    X, y, index, kmers = np.asarray(ph.ML["X"], dtype=np.float64), np.asarray(ph.ML["phenotype"]), ph.ML["index"], ph.ML["kmers"]
    block = summary.split("Predicted_phenotype\n")[1].split("\n\n")[0].splitlines()
    want = ph.model_fitted.predict(X)
    assert block == ["%s %s %s" % (nm, a, p) for nm, a, p in zip(index, y, want)]
    lines = coef.splitlines()
    assert lines[0] == "K-mer\tcoef._in_NB_model\tNo._of_samples_with_k-mer\tSamples_with_k-mer" and len(lines) == 1 + len(kmers)
    for j, ln in enumerate(lines[1:]):
        who = [index[i] for i in np.nonzero(X[:, j])[0]]
        assert ln == "%s\tNA\t%d\t| %s" % (kmers[j], len(who), " ".join(who)), j
    pkg = joblib.load("NB_model_Pheno.pkl")                          # `model` is the estimator, not a search around it
    assert type(pkg["model"]).__module__ == "sklearn.naive_bayes" and type(pkg["model"]).__name__ == "BernoulliNB"
    assert list(pkg["kmers"]) == list(kmers) and pkg["pred_scale"] == "binary" and pkg["pca"] is False
    assert np.array_equal(pkg["model"].feature_log_prob_, ph.model_fitted.feature_log_prob_)
    # the same samples as k-mer counts under --real_counts: the same model, the same files
    _, ph3, (summary3, coef3, pkl3) = _host_run(os.path.join(tmp_path, "counts"), monkeypatch, ["--real_counts"], scale=3)
    assert np.asarray(ph3.ML["X"]).max() == 3
    assert summary3.decode() == summary and coef3.decode() == coef and pkl3 == pkl


def test_abi_names_the_nb_entry_points():
    from phenotypeseeker_amd import _lib
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psk.h")) as f:
        header = f.read()
    assert "---- f8:" in header
    for name in ("psk_nb_fit", "psk_nb_jll"):
        assert name in _lib.exported_names()
        assert "int %s(psk_ctx *ctx" % name in header
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib._SIGNATURES[name][1]), name
