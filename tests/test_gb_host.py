"""CPU tests (-m "not gpu") of `-bc XGBC` / `-reg XGBR`: the NumPy restatement of the gradient-boosting contract (gb_restated.py,
what psk_gb_fit computes bit for bit) against scikit-learn's record (tests/golden/gb_kat.npz, tools/gen_gb_golden.py) on decisive
inputs within the recorded bounds; gb_exp against np.exp; model.GradientBoosting over a stand-in engine; the model file three
ways; the PSK_GB knob; the ABI; and the files of a host run."""
import os
from collections import OrderedDict

import numpy as np
import pytest

import gb_restated as R
from helpers import GOLDEN, ROOT

MARGIN, MIN_IMPURITY = 1e-9, 1e-12       # the decisive-input condition of tools/gen_gb_golden.py
LOSS_NAME = {0: "squared_error", 1: "log_loss"}


class Fixture:
    """The golden record and, per case, the restatement's fit of it (with the decisive-input diagnostic), computed once."""

    def __init__(self):
        g = np.load(os.path.join(GOLDEN, "gb_kat.npz"))
        self.g, self.rate = g, float(g["learning_rate"])
        self.designs = [dict(X=g["X_%d" % d].astype(np.float64), y=g["y_%d" % d], fold=g["fold_%d" % d]) for d in range(6)]
        self.cases = []
        for k in range(len(g["case_design"])):
            c = dict(k=k, design=int(g["case_design"][k]), fit_fold=int(g["case_fit_fold"][k]), loss=int(g["case_loss"][k]),
                     stages=int(g["case_stages"][k]), depth=int(g["case_depth"][k]))
            for name in ("staged", "predict", "proba", "init", "train_score", "d_ref", "bound"):
                c[name] = g["%s_%d" % (name, k)]
            D = self.designs[c["design"]]
            c["in_bag"] = D["fold"] != c["fit_fold"]
            c["init_raw"] = R.init_raw(D["y"], c["in_bag"], c["loss"])
            c["fit"] = R.fit_one(D["X"], D["y"], c["in_bag"], c["loss"], c["stages"], self.rate, c["depth"], c["init_raw"], diagnose=True)
            self.cases.append(c)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def test_the_fixture_holds_what_the_tests_need(fx):
    g = fx.g
    assert str(g["sklearn_version"]) == "1.7.2" and fx.rate == 0.1
    assert len(fx.cases) == 26 and [c["loss"] for c in fx.cases].count(1) == 13
    assert {(c["stages"], c["depth"]) for c in fx.cases} == {(30, 3), (10, 1), (10, 4)}
    for loss in (0, 1):
        kept, skipped = list(g["seeds_kept_%d" % loss]), list(g["seeds_skipped_%d" % loss])
        assert len(kept) == 3 and max(kept) < 16 and sorted(kept + skipped) == list(range(max(kept) + 1))
    for D in fx.designs:
        assert D["X"].shape == (96, 40) and set(np.unique(D["X"])) == {0.0, 1.0} and set(np.unique(D["fold"])) == {0, 1, 2}
    for c in fx.cases:
        nb = int(c["in_bag"].sum())
        assert c["staged"].shape == (c["stages"], nb) and c["predict"].shape == (nb,) and c["train_score"].shape == (c["stages"],)
        # the bound is made of scikit-learn's own spread and the format's precision, never of the code under test
        assert float(c["bound"]) == 8.0 * max(float(c["d_ref"]), 2.0 ** -52 * float(np.abs(c["staged"]).max()))
        assert float(c["bound"]) < 1e-13


def test_every_golden_case_is_decisive(fx):
    for c in fx.cases:
        assert c["fit"]["margin"] >= MARGIN and c["fit"]["min_impurity"] >= MIN_IMPURITY, (c["k"], c["fit"]["margin"], c["fit"]["min_impurity"])


def test_restatement_is_within_the_bound_of_scikit_learn(fx):
    for c in fx.cases:
        f, tr, bound = c["fit"], c["in_bag"], float(c["bound"])
        assert abs(c["init_raw"] - float(c["init"])) <= bound, c["k"]
        err = float(np.abs(f["staged"][:, tr] - c["staged"]).max())
        assert err <= bound, (c["k"], err, bound)
        raw = f["raw"][tr]
        if c["loss"] == 0:
            assert np.all(np.abs(raw - c["predict"]) <= bound), c["k"]
            score = np.array([np.mean((fx.designs[c["design"]]["y"][tr] - s[tr]) ** 2) for s in f["staged"]])
        else:
            from phenotypeseeker_amd.model_gb import expit
            assert np.all(np.abs(np.column_stack([1 - expit(raw), expit(raw)]) - c["proba"]) <= bound), c["k"]
            assert np.all(np.abs(raw) > bound) and np.array_equal((raw >= 0).astype(np.int64), c["predict"].astype(np.int64)), c["k"]
            y = fx.designs[c["design"]]["y"][tr]
            score = np.array([2.0 * np.mean(np.logaddexp(0.0, s[tr]) - y * s[tr]) for s in f["staged"]])
        # (a mean of n losses whose raw values are within the bound: the derivative of either loss in raw is below 2 max|y - raw|)
        assert np.all(np.abs(score - c["train_score"]) <= 1e-12), c["k"]


def test_gb_exp_is_within_its_recorded_distance_of_np_exp(fx):
    rng = np.random.default_rng(5)
    x = np.concatenate([np.linspace(-50.0, 50.0, 400001), rng.uniform(-50.0, 50.0, 400000), rng.normal(0.0, 2.0, 200000)])
    ref = np.exp(x)
    ulp = float(np.max(np.abs(R.gb_exp(x) - ref) / np.spacing(ref)))
    assert ulp <= float(fx.g["gb_exp_ulp"]) <= 1.0, ulp
    assert R.gb_exp(0.0) == 1.0 and R.gb_exp(1000.0) == R.gb_exp(708.0) and np.isfinite(R.gb_exp(708.0)) and R.gb_exp(-1000.0) > 0.0
    assert R.gb_expit(0.0) == 0.5 and R.gb_expit(-1000.0) > 0.0 and R.gb_expit(1000.0) == 1.0


def test_the_headers_gb_exp_on_the_host_equals_numpys_mirror_bit_for_bit(tmp_path):
    """csrc/solver_gb_math.h compiled for the host (no fused multiply-add, as the library's unit) against gb_restated.gb_exp: the
    mirror is line for line.  (The device's evaluation is held to the same mirror by every == of test_gpu_gb.py.)"""
    import subprocess
    from test_gz_plan_host import _hipcc
    exe = os.path.join(tmp_path, "gb_exp_check")
    subprocess.run([_hipcc(), "-std=c++17", "-O3", "-ffp-contract=off", "-Wall", "-x", "c++", os.path.join(ROOT, "tests", "gb_exp_check.cpp"),
                    "-o", exe], check=True)
    rng = np.random.default_rng(9)
    x = np.concatenate([np.linspace(-60.0, 60.0, 100001), rng.normal(0.0, 3.0, 100000), rng.uniform(-750.0, 750.0, 20000),
                        [0.0, -0.0, 708.0, -708.0, 709.0, -1e300, 1e300, 5e-324, 0.5 * np.log(2.0), -0.5 * np.log(2.0)]])
    x.tofile(os.path.join(tmp_path, "x.bin"))
    subprocess.run([exe, os.path.join(tmp_path, "x.bin"), os.path.join(tmp_path, "y.bin")], check=True, timeout=60)
    got = np.fromfile(os.path.join(tmp_path, "y.bin")).reshape(-1, 2)
    assert got.shape == (len(x), 2)
    assert np.array_equal(got[:, 0].view(np.uint64), R.gb_exp(x).view(np.uint64))
    assert np.array_equal(got[:, 1].view(np.uint64), R.gb_expit(x).view(np.uint64))


def test_two_level_sum_is_sequential_within_and_over_words():
    rng = np.random.default_rng(1)
    v = rng.normal(0.0, 1.0, 192) * 10.0 ** rng.integers(-8, 8, 192)
    want = 0.0
    for w in range(3):
        part = 0.0
        for s in range(64):
            part += v[w * 64 + s]
        want += part
    assert R.two_level_sum(v) == want


def _estimator(fx, k):
    from phenotypeseeker_amd import model as M
    c = fx.cases[k]
    D = fx.designs[c["design"]]
    tr = c["in_bag"]
    y = D["y"][tr] if c["loss"] == 0 else D["y"][tr].astype(np.int64)
    m = M.GradientBoosting(LOSS_NAME[c["loss"]], n_estimators=c["stages"], max_depth=c["depth"]).fit(D["X"][tr], y, R.Engine())
    return c, D, tr, y, m


@pytest.mark.parametrize("k", [1, 4, 13, 17])
def test_estimator_over_the_stand_in_engine_reproduces_the_restatement(fx, k):
    """A fit on the in-bag rows alone is the masked fit on all rows: a word of 64 samples holds other samples, so the two-level
    sums differ in order -- equal within the bound, and bit-equal when no row is held out."""
    c, D, tr, y, m = _estimator(fx, k)
    f = c["fit"]
    assert m.init_raw_ == c["init_raw"] and m.n_estimators_ == c["stages"]
    staged = m.staged_raw(D["X"][tr])
    if c["fit_fold"] == -1:
        assert np.array_equal(m.node_count_, f["node_count"]) and np.array_equal(m.nodes_, f["nodes"])
        assert np.array_equal(m.value_, f["value"]) and np.array_equal(m.impurity_, f["impurity"])
        assert np.array_equal(staged, f["staged"]) and np.array_equal(m.raw(D["X"]), f["raw"])
        assert np.array_equal(m.feature_importances_, R.feature_importances(f, 40))
    else:
        assert np.abs(staged - f["staged"][:, tr]).max() <= float(c["bound"])
    assert np.array_equal(m.raw(D["X"][tr], R.Engine()), m.raw(D["X"][tr]))          # the device's order is the host's
    assert np.abs(m.train_score_ - c["train_score"]).max() <= 1e-12
    imp = m.feature_importances_
    assert imp.shape == (40,) and np.all(imp >= 0) and abs(imp.sum() - 1.0) < 1e-12
    if c["loss"] == 1:
        assert np.array_equal(m.predict(D["X"][tr]), c["predict"].astype(np.int64)) and m.score(D["X"][tr], y) == np.mean(c["predict"] == y)
        assert np.abs(m.predict_proba(D["X"][tr]) - c["proba"]).max() <= float(c["bound"])
        assert repr(m) == ("GradientBoostingClassifier(max_depth=%d, n_estimators=%d)" % (c["depth"], c["stages"])).replace("max_depth=3, ", "")
    else:
        assert np.abs(m.predict(D["X"][tr]) - c["predict"]).max() <= float(c["bound"])
        assert repr(m).startswith("GradientBoostingRegressor(")


def test_estimator_refuses_what_the_engine_does_not_fit():
    from phenotypeseeker_amd import model as M
    assert repr(M.GradientBoosting("log_loss")) == "GradientBoostingClassifier()" and repr(M.GradientBoosting("squared_error")) == "GradientBoostingRegressor()"
    for kw in (dict(loss="huber"), dict(loss="log_loss", max_depth=11), dict(loss="log_loss", max_depth=None), dict(loss="log_loss", n_estimators=0),
               dict(loss="log_loss", n_estimators=1001), dict(loss="squared_error", learning_rate=0.0), dict(loss="squared_error", learning_rate=float("nan"))):
        with pytest.raises(ValueError):
            M.GradientBoosting(**kw)
    with pytest.raises(ValueError):
        M.GradientBoosting("log_loss").fit(np.zeros((4, 2)), np.array([0, 1, 2, 1]), R.Engine())


@pytest.mark.parametrize("k", [0, 13])
def test_model_file_round_trips(tmp_path, fx, k):
    """The package `modeling` writes loads with joblib.load into a real scikit-learn estimator whose predictions are ours within
    the bound; `prediction` reads the same file and predicts what this package's estimator predicts."""
    pytest.importorskip("sklearn")
    import joblib
    from phenotypeseeker_amd import model as M, model_gb, prediction as P, skpickle
    c, D, tr, y, m = _estimator(fx, k)
    X, bound = D["X"], float(c["bound"])
    assert m.to_sklearn_shell() is None
    kmers = np.array(["ACGTACGTACGTA"] * 40, dtype=object)
    path = os.path.join(tmp_path, "gb.pkl")
    joblib.dump({"model": m.to_sklearn(), "kmers": kmers, "pca": False, "pred_scale": "binary" if c["loss"] else "continuous"}, path)
    sk = joblib.load(path)["model"]
    name = "GradientBoostingClassifier" if c["loss"] else "GradientBoostingRegressor"
    assert type(sk).__module__ == "sklearn.ensemble._gb" and type(sk).__name__ == name and repr(sk) == repr(m)
    from sklearn import ensemble
    ref = getattr(ensemble, name)(n_estimators=2).fit(X[:20], y[:20])
    assert sk.__dict__.keys() == ref.__dict__.keys()
    assert sk.init_.__dict__.keys() == ref.init_.__dict__.keys() and sk.estimators_[0, 0].__dict__.keys() == ref.estimators_[0, 0].__dict__.keys()
    assert sk.estimators_.shape == (c["stages"], 1) and sk.n_estimators_ == c["stages"] and np.array_equal(sk.train_score_, m.train_score_)
    assert type(sk.estimators_[0, 0]).__name__ == "DecisionTreeRegressor" and type(sk._loss).__name__ == type(ref._loss).__name__
    assert np.abs(sk.predict(X) - m.predict(X)).max() <= bound if c["loss"] == 0 else np.array_equal(sk.predict(X), m.predict(X))
    raw = sk.decision_function(X) if c["loss"] else sk.predict(X)
    assert np.abs(raw - m.raw(X)).max() <= bound
    assert np.abs(np.array(list(sk.staged_decision_function(X) if c["loss"] else sk.staged_predict(X))).reshape(c["stages"], -1) - m.staged_raw(X)).max() <= bound
    if c["loss"]:
        assert np.abs(sk.predict_proba(X) - m.predict_proba(X)).max() <= bound
    assert np.abs(sk.feature_importances_ - m.feature_importances_).max() <= 1e-12
    assert skpickle.load_linear_package(path) is None                    # joblib's file: `prediction` takes joblib.load
    back = model_gb.from_sklearn(sk)
    assert isinstance(back, M.GradientBoosting) and np.array_equal(back.raw(X), m.raw(X)) and np.array_equal(back.nodes_, m.nodes_)
    assert model_gb.from_sklearn(getattr(ensemble, name)(n_estimators=2, subsample=0.5, init="zero").fit(X[:20], y[:20])) is None
    # `prediction` on the same file (no context: the host's order, which is the device's)
    os.chdir(tmp_path)
    P.Input.reset()
    names = ["S%03d" % i for i in range(len(X))]
    P.Input.samples = OrderedDict((nm, P.Samples(nm, nm + ".fa")) for nm in names)
    ph = P.Phenotypes.from_inputfile("Pheno %s" % path)
    ph.matrix[:, :] = X
    ph.predict(None)
    out = open("predictions_Pheno.txt").read().splitlines()
    pred = m.predict(X)
    if c["loss"]:
        assert out[0] == "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class"
        proba = m.predict_proba(X)
        assert out[1:] == ["%s\t%s\t%s" % (nm, str(pr), str(round(pp[1], 2))) for nm, pr, pp in zip(names, pred, proba)]
    else:
        assert out[0] == "Sample_ID\tpredicted_phenotype" and out[1:] == ["%s\t%s" % (nm, str(pr)) for nm, pr in zip(names, pred)]
    P.Input.reset()


# ---- `modeling -bc XGBC` / `-reg XGBR` ---------------------------------------------------------------------------------------
OFF_BC = "Only the logistic-regression classifier runs on the GPU engine, got 'XGBC' (SVM/RF/DT/NB are outside the accelerated path)."
OFF_REG = "Only the linear (Lasso) regressor runs on the GPU engine, got 'XGBR'."


def _input_args(tmp_path, extra, binary):
    from test_host_modeling import _args
    from phenotypeseeker_amd import modeling as M
    os.chdir(tmp_path)
    with open("d.pheno", "w") as f:
        f.write("ID\tAddr\tMIC\n")
        for i in range(12):
            f.write("S%d\ts%d.fa\t%s\n" % (i, i, i % 2 if binary else "%.2f" % (0.25 * i + 0.5)))
    a = _args(extra)
    M.Input.reset()
    M.Input.get_input_data("d.pheno", a.take_logs, a.mpheno)
    M.Input.Input_args(a.alphas, a.alpha_min, a.alpha_max, a.n_alphas, a.gammas, a.gamma_min, a.gamma_max, a.n_gammas,
                       a.min, a.max, a.kmer_length, a.cutoff, a.num_threads, a.pvalue, a.n_kmers, a.binary_classifier,
                       a.regressor, a.penalty, a.max_iter, a.tolerance, a.l1_ratio, a.n_splits_cv_outer, a.kernel,
                       a.n_iter, a.n_splits_cv_inner, a.testset_size, a.train_on_whole, a.logreg_solver, a.jump_to,
                       a.pca, a.real_counts, a.omit_B_correction, a.kmerDB)
    return M


def test_both_flags_sit_behind_the_knob(tmp_path, monkeypatch):
    for knob in ("PSK_GB", "PSK_NB", "PSK_SVM", "PSK_DT", "PSK_RF", "PSK_PCA", "PSK_ENET"):
        monkeypatch.delenv(knob, raising=False)
    for flag in (None, "0"):
        if flag is not None:
            monkeypatch.setenv("PSK_GB", flag)
        for extra, binary, off in ((["-bc", "XGBC"], True, OFF_BC), (["-reg", "XGBR"], False, OFF_REG)):
            with pytest.raises(SystemExit) as e:
                _input_args(tmp_path, extra, binary)
            assert str(e.value) == off
    monkeypatch.setenv("PSK_NB", "1")                                   # no other knob opens them
    with pytest.raises(SystemExit) as e:
        _input_args(tmp_path, ["-bc", "XGBC"], True)
    assert str(e.value) == OFF_BC
    monkeypatch.delenv("PSK_NB")
    monkeypatch.setenv("PSK_GB", "1")
    M = _input_args(tmp_path, ["-bc", "XGBC", "--penalty", "L1+L2", "-cv2", "3"], True)     # --penalty and -cv2 play no part
    assert (M.phenotypes.model_name_long, M.phenotypes.model_name_short) == ("gradient boosting classifier", "GBC")
    assert M.phenotypes.gradient_boosting and M.phenotypes.binary_classifier == "XGBC"
    est, pname, grid = M.Input.phenotypes_to_analyse["MIC"]._new_estimator()
    assert repr(est) == "GradientBoostingClassifier()" and pname is None and grid is None
    M = _input_args(tmp_path, ["-reg", "XGBR"], False)
    assert (M.phenotypes.model_name_long, M.phenotypes.model_name_short) == ("gradient boosting regressor", "GBR")
    est, pname, grid = M.Input.phenotypes_to_analyse["MIC"]._new_estimator()
    assert repr(est) == "GradientBoostingRegressor()" and pname is None and grid is None
    for extra, binary, flag in ((["-bc", "XGBC"], True, "-bc XGBC"), (["-reg", "XGBR"], False, "-reg XGBR")):
        for option in ("--pca", "--real_counts"):
            with pytest.raises(SystemExit) as e:
                _input_args(tmp_path, extra + [option], binary)
            assert option in str(e.value) and flag in str(e.value) and "0/1 presence matrix only" in str(e.value)
    # the knob opens nothing else, and a flag of the other scale is not looked at (as in the reference)
    with pytest.raises(SystemExit) as e:
        _input_args(tmp_path, ["-bc", "NB"], True)
    assert str(e.value) == OFF_BC.replace("'XGBC'", "'NB'")
    M = _input_args(tmp_path, [], True)
    assert M.phenotypes.model_name_short == "log_reg" and not M.phenotypes.gradient_boosting
    M = _input_args(tmp_path, ["-bc", "XGBC"], False)
    assert M.phenotypes.model_name_short == "linreg" and not M.phenotypes.gradient_boosting


def test_abi_names_the_gb_entry_points():
    from phenotypeseeker_amd import _lib
    with open(os.path.join(ROOT, "include", "psk.h")) as f:
        header = f.read()
    assert "---- f16:" in header and "#define PSK_GB_NODE_CAP(max_depth)" in header
    for name in ("psk_gb_fit", "psk_gb_decision"):
        assert name in _lib.exported_names()
        assert "int %s(psk_ctx *ctx" % name in header
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib._SIGNATURES[name][1]), name
    assert hasattr(_lib.load(), "psk_gb_fit") and hasattr(_lib.load(), "psk_gb_decision")


def _host_run(tmp, monkeypatch, dataset, pheno, flags, short):
    """machine_learning_modelling from a recorded <pheno>_MLdf.csv (-jt modelling) with the engine served by the restatement."""
    from test_host_modeling import _args
    from phenotypeseeker_amd import modeling as M
    gd = os.path.join(GOLDEN, dataset)
    os.makedirs(tmp)
    os.chdir(tmp)
    for nm in ("data.pheno", pheno + "_MLdf.csv"):
        with open(os.path.join(gd, nm)) as f, open(nm, "w") as g:
            g.write(f.read())
    monkeypatch.setenv("PSK_GB", "1")
    a = _args(["-jt", "modelling", "--omit_B_correction", "--n_kmers", "100"] + flags)
    M.Input.reset()
    M.Input.get_input_data(a.inputfile, a.take_logs, a.mpheno)
    M.Input.Input_args(a.alphas, a.alpha_min, a.alpha_max, a.n_alphas, a.gammas, a.gamma_min, a.gamma_max, a.n_gammas,
                       a.min, a.max, a.kmer_length, a.cutoff, a.num_threads, a.pvalue, a.n_kmers, a.binary_classifier,
                       a.regressor, a.penalty, a.max_iter, a.tolerance, a.l1_ratio, a.n_splits_cv_outer, a.kernel,
                       a.n_iter, a.n_splits_cv_inner, a.testset_size, a.train_on_whole, a.logreg_solver, a.jump_to,
                       a.pca, a.real_counts, a.omit_B_correction, a.kmerDB)
    ph = M.Input.phenotypes_to_analyse[pheno]
    ph.machine_learning_modelling(R.Engine())
    names = ["summary_of_%s_analysis_%s.txt" % (short, pheno), "k-mers_and_coefficients_in_%s_model_%s.txt" % (short, pheno),
             "%s_model_%s.pkl" % (short, pheno)]
    for nm in names:
        assert os.path.exists(nm), nm
    return ph, open(names[0]).read(), open(names[1]).read(), names[2]


@pytest.mark.parametrize("dataset,pheno,flags,short", [("ds_omitB", "Pheno", ["-bc", "XGBC"], "GBC"), ("ds_cont", "MIC", ["-reg", "XGBR"], "GBR")])
def test_summary_and_coefficient_files_of_a_host_run(tmp_path, monkeypatch, dataset, pheno, flags, short):
    pytest.importorskip("sklearn")
    import joblib
    from phenotypeseeker_amd import model as Mo
    ph, summary, coef, pkl = _host_run(os.path.join(tmp_path, "run"), monkeypatch, dataset, pheno, flags, short)
    m = ph.model_fitted
    assert isinstance(m, Mo.GradientBoosting) and m.n_estimators_ == 100                 # no search: the fitted estimator itself
    name = "GradientBoostingClassifier" if short == "GBC" else "GradientBoostingRegressor"
    assert summary.startswith("Parameters:\n%s()\n\n\nModel predictions on samples:\nSample_ID Acutal_phenotype Predicted_phenotype\n" % name)
    assert "Grid scores" not in summary and "Best parameters" not in summary
    assert summary.rstrip("\n").endswith("### Outputting the model to a model file! ###")
    assert ("Mean accuracy: " in summary) if short == "GBC" else ("Mean squared error: " in summary and "The coefficient of determination: " in summary)
    X, y, index, kmers = np.asarray(ph.ML["X"], dtype=np.float64), np.asarray(ph.ML["phenotype"]), ph.ML["index"], ph.ML["kmers"]
    block = summary.split("Predicted_phenotype\n")[1].split("\n\n")[0].splitlines()
    assert block == ["%s %s %s" % (nm, a, p) for nm, a, p in zip(index, y, m.predict(X))]
    want = R.fit_one(X, y, np.ones(len(y), dtype=bool), int(short == "GBC"), 100, 0.1, 3, R.init_raw(y, np.ones(len(y), dtype=bool), int(short == "GBC")))
    assert np.array_equal(m.raw(X), want["raw"])
    lines = coef.splitlines()
    assert lines[0] == "K-mer\tcoef._in_%s_model\tNo._of_samples_with_k-mer\tSamples_with_k-mer" % short and len(lines) == 1 + len(kmers)
    imp = m.feature_importances_
    assert np.array_equal(imp, R.feature_importances(want, len(kmers))) and imp.max() > 0
    for j, ln in enumerate(lines[1:]):
        who = [index[i] for i in np.nonzero(X[:, j])[0]]
        cells = ln.split("\t")
        assert cells[0] == kmers[j] and float(cells[1]) == imp[j] and cells[2] == str(len(who)) and cells[3] == "| " + " ".join(who), j
    pkg = joblib.load(pkl)                                              # `model` is the estimator, not a search around it
    assert type(pkg["model"]).__name__ == name and list(pkg["kmers"]) == list(kmers) and pkg["pca"] is False
    assert pkg["pred_scale"] == ("binary" if short == "GBC" else "continuous")
    assert np.abs((pkg["model"].decision_function(X) if short == "GBC" else pkg["model"].predict(X)) - m.raw(X)).max() <= 1e-13
