"""GPU tests (-m gpu) of psk_logreg_l1_free_fit -- L1 logistic regression with a free intercept, the PI = false instances of
logreg_newglmnet_kernel (csrc/solver.hip) and logreg_newglmnet_bits_kernel (csrc/solver_l1_bits.h) -- on every route that
psk_logreg_l1_fit has: the float kernel in the placements of its per-fit state, the bit-packed kernel with the Gram matrix in
global memory, as four-wave register arrays, as one-wave arrays and with the LDS Gram block, at 16 / 32 / 64 sample words.
Yardstick: l1_free_restated.free_arbiter, certified on the CPU (tests/test_l1_free_host.py); bounds: those of
l1_float_cases.judge_logit / judge_tight restated for the free objective.  Then `modeling --logreg_solver saga` behind
PSK_L1_SAGA=1 and `prediction` of its model file.  Every test prints what it measured over its bound."""
import os
import time

import numpy as np
import pytest

import l1_float_cases as L
import l1_free_restated as F

pytestmark = pytest.mark.gpu

np.seterr(over="ignore")        # exp() of a large margin overflows to inf on purpose: 1 / (1 + inf) = 0
EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


def _fit(ctx, name, tol, max_iter):
    X, y, fold, fp, ff = F.case_data(name)
    t0 = time.perf_counter()
    r = ctx.logreg_l1_free_fit(X, y, fold, fp, ff, tol=tol, max_iter=max_iter)
    return r, time.perf_counter() - t0


@pytest.mark.parametrize("name", F.FLOAT_CASES)
def test_the_float_kernel_reaches_the_certified_optimum_at_the_reference_tolerance(ctx, name):
    """tol = 1e-4, max_iter = 1000: fewer than 200 Newton steps, the stop rule for the true gradient (slack 1.5), the objective
    within [1 - 1e-9, 1.01] of the arbiter's."""
    X, y, fold, fp, ff = F.case_data(name)
    assert L.route_is_float(name) and L.placement(*X.shape) == L.CASES[name]["place"]
    arbs = F.certified(name)
    assert all(a["kkt"] < F.KKT_MAX for a in arbs)
    (coef, icpt, iters), secs = _fit(ctx, name, 1e-4, 1000)
    stop, gap, steps = F.judge_logit(name, X, y, fold, fp, ff, coef, icpt, iters, arbs)
    print("%s %dx%d placement %s, %d fits: stop-rule violation / bound %.3g, objective gap / 1 %% %.3g, Newton steps %d..%d, "
          "%.2f s on the device" % (name, X.shape[0], X.shape[1], L.CASES[name]["place"], len(fp), stop, gap, iters.min(), steps, secs))


@pytest.mark.parametrize("name", [n for n in F.FLOAT_CASES + (F.SEAM_CASE,) if L.CASES[n]["tight"]])
def test_tight_tolerance_lands_on_the_certified_coefficients(ctx, name):
    """tol = 1e-12, max_iter = 5000: the same support with exact zeros off it (the constant column's pattern among them),
    pattern sums and intercept rtol 1e-6, the training predictor rtol 1e-6 / atol 1e-12, the objective rel 1e-12.
    C-bin-4096 is the bit-packed side of the seam at 4,096 samples, C-bin (4,097 rows) the float side."""
    X, y, fold, fp, ff = F.case_data(name)
    assert L.route_is_float(name) == (name != F.SEAM_CASE)
    (coef, icpt, iters), secs = _fit(ctx, name, 1e-12, 5000)
    ce, le, oe, steps = F.judge_tight(name, X, y, fold, fp, ff, coef, icpt, iters, F.certified(name))
    print("%s tol 1e-12: coefficient error / 1e-6 %.3g, predictor error / bound %.3g, objective error / 1e-12 %.3g, Newton steps "
          "%d..%d, %.2f s" % (name, ce, le, oe, iters.min(), steps, secs))


def test_the_seam_at_4096_samples(ctx):
    """C-bin-4096 (bit-packed) against C-bin (float) at the tight tolerance, one row apart: adding a row adds a non-negative
    loss, and the smaller problem's optimum is a point of the larger one -- opt(4096) <= opt(4097) <= opt(4096) + C loss of row
    4096 at the smaller optimum (test_gpu_l1_float.py::test_the_hand_over_at_4096_samples, for the free objective)."""
    X, y, fold, fp, ff = F.case_data("C-bin")
    assert L.route_is_float("C-bin") and not L.route_is_float(F.SEAM_CASE)
    (c7, b7, _), _ = _fit(ctx, "C-bin", 1e-12, 5000)
    (c6, b6, _), _ = _fit(ctx, F.SEAM_CASE, 1e-12, 5000)
    ypm = 2.0 * y - 1.0
    o7 = F.objectives(X, ypm, fold, fp, ff, c7, b7)
    o6 = F.objectives(X[:4096], ypm[:4096], fold[:4096], fp, ff, c6, b6)
    last = fp * np.logaddexp(0.0, -ypm[4096] * (c6 @ X[4096].astype(np.float64) + b6))
    for j in range(len(fp)):
        assert o6[j] * (1 - 1e-12) <= o7[j] <= (o6[j] + last[j]) * (1 + 1e-12), (j, o6[j], o7[j], last[j])
    print("objective(4097) - objective(4096) over the last row's loss: %s" % ((o7 - o6) / last).round(4).tolist())


FORMS = (("gram-global", None), ("four-wave arrays", "PSK_NO_GRAM_GLOBAL"), ("one-wave arrays", "PSK_NO_CD_REGS"))


@pytest.mark.parametrize("n", [40, 130, 700, 2048, 4096])
def test_the_forms_of_the_bit_packed_descent_agree(ctx, n, monkeypatch):
    """The design of test_gpu_parity.py::test_l1_logreg_three_forms_of_the_descent_agree (p = 250 > 192: the Gram matrix in
    global memory by default, with its accelerator; PSK_NO_GRAM_GLOBAL=1 the four-wave register arrays; PSK_NO_CD_REGS=1 the
    one-wave arrays) and its first 40 columns (the LDS Gram block), five fits each; n meets the 16-, 32- and 64-word
    instances.  Every form twice, bit-identical; every form meets the stop rule; the objectives agree to rtol 1e-5; up to
    700 samples every form is judged against the arbiter as well.

    Measured on an MI355X, the largest objective gap over the arbiter's at n = 130: Gram-global 4.5e-6, the array forms 2.2e-6."""
    for knob in ("PSK_NO_GRAM", "PSK_NO_GRAM_GLOBAL", "PSK_NO_CD_REGS", "PSK_GG_MIN_P1", "PSK_FORCE_WMREG"):
        monkeypatch.delenv(knob, raising=False)
    for p, forms in ((250, FORMS), (40, (("lds gram block", None),))):
        X, y, fold, fp, ff = F.bits_design(n, p)
        assert not F.one_class_fits(y, fold, ff)
        arbs = F.bits_certified(n, p) if n <= 700 else None
        assert arbs is None or all(a["kkt"] < F.KKT_MAX for a in arbs)
        ypm = 2.0 * y - 1.0
        objs = {}
        for tag, env in forms:
            if env:
                monkeypatch.setenv(env, "1")
            t0 = time.perf_counter()
            r = ctx.logreg_l1_free_fit(X, y, fold, fp, ff, tol=1e-4, max_iter=1000)
            secs = time.perf_counter() - t0
            r2 = ctx.logreg_l1_free_fit(X, y, fold, fp, ff, tol=1e-4, max_iter=1000)
            if env:
                monkeypatch.delenv(env)
            assert all(np.array_equal(u, v) for u, v in zip(r, r2)), (tag, p)
            stop, gap, steps = F.judge_logit("%s %dx%d" % (tag, n, p), X, y, fold, fp, ff, r[0], r[1], r[2], arbs)
            objs[tag] = F.objectives(X, ypm, fold, fp, ff, r[0], r[1])
            print("%s %dx%d: stop-rule violation / bound %.3g, objective gap / 1 %% %.3g, Newton steps %s, intercepts %s, %.2f s"
                  % (tag, n, p, stop, gap, r[2].tolist(), r[1].round(4).tolist(), secs))
        first = forms[0][0]
        for tag, _ in forms[1:]:
            assert np.allclose(objs[first], objs[tag], rtol=1e-5, atol=0), (tag, objs[first], objs[tag])


def test_a_training_fold_of_one_class_is_refused(ctx):
    """b runs off to infinity: no minimiser.  PSK_EINVAL naming the fit; the context stays usable."""
    from phenotypeseeker_amd.engine import PskError
    X, y, fold, fp, ff = F.case_data("A-tail-65x3")
    fold1 = np.where(y == 1, 0, 1).astype(np.int32)       # holding fold 0 out leaves class 0 only
    with pytest.raises(PskError) as e:
        ctx.logreg_l1_free_fit(X, y, fold1, fp[:3], np.array([-1, 2, 0], np.int32))         # (no row is of fold 2)
    assert e.value.code == EINVAL and "fit 2" in str(e.value) and "one class" in str(e.value)
    (coef, icpt, iters), _ = _fit(ctx, "A-tail-65x3", 1e-4, 1000)
    F.judge_logit("after the refusal", X, y, fold, fp, ff, coef, icpt, iters, F.certified("A-tail-65x3"))


def test_the_penalised_entry_point_is_untouched_by_the_free_calls(ctx):
    """psk_logreg_l1_fit on case A before and after free calls on the float and the bit-packed route, in one process:
    bit-identical outputs; and the two entry points do not return the same model."""
    X, y, fold, fp, ff = L.case_data("A")
    before = ctx.logreg_l1_fit(X, y, fold, fp, ff, tol=1e-4, max_iter=1000)
    free = ctx.logreg_l1_free_fit(X, y, fold, fp, ff, tol=1e-4, max_iter=1000)
    Xb, yb, foldb, fpb, ffb = F.bits_design(130)
    ctx.logreg_l1_free_fit(Xb, yb, foldb, fpb, ffb, tol=1e-4, max_iter=1000)
    after = ctx.logreg_l1_fit(X, y, fold, fp, ff, tol=1e-4, max_iter=1000)
    for u, v, what in zip(before, after, ("coef", "intercept", "Newton steps")):
        assert np.array_equal(u, v), what
    assert not np.array_equal(before[1], free[1])
    ypm = 2.0 * y - 1.0
    # in the free objective the free optimum lies below liblinear's point
    assert np.all(F.objectives(X, ypm, fold, fp, ff, free[0], free[1]) < F.objectives(X, ypm, fold, fp, ff, before[0], before[1]))


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


def test_cli_end_to_end(tmp_path, monkeypatch):
    """PSK_L1_SAGA=1 phenotypeseeker modeling -ls saga on the small dataset fixture: refused without the knob in today's words;
    with it the files are named as the liblinear run's, the summary's Parameters line names saga, the model's intercept differs
    from the liblinear run's (the coefficient file itself has no intercept line: the intercept is read from the .pkl), and
    `prediction` of the written .pkl reproduces the summary's predictions."""
    from helpers import load_dataset
    from test_host_modeling import _write_dataset
    from phenotypeseeker_amd import skpickle
    ds = load_dataset("ds_omitB")
    names = ["summary_of_log_reg_analysis_Pheno.txt", "k-mers_and_coefficients_in_log_reg_model_Pheno.txt", "log_reg_model_Pheno.pkl"]
    base = ["modeling", "data.pheno", "--omit_B_correction", "--n_kmers", "100"]
    icpt, wds = {}, {}
    for solver in ("liblinear", "saga"):
        wd = tmp_path / solver
        wd.mkdir()
        _write_dataset(ds, str(wd))
        argv = base + (["-ls", "saga"] if solver == "saga" else [])
        if solver == "saga":
            monkeypatch.delenv("PSK_L1_SAGA", raising=False)
            with pytest.raises(SystemExit) as e:
                _run(wd, argv)
            assert str(e.value) == "Logistic Regression with L1 penalty on the GPU engine implements the liblinear objective only, got saga."
            monkeypatch.setenv("PSK_L1_SAGA", "1")
        _run(wd, argv)
        for nm in names:
            assert (wd / nm).exists(), (solver, nm)
        params = (wd / names[0]).read_text().split("Parameters:\n")[1].splitlines()[0]
        assert params == "LogisticRegression(max_iter=1000, penalty='l1', solver='%s')" % solver
        pkg = skpickle.load_linear_package(str(wd / names[2]))
        assert pkg is not None
        icpt[solver] = float(np.asarray(pkg["model"].intercept_).ravel()[0])
        wds[solver] = wd
    assert icpt["saga"] != icpt["liblinear"], icpt
    print("intercepts of the two models: %r" % icpt)
    wd = wds["saga"]
    summary = (wd / names[0]).read_text()
    block = summary.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: ln.split()[2] for ln in block.splitlines()}
    assert len(trained) == sum(1 for v in ds["pheno"] if v != "NA")
    os.chdir(wd)
    with open("samples.txt", "w") as f:
        for line in open("data.pheno").read().splitlines()[1:]:
            if line.strip():
                f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    _run(wd, ["prediction", "samples.txt", "phenos.txt"])
    out = open("predictions_Pheno.txt").read().splitlines()
    pred = {ln.split("\t")[0]: ln.split("\t")[1] for ln in out[1:]}
    assert {k: pred[k] for k in trained} == trained
