"""GPU tests (-m gpu) of the float L1 kernels of csrc/solver.hip on count designs and on every placement of their per-fit
state: logreg_newglmnet_kernel with the feature and the sample arrays in LDS or in global scratch (cases A..D of
tests/l1_float_cases.py), past one 64-lane trip with a tail, on cells that are neither 0 nor 1, and at the hand-over from the
bit-packed kernels at 4,096 / 4,097 samples; lasso_kernel<EN> where the residual is exactly 64 KiB of LDS and where it leaves
LDS.  Yardsticks: oracle_model.logreg_l1_arbiter from a zero hint and the certified NumPy descent of l1_float_cases, both held
to their own KKT conditions on the CPU (tests/test_l1_float_host.py).  Every test prints what it measured over its bound."""
import time

import numpy as np
import pytest

import l1_float_cases as L

pytestmark = pytest.mark.gpu

np.seterr(over="ignore")        # exp() of a large margin overflows to inf on purpose: 1 / (1 + inf) = 0


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


def _fit(ctx, name, tol, max_iter):
    X, y, fold, fp, ff = L.case_data(name)
    t0 = time.perf_counter()
    r = ctx.logreg_l1_fit(X, y, fold, fp, ff, tol=tol, max_iter=max_iter)
    return r, time.perf_counter() - t0


def _against_the_arbiter(ctx, name):
    X, y, fold, fp, ff = L.case_data(name)
    arbs = L.certified(name)
    assert all(a["kkt"] < L.KKT_MAX for a in arbs)
    (coef, icpt, iters), secs = _fit(ctx, name, 1e-4, 1000)
    stop, gap, steps = L.judge_logit(name, X, y, fold, fp, ff, coef, icpt, iters, arbs)
    print("%s %dx%d placement %s, %d fits: stop-rule violation / bound %.3g, objective gap / 1 %% %.3g, Newton steps %d..%d, "
          "%.2f s on the device" % (name, X.shape[0], X.shape[1], L.CASES[name]["place"], len(fp), stop, gap, iters.min(), steps, secs))


@pytest.mark.parametrize("name", [n for n in L.TABLE if n != "D"])
def test_every_placement_reaches_the_certified_optimum_at_the_reference_tolerance(ctx, name):
    """tol = 1e-4, max_iter = 1000 (what the reference runs): fewer than 200 Newton steps, liblinear's stop rule for the true
    gradient, the objective within [1 - 1e-9, 1.01] of the arbiter's."""
    _against_the_arbiter(ctx, name)


def test_case_d_with_every_array_in_global_scratch(ctx):
    """3892 x 3892: neither the feature nor the sample arrays fit LDS.  The longest case, in a function of its own."""
    _against_the_arbiter(ctx, "D")


@pytest.mark.parametrize("name", [n for n in L.TABLE if L.CASES[n]["tight"]])
def test_tight_tolerance_lands_on_the_certified_coefficients(ctx, name):
    """tol = 1e-12, max_iter = 5000, the bounds of test_l1_logreg_solver_reaches_liblinear_optimum: pattern sums and intercept
    rel 1e-6, the same support, the linear predictor rtol 1e-6, the objective rel 1e-12."""
    X, y, fold, fp, ff = L.case_data(name)
    (coef, icpt, iters), secs = _fit(ctx, name, 1e-12, 5000)
    ce, le, oe, steps = L.judge_tight(name, X, y, fold, fp, ff, coef, icpt, iters, L.certified(name))
    print("%s tol 1e-12: coefficient error / 1e-6 %.3g, predictor error / bound %.3g, objective error / 1e-12 %.3g, Newton steps "
          "%d..%d, %.2f s" % (name, ce, le, oe, iters.min(), steps, secs))


def test_the_hand_over_at_4096_samples(ctx):
    """The 4,097-row 0/1 design runs the float kernel, its first 4,096 rows the bit-packed one (each held to the arbiter above).
    One row apart, the two optima bracket each other: adding a row adds a non-negative loss, and the smaller problem's optimum
    is a point of the larger one -- opt(4096) <= opt(4097) <= opt(4096) + C loss of row 4096 at the smaller optimum."""
    X, y, fold, fp, ff = L.case_data("C-bin")
    assert L.route_is_float("C-bin") and not L.route_is_float("C-bin-4096")
    (c7, b7, _), _ = _fit(ctx, "C-bin", 1e-12, 5000)
    (c6, b6, _), _ = _fit(ctx, "C-bin-4096", 1e-12, 5000)
    ypm = 2.0 * y - 1.0
    o7 = L.objectives(X, ypm, fold, fp, ff, c7, b7)
    o6 = L.objectives(X[:4096], ypm[:4096], fold[:4096], fp, ff, c6, b6)
    last = fp * np.logaddexp(0.0, -ypm[4096] * (c6 @ X[4096].astype(np.float64) + b6))
    for j in range(len(fp)):
        assert o6[j] * (1 - 1e-12) <= o7[j] <= (o6[j] + last[j]) * (1 + 1e-12), (j, o6[j], o7[j], last[j])
    print("objective(4097) - objective(4096) over the last row's loss: %s" % ((o7 - o6) / last).round(4).tolist())


@pytest.mark.parametrize("name", ["A", "C"])
def test_held_out_rows_do_not_matter(ctx, name):
    """The rows of fold 1 overwritten with counts up to 1e6 and their labels flipped: every output of the fits that hold fold 1
    out is bit-identical."""
    X, y, fold, fp, ff = L.case_data(name)
    X2, y2 = L.garbage(X, y, fold, 1)
    assert np.any((X2[fold != 1] != 0) & (X2[fold != 1] != 1))      # still the float route without the overwritten rows
    sel = np.nonzero(ff == 1)[0]
    assert len(sel) >= 3
    a = ctx.logreg_l1_fit(X, y, fold, fp, ff, tol=1e-4, max_iter=1000)
    b = ctx.logreg_l1_fit(X2, y2, fold, fp, ff, tol=1e-4, max_iter=1000)
    for u, v, what in zip(a, b, ("coef", "intercept", "Newton steps")):
        assert np.array_equal(u[sel], v[sel]), (name, what)
    assert np.any(a[0][sel] != 0)


def test_six_hundred_fits_in_one_launch_are_deterministic(ctx):
    """More fits than compute units: 20 C x (5 folds + refit) of 65 x 30 counts, five times over.  The launch equals its own
    repeat bit for bit; its first 120 fits launched alone equal indices 0..119 (the sweep permutation is seeded by the fit
    index, so only equal indices are comparable); every fit meets the bounds of the reference tolerance."""
    X, y, fold, fp, ff = L.case_data("E")
    arbs = L.certified("E")
    fp5, ff5 = np.tile(fp, 5), np.tile(ff, 5)
    assert len(fp5) == 600
    t0 = time.perf_counter()
    a = ctx.logreg_l1_fit(X, y, fold, fp5, ff5, tol=1e-4, max_iter=1000)
    secs = time.perf_counter() - t0
    b = ctx.logreg_l1_fit(X, y, fold, fp5, ff5, tol=1e-4, max_iter=1000)
    c = ctx.logreg_l1_fit(X, y, fold, fp, ff, tol=1e-4, max_iter=1000)
    for u, v, w, what in zip(a, b, c, ("coef", "intercept", "Newton steps")):
        assert np.array_equal(u, v), what
        assert np.array_equal(u[:120], w), what
    stop, gap, steps = L.judge_logit("E", X, y, fold, fp5, ff5, a[0], a[1], a[2], arbs * 5)
    print("600 fits of 65x30: stop-rule violation / bound %.3g, objective gap / 1 %% %.3g, Newton steps %d..%d, %.2f s"
          % (stop, gap, a[2].min(), steps, secs))


def _lasso(ctx, name, l1_ratio, X=None, y=None):
    X0, y0, fold, fa, ff = L.lasso_data(name)
    X, y = (X0, y0) if X is None else (X, y)
    if l1_ratio is None:
        return ctx.lasso_fit(X, y, fold, fa, ff, tol=L.LASSO_TOL, max_iter=L.LASSO_MAX_ITER)
    return ctx.enet_fit(X, y, fold, fa, ff, l1_ratio, tol=L.LASSO_TOL, max_iter=L.LASSO_MAX_ITER)


@pytest.mark.parametrize("l1_ratio", [None, 0.5], ids=["lasso", "enet 0.5"])
@pytest.mark.parametrize("name", list(L.LASSO_CASES))
def test_lasso_and_elastic_net_where_the_residual_leaves_lds(ctx, name, l1_ratio):
    """8192 samples: the residual is exactly 64 KiB of dynamic LDS; 8193: it lives in global scratch.  tol = 1e-10 against
    the certified NumPy descent: coefficients within 1e-6 of the largest, the same support, the intercept rel 1e-6 / abs
    1e-9.  Then the rows of fold 1 overwritten: the fits that hold it out are bit-identical."""
    X, y, fold, fa, ff = L.lasso_data(name)
    assert L.lasso_use_lds(X.shape[0]) == L.LASSO_CASES[name]["use_lds"]
    refs = L.lasso_certified(name, 1.0 if l1_ratio is None else l1_ratio)
    t0 = time.perf_counter()
    coef, icpt, iters = _lasso(ctx, name, l1_ratio)
    secs = time.perf_counter() - t0
    worst = L.judge_lasso(name, coef, icpt, iters, refs)
    print("%s %s use_lds %d: coefficient error / (1e-6 of the largest) %.3g, sweeps %d..%d, %.2f s"
          % (name, "lasso" if l1_ratio is None else "l1_ratio 0.5", L.LASSO_CASES[name]["use_lds"], worst, iters.min(), iters.max(), secs))
    X2, y2 = L.garbage(X, y, fold, 1)
    g = _lasso(ctx, name, l1_ratio, X2, y2)
    sel = np.nonzero(ff == 1)[0]
    for u, v, what in zip((coef, icpt, iters), g, ("coef", "intercept", "sweeps")):
        assert np.array_equal(u[sel], v[sel]), (name, what)


@pytest.mark.parametrize("name", [n for n, c in L.LASSO_CASES.items() if not c["use_lds"]])
def test_l1_ratio_one_is_the_lasso_bit_for_bit_on_the_global_route(ctx, name):
    """test_gpu_enet.py::test_l1_ratio_one_is_the_lasso_bit_for_bit, with the residual in global scratch."""
    a = _lasso(ctx, name, 1.0)
    b = _lasso(ctx, name, None)
    for u, v, what in zip(a, b, ("coef", "intercept", "sweeps")):
        assert np.array_equal(u, v), (name, what)
