"""CPU tests of the L2 solvers' algorithms: tests/l2_restated.py -- the two kernels of csrc/solver_l2.hip in NumPy -- against
oracle_model's direct solves, on every design, launch, tolerance and bound that tests/test_gpu_l2_solvers.py puts to the device.
A case that fails here is outside what the algorithm itself delivers and has no place in the GPU tests."""
import numpy as np
import pytest

import l2_restated as R

np.seterr(over="ignore")        # exp() of a large margin overflows to inf on purpose: 1 / (1 + inf) = 0


@pytest.fixture(scope="module")
def oracle():
    return R.Oracle()


def _launch_ridge(X, y, fold, fit_param, fit_fold):
    fits = [R.ridge_fit(X[fold != tf], y[fold != tf], a, n_all=len(X)) for a, tf in zip(fit_param, fit_fold)]
    return np.array([f[0] for f in fits]), np.array([f[1] for f in fits]), np.array([f[2] for f in fits])


def _launch_logit(X, y01, fold, fit_param, fit_fold, tol, pen, max_iter=R.MAX_ITER):
    fits = [R.logreg_l2_fit(X[fold != tf], y01[fold != tf], C, tol, max_iter, pen) for C, tf in zip(fit_param, fit_fold)]
    return np.array([f[0] for f in fits]), np.array([f[1] for f in fits]), np.array([f[2] for f in fits])


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_restated_ridge_against_the_oracle(oracle, shape):
    alphas, Cs = R.grids()
    for name, X, yc, y01 in R.designs([shape]):
        for fold, fp, ff in R.plans(X, y01, alphas, Cs)["ridge"]:
            e, r, steps, capped = R.judge_ridge(oracle, name, X, yc, fold, fp, ff, *_launch_ridge(X, yc, fold, fp, ff))
            print("%s ridge, %d fits: error/bound %.3g, residual/bound %.3g, most CG steps %d of %d, %d at the cap"
                  % (name, len(fp), e, r, steps, 4 * min(shape) + 100, capped))


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_restated_logistic_against_the_oracle(oracle, shape):
    alphas, Cs = R.grids()
    for name, X, yc, y01 in R.designs([shape]):
        for fold, fp, ff in R.plans(X, y01, alphas, Cs)["logit"]:
            for pen in (False, True):
                for tol in R.TOLS:
                    e, s, newton = R.judge_logit(oracle, name, X, y01, fold, fp, ff, *_launch_logit(X, y01, fold, fp, ff, tol, pen),
                                                 tol, pen)
                    print("%s %s tol=%g, %d fits: error %.3g, gradient/bound %.3g, most Newton steps %d"
                          % (name, "liblinear" if pen else "free", tol, len(fp), e, s, newton))


def test_restated_one_class_training_set(oracle):
    """liblinear's rule on a training set of one class: the penalised intercept keeps the optimum finite."""
    alphas, Cs = R.grids()
    X, _, y01 = R.design(261, 40, False)
    fold = R.one_class_folds(y01)
    for tol in R.TOLS:
        R.judge_logit(oracle, "261x40 one class", X, y01, fold, Cs[::4], [0] * 4, *_launch_logit(X, y01, fold, Cs[::4], [0] * 4, tol, True),
                      tol, True)


def test_the_line_search_can_stall():
    """The algorithm as it stands, on a 261 x 40 0/1 design with a free intercept at tol = 1e-8: the fit of C = 0.0316 is at
    twenty times its threshold (6.6e-9 against 3.2e-10) when the decrease a Newton step promises (about 1e-16) falls below the rounding of the objective;
    the Armijo test then rejects the step down to one that changes nothing, and the fit spends all 200 iterations there.
    What it returns is accurate all the same; what it costs is max_iter CG solves.  Whether a fit does this depends on the
    last bits of its sums: the device ran this design in 9 steps, and needed 173 instead of 10 on it under liblinear's rule
    at tol = 1e-12 (docs/NOTEBOOK.md, round 24)."""
    alphas, Cs = R.grids()
    X, _, y01 = R.design(261, 40, False, seed=R.STALL_SEED)
    fold, ff = np.zeros(len(X), dtype=np.int32), [-1] * len(Cs)
    coef, icpt, newton = _launch_logit(X, y01, fold, Cs, ff, 1e-8, False)
    print("Newton steps %s" % newton.tolist())
    assert (newton == R.MAX_ITER).tolist() == [C == Cs[9] for C in Cs]
    g = np.abs(R.grad_l2(X, y01, coef[9], icpt[9], Cs[9], False)).max()
    assert g > 1e-8 * Cs[9]
    from oracle import oracle_model as OM
    wo, bo = OM.logreg_l2_fit(X, y01, Cs[9])
    assert np.allclose(np.append(coef[9], icpt[9]), np.append(wo, bo), rtol=1e-6, atol=1e-8)


def test_max_iter_one_is_one_newton_step():
    """The device's first iterate is held to the restatement's within 1e-9: on the cases chosen, the restatement with its rows
    and columns permuted -- every sum in another order -- agrees with itself to 1e-10."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for name, X, y01, Cs in R.one_step_cases(R.grids()[1]):
        n, p = X.shape
        for pen in (False, True):
            for C in Cs:
                w, b, newton = R.logreg_l2_fit(X, y01, C, 1e-8, 1, pen)
                assert newton == 1 and np.any(w != 0.0), (name, C)
                rows, cols = rng.permutation(n), rng.permutation(p)
                w2, b2, _ = R.logreg_l2_fit(X[rows][:, cols], y01[rows], C, 1e-8, 1, pen)
                back = np.empty(p)
                back[cols] = w2
                moved = max(np.abs(back - w).max(), abs(b2 - b)) / max(np.abs(w).max(), abs(b))
                worst = max(worst, moved)
                assert moved <= 1e-10, (name, pen, C, moved)
    print("one Newton step under a permutation of rows and columns: moved by %.3g of its largest entry at most" % worst)


def test_the_model_layer_design_has_no_sample_on_the_boundary():
    """test_gpu_l2_solvers.py asks the grid search for the oracle's accuracy exactly: no test sample of any fold, under any C
    and either intercept rule, may have a decision value within 1e-6 of 0 in the oracle."""
    from oracle import oracle_model as OM
    alphas, Cs = R.grids()
    X, _, y01 = R.design(261, 40, True)
    folds = OM.stratified_kfold(y01, 5)
    closest = np.inf
    for pen in (False, True):
        for C in Cs:
            for f in range(5):
                w, b = OM.logreg_l2_fit(X[folds != f], y01[folds != f], C, pen)
                closest = min(closest, float(np.abs(X[folds == f] @ w + b).min()))
    print("closest decision value to 0: %.3g" % closest)
    assert closest > 1e-6
