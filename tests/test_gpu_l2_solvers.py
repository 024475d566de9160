"""GPU tests (-m gpu) of psk_ridge_fit and psk_logreg_l2_fit past one trip of their 256-thread loops: the shapes of
l2_restated.SHAPES as 0/1 and count designs, against oracle_model's direct solves under bounds that follow from the
objectives' convexity (l2_restated.judge_ridge / judge_logit; tests/test_l2_host.py holds the algorithm itself to the same);
held-out rows that must not count, 600 fits in one launch, determinism, one Newton step, and the model layer."""
import numpy as np
import pytest

import l2_restated as R

pytestmark = pytest.mark.gpu

np.seterr(over="ignore")        # the host's exp() of a large margin overflows to inf on purpose


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    return R.Oracle()


@pytest.fixture(scope="module")
def grid():
    return R.grids()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_ridge_against_the_oracle(ctx, oracle, grid, shape):
    """Every alpha on all samples; on 261 x 40 and 515 x 517 also every fourth alpha on 10 contiguous folds; on 2 x 1 the fit
    that trains on one row.  Error and residual bounds, degenerate columns and the step cap: judge_ridge."""
    alphas, Cs = grid
    for name, X, yc, y01 in R.designs([shape]):
        for fold, fp, ff in R.plans(X, y01, alphas, Cs)["ridge"]:
            e, r, steps, capped = R.judge_ridge(oracle, name, X, yc, fold, fp, ff, *ctx.ridge_fit(X, yc, fold, fp, ff))
            print("%s ridge, %d fits: error/bound %.3g, residual/bound %.3g, most CG steps %d of %d, %d at the cap"
                  % (name, len(fp), e, r, steps, 4 * min(shape) + 100, capped))


@pytest.mark.parametrize("pen", [False, True], ids=["free", "liblinear"])
@pytest.mark.parametrize("counts", [False, True], ids=["0/1", "counts"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_logistic_against_the_oracle(ctx, oracle, grid, shape, counts, pen):
    """Every C on all samples, on the two fold shapes also every fourth C on 5 stratified folds; tol 1e-4 and 1e-8, both
    intercept rules, max_iter = 200 that no fit may reach.  Stop contract, distance to the oracle, degenerate columns:
    judge_logit."""
    alphas, Cs = grid
    name, X, yc, y01 = R.designs([shape])[int(counts)]
    for fold, fp, ff in R.plans(X, y01, alphas, Cs)["logit"]:
        for tol in R.TOLS:
            got = ctx.logreg_l2_fit(X, y01, fold, fp, ff, tol=tol, max_iter=R.MAX_ITER, penalise_intercept=pen)
            e, s, newton = R.judge_logit(oracle, name, X, y01, fold, fp, ff, *got, tol, pen)
            print("%s %s tol=%g, %d fits: error %.3g, gradient/bound %.3g, most Newton steps %d"
                  % (name, "liblinear" if pen else "free", tol, len(fp), e, s, newton))


def test_one_class_training_set(ctx, oracle, grid):
    """liblinear's rule with the samples of class 0 held out: the penalised intercept keeps the optimum finite."""
    Cs = grid[1][::4]
    X, _, y01 = R.design(261, 40, False)
    fold = R.one_class_folds(y01)
    for tol in R.TOLS:
        got = ctx.logreg_l2_fit(X, y01, fold, Cs, [0] * len(Cs), tol=tol, max_iter=R.MAX_ITER, penalise_intercept=True)
        R.judge_logit(oracle, "261x40 one class", X, y01, fold, Cs, [0] * len(Cs), *got, tol, True)
        assert np.all(got[1] > 0)


@pytest.mark.parametrize("counts", [False, True], ids=["0/1", "counts"])
@pytest.mark.parametrize("shape", R.FOLD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_held_out_rows_do_not_count(ctx, grid, shape, counts):
    """The held-out rows of a fold overwritten with values up to 1e6, their labels flipped, their y replaced: every masked term
    is a product with an exact 0, so coefficients, intercepts and iteration counts keep their bits.  The first fold and the
    last (whose rows lie in the last trip of the sample loops)."""
    from oracle import oracle_model as OM
    alphas, Cs = grid
    rng = np.random.default_rng(7)
    for name, X, yc, y01 in R.designs([shape])[int(counts):int(counts) + 1]:
        n, p = X.shape
        for kind, fold, k in (("ridge", OM.kfold(n, 10).astype(np.int32), 10), ("logit", OM.stratified_kfold(y01, 5).astype(np.int32), 5)):
            for tf in (0, k - 1):
                out = fold == tf
                X2, yc2, y2 = X.copy(), yc.copy(), y01.copy()
                X2[out] = rng.uniform(-1e6, 1e6, (int(out.sum()), p)).astype(np.float32)
                yc2[out] = 1e6 * rng.standard_normal(int(out.sum()))
                y2[out] = 1 - y2[out]
                if kind == "ridge":
                    a = ctx.ridge_fit(X, yc, fold, alphas[::4], [tf] * 4)
                    b = ctx.ridge_fit(X2, yc2, fold, alphas[::4], [tf] * 4)
                    assert _same(a, b), (name, kind, tf)
                    continue
                for pen in (False, True):
                    a = ctx.logreg_l2_fit(X, y01, fold, Cs[::4], [tf] * 4, tol=1e-8, max_iter=R.MAX_ITER, penalise_intercept=pen)
                    b = ctx.logreg_l2_fit(X2, y2, fold, Cs[::4], [tf] * 4, tol=1e-8, max_iter=R.MAX_ITER, penalise_intercept=pen)
                    assert _same(a, b), (name, kind, tf, pen)


@pytest.mark.parametrize("counts", [False, True], ids=["0/1", "counts"])
def test_many_fits_in_one_launch(ctx, grid, counts):
    """600 fits of a 60 x 259 design -- more workgroups than the device has CUs: every (parameter, fold) of the grid search,
    repeated.  All repeats of a pair carry the same bits, and the first fit, the last and ten between them the bits of that
    pair solved in a launch of its own: no slice of the scratch buffer reaches into its neighbour's."""
    from oracle import oracle_model as OM
    alphas, Cs = grid
    X, yc, y01 = R.design(60, 259, counts)
    solo = [0, 599] + list(range(37, 599, 56))[:10]
    for kind, params, fold, k in (("ridge", alphas, OM.kfold(60, 10).astype(np.int32), 10),
                                  ("free", Cs, OM.stratified_kfold(y01, 5).astype(np.int32), 5),
                                  ("liblinear", Cs, OM.stratified_kfold(y01, 5).astype(np.int32), 5)):
        pairs = [(q, f) for q in params for f in list(range(k)) + [-1]]
        plan = (pairs * (600 // len(pairs) + 1))[:600]
        fp, ff = [q for q, _ in plan], [f for _, f in plan]
        if kind == "ridge":
            fit = lambda fp, ff: ctx.ridge_fit(X, yc, fold, fp, ff)
        else:
            fit = lambda fp, ff: ctx.logreg_l2_fit(X, y01, fold, fp, ff, tol=1e-8, max_iter=R.MAX_ITER, penalise_intercept=kind == "liblinear")
        coef, icpt, iters = fit(fp, ff)
        assert np.all(np.isfinite(coef)) and len(set(map(bytes, coef))) == len(pairs), kind      # every pair has its own result
        for j in range(len(pairs), 600):
            i = j % len(pairs)
            assert np.array_equal(coef[j], coef[i]) and icpt[j] == icpt[i] and iters[j] == iters[i], (kind, j)
        for j in solo:
            c1, b1, i1 = fit([fp[j]], [ff[j]])
            assert np.array_equal(coef[j], c1[0]) and icpt[j] == b1[0] and iters[j] == i1[0], (kind, j)
        assert _same((coef, icpt, iters), fit(fp, ff)), kind        # and the launch as a whole is deterministic


def test_the_same_call_twice_gives_the_same_bits(ctx, grid):
    """Neither kernel has an atomic: 515 x 517 counts (three trips of every loop), the grid on all samples."""
    alphas, Cs = grid
    X, yc, y01 = R.design(515, 517, True)
    zero = np.zeros(len(X), dtype=np.int32)
    assert _same(ctx.ridge_fit(X, yc, zero, alphas[::3], [-1] * 5), ctx.ridge_fit(X, yc, zero, alphas[::3], [-1] * 5))
    for pen in (False, True):
        a, b = (ctx.logreg_l2_fit(X, y01, zero, Cs[::3], [-1] * 5, tol=1e-8, max_iter=R.MAX_ITER, penalise_intercept=pen) for _ in range(2))
        assert _same(a, b), pen


def test_max_iter_one_is_one_newton_step(ctx, grid):
    """iters_out == 1 and the restatement's first iterate to 1e-9 of its largest entry: two f64 evaluations of one step whose
    sums run in a different order (the cases: l2_restated.one_step_cases)."""
    worst = 0.0
    for name, X, y01, Cs in R.one_step_cases(grid[1]):
        zero = np.zeros(len(X), dtype=np.int32)
        for pen in (False, True):
            coef, icpt, iters = ctx.logreg_l2_fit(X, y01, zero, Cs, [-1] * len(Cs), tol=1e-8, max_iter=1, penalise_intercept=pen)
            assert np.all(iters == 1), (name, pen)
            for k, C in enumerate(Cs):
                w, b, _ = R.logreg_l2_fit(X, y01, C, 1e-8, 1, pen)
                th, got = np.append(w, b), np.append(coef[k], icpt[k])
                worst = max(worst, float(np.abs(got - th).max() / np.abs(th).max()))
                assert np.abs(got - th).max() <= 1e-9 * np.abs(th).max(), (name, pen, C)
    print("first Newton step: largest |device - restatement| / max|restatement| = %.3g" % worst)


def test_grid_search_against_the_oracle(ctx, grid):
    """GridSearch over RidgeRegression and over L2LogisticRegression (lbfgs: free intercept; liblinear) on the 261 x 40 count
    design against oracle_model.grid_search: folds, R^2 to the parity test's rtol 1e-6 / atol 1e-8, accuracy exactly (no test
    sample is within 1e-6 of the boundary: tests/test_l2_host.py), the best parameter."""
    from oracle import oracle_model as OM
    from phenotypeseeker_amd.model import GridSearch, L2LogisticRegression, RidgeRegression
    alphas, Cs = grid
    X, yc, y01 = R.design(261, 40, True)
    want = OM.grid_search(X, yc, alphas, "ridge", 10)
    gr = GridSearch(RidgeRegression(tol=1e-4, max_iter=1000), "alpha", alphas, 10).fit(X, yc, ctx)
    assert np.array_equal(gr.test_folds_, want["folds"])
    assert np.allclose(gr.cv_results_["mean_test_score"], want["mean_test_score"], rtol=1e-6, atol=1e-8)
    assert gr.best_params_ == {"alpha": alphas[want["best_index"]]}
    for solver, kind in (("lbfgs", "logreg_l2"), ("liblinear", "logreg_l2_liblinear")):
        want = OM.grid_search(X, y01, Cs, kind, 5)
        gl = GridSearch(L2LogisticRegression(tol=1e-8, max_iter=R.MAX_ITER, solver=solver), "C", Cs, 5).fit(X, y01, ctx)
        assert np.array_equal(gl.test_folds_, want["folds"]), solver
        assert np.array_equal(gl.cv_results_["mean_test_score"], want["mean_test_score"]), solver
        assert gl.best_params_ == {"C": Cs[want["best_index"]]}, solver
        assert gl.n_iter_.max() < R.MAX_ITER, solver
