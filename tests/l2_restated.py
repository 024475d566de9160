"""The two kernels of csrc/solver_l2.hip restated in NumPy, f64: the CPU yardstick of the L2 solver tests.  Step for step
what one workgroup runs on the training rows of its fit, so that the iteration counts and a fit stopped early are comparable:
  * ridge: conjugate gradients on (Xc'Xc + alpha I) w = Xc'yc, Xc and yc centred by the training rows' means; stop when
    rs <= 1e-26 b2 (rs the recurrence's squared residual, b2 that of w = 0) or d'Ad <= 0; at most 4 min(n, p) + 100 steps,
    n counting the held-out rows too; intercept = ybar - mu.w;
  * logistic: Newton steps on 0.5 (w'w [+ b^2]) + C sum log(1 + exp(-y (x.w + b))) from w = b = 0, each solved by CG on the
    Hessian (stop rs <= 1e-20 g2 or p'Hp <= 0, at most min(l, p) + 10 steps, l the training rows), then Armijo halving
    (f1 <= f0 + 1e-4 step g'd, 40 halvings).  Stop rules, evaluated before a step is taken:
      free intercept   max|grad| <= tol C
      liblinear        ||grad|| <= tol min(pos, neg)/l ||grad at 0||     (min(pos, neg) at least 1)
    Near the optimum the decrease a Newton step promises, |g'd|, falls below the rounding of the objective (eps |f0|); the
    Armijo test then compares noise, may halve a good step down to one that changes nothing, "accept" that, and do so again
    every Newton step until max_iter (tests/test_l2_host.py::test_the_line_search_can_stall).
What differs from the device is the order of every sum, nothing else.

Also here, shared by tests/test_l2_host.py and tests/test_gpu_l2_solvers.py: the designs, grad_l2, ridge_residual and the
bounds both files assert."""
import numpy as np

EPS = 2.0 ** -52

# (n, p): the smallest shapes that reach each path of a 256-thread workgroup whose matrix products are unrolled by 4
SHAPES = [(261, 40),     # a second trip over the samples, tail 1
          (60, 259),     # a second trip over the columns, tail 3
          (515, 517),    # a third trip of both, tails 3 and 1, p > n
          (1030, 130),   # a fifth trip, tail 2
          (7, 3),        # tail only
          (300, 2),      # tail only in p
          (2, 1)]        # the smallest shape the entry points admit
FOLD_SHAPES = [(261, 40), (515, 517)]
TOLS = (1e-4, 1e-8)
MAX_ITER = 200
# Seeds of the designs, (n, p, counts) -> seed, 0 where none is named.  With C = 1000 a training fold is nearly separable and the
# free-intercept optimum lies in a flat valley: a fit that meets max|grad| <= tol C there may still be more than 1e-6 from the
# oracle, whichever solver found it (most seeds of the two fold shapes: 28 of the first 29 of 515 x 517 counts).  These are
# seeds under which the restatement's fits stay within rtol 1e-6 / atol 1e-8 -- by a factor of 4 and more on the first three,
# by 1.16 on 515 x 517 counts (132: the best of 280 seeds tried); test_l2_host.py prints the figures.
SEEDS = {(261, 40, False): 4, (261, 40, True): 18, (515, 517, False): 5, (515, 517, True): 132}
STALL_SEED = 32    # 261 x 40 0/1: the restatement's free-intercept fit of C = 0.0316 at tol = 1e-8 stalls in its line search
CONST_COL, ZERO_COL, DUP_COL = 3, 5, 7      # with p > 9; the duplicate of DUP_COL is the last column


def design(n, p, counts, seed=None):
    """(X[n][p], yc[n], y01[n]).  Twelve random 0/1 base columns (density 0.4); every column of X is one of them with 15 %
    of its cells flipped, so the columns are strongly correlated as k-mers of one genome region are.  counts: every cell
    times max(1, Poisson(2)), five cells set to 200.  p > 9: a constant-1 column, an all-zero column and an exact duplicate
    pair.  yc: six columns times normal weights plus N(0, 0.3); y01: the same signal plus N(0, 0.5), cut at its median."""
    rng = np.random.default_rng([SEEDS.get((n, p, bool(counts)), 0) if seed is None else seed, n, p, int(counts)])
    base = rng.random((n, 12)) < 0.4
    X = (base[:, rng.integers(0, 12, p)] ^ (rng.random((n, p)) < 0.15)).astype(np.float64)
    if counts:
        X *= np.maximum(1, rng.poisson(2, (n, p)))
        X[rng.integers(0, n, 5), rng.integers(0, p, 5)] = 200.0
    if p > 9:
        X[:, CONST_COL] = 1.0
        X[:, ZERO_COL] = 0.0
        X[:, p - 1] = X[:, DUP_COL]
    cols = rng.choice(p, min(6, p), replace=False)
    signal = X[:, cols] @ rng.standard_normal(len(cols))
    yc = signal + 0.3 * rng.standard_normal(n)
    noisy = signal + 0.5 * rng.standard_normal(n)
    y01 = (noisy > np.median(noisy)).astype(np.int64)
    return X, yc, y01


def designs(shapes=SHAPES, seed=None):
    """[(name, X, yc, y01)]: every shape as a 0/1 and as a count design."""
    return [("%dx%d %s" % (n, p, "counts" if c else "0/1"),) + design(n, p, c, seed) for n, p in shapes for c in (False, True)]


# ---------------------------------------------------------------------------------------------------------------------------
# ridge
# ---------------------------------------------------------------------------------------------------------------------------
def ridge_fit(X, y, alpha, n_all=None):
    """X, y: the training rows; n_all: the number of rows of the call (the step cap counts the held-out rows too).
    Returns (coef, intercept, CG steps)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = X.shape
    mu, ybar = X.mean(axis=0), y.mean()
    Xc, yc = X - mu, y - ybar
    w = np.zeros(p)
    r = Xc.T @ yc
    d = r.copy()
    rs = b2 = r @ r
    it, cap = 0, 4 * min(n if n_all is None else n_all, p) + 100
    while it < cap:
        if not rs > 1e-26 * b2:
            break
        q = Xc.T @ (Xc @ d) + alpha * d
        dq = d @ q
        if not dq > 0.0:
            break
        a = rs / dq
        w += a * d
        r -= a * q
        rs_new = r @ r
        d = r + (rs_new / rs) * d
        rs = rs_new
        it += 1
    return w, float(ybar - mu @ w), it


def ridge_residual(X, y, w, alpha):
    """Xc'yc - (Xc'Xc + alpha I) w over the rows given: the gradient of the ridge objective over -2, zero at the optimum."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    Xc, yc = X - X.mean(axis=0), y - y.mean()
    return Xc.T @ (yc - Xc @ w) - alpha * np.asarray(w, dtype=np.float64)


def ridge_system(X, y, alpha):
    """(||Xc'yc||_2, ||Xc'Xc + alpha I||_2) over the rows given: what the residual bound is made of."""
    X = np.asarray(X, dtype=np.float64)
    Xc, yc = X - X.mean(axis=0), np.asarray(y, dtype=np.float64) - np.mean(y)
    return float(np.linalg.norm(Xc.T @ yc)), float(np.linalg.norm(Xc, 2) ** 2 + alpha)


def ridge_residual_bound(X, y, w, alpha, steps):
    """What ||ridge_residual|| of a fit that stopped by its rule may be: the rule's 1e-13 ||b|| on the recurrence's residual,
    plus the gap between that and the true residual.  Every CG step adds to the gap the rounding of one product A d (n + p
    terms per entry) and of the updates of w and r; summed over the steps that is at most steps (n + p) eps ||A||_2 ||w||_2
    to first order (Greenbaum 1997, "Estimating the attainable accuracy of recursively computed residual methods", with
    max_k ||w_k|| taken as ||w||: CG's iterates grow monotonically in norm from w = 0).  One more step's worth for the f64
    evaluation on the host.  A kernel that sums the wrong rows or columns leaves a residual near ||b||."""
    b, A = ridge_system(X, y, alpha)
    n, p = np.shape(X)
    return 1e-13 * b + (steps + 1) * (n + p) * EPS * A * float(np.linalg.norm(w))


def ridge_error_bound(X, y, w_a, w_b, alpha):
    """||w_a - w_b||_2 <= (||res(w_a)|| + ||res(w_b)||) / alpha: the system's smallest eigenvalue is at least alpha.  Times 2
    for the rounding of the residuals' own evaluation."""
    return 2.0 * (np.linalg.norm(ridge_residual(X, y, w_a, alpha)) + np.linalg.norm(ridge_residual(X, y, w_b, alpha))) / alpha


def ridge_intercept_bound(X, y, w_a, w_b, alpha):
    """|b_a - b_b| = |mu.(w_a - w_b)| <= ||mu|| ||w_a - w_b||, plus 1e-12 |ybar| for the two means."""
    X = np.asarray(X, dtype=np.float64)
    return ridge_error_bound(X, y, w_a, w_b, alpha) * np.linalg.norm(X.mean(axis=0)) + 1e-12 * abs(float(np.mean(y)))


# ---------------------------------------------------------------------------------------------------------------------------
# L2 logistic regression
# ---------------------------------------------------------------------------------------------------------------------------
def _log1pexp(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def logreg_l2_fit(X, y01, C, tol=1e-4, max_iter=MAX_ITER, pen=False, counts=None):
    """X, y01: the training rows.  Returns (coef, intercept, Newton steps).  counts: a list that receives the CG steps of
    every Newton step."""
    X = np.asarray(X, dtype=np.float64)
    y = 2.0 * np.asarray(y01, dtype=np.float64) - 1.0
    l, p = X.shape
    bpen = 1.0 if pen else 0.0
    npos, nneg = float((y > 0).sum()), float((y < 0).sum())
    eps_ll = tol * max(min(npos, nneg), 1.0) / l
    w, b, z = np.zeros(p), 0.0, np.zeros(l)
    g0norm = 0.0
    newton = 0
    while newton < max_iter:
        s = 1.0 / (1.0 + np.exp(y * z))
        t = -C * y * s
        Dv = C * s * (1.0 - s)
        fsum = C * _log1pexp(-y * z).sum()
        gb = t.sum() + bpen * b
        g = X.T @ t + w
        g2 = g @ g + gb * gb
        gmax = max(np.abs(g).max(), abs(gb))
        ww = w @ w + bpen * b * b
        gnorm = np.sqrt(g2)
        if newton == 0:
            g0norm = gnorm
        if (gnorm <= eps_ll * g0norm if pen else gmax <= tol * C) or not gnorm > 0.0:
            break
        f0 = 0.5 * ww + fsum
        dw, db = np.zeros(p), 0.0
        r, rb = -g, -gb
        pw, pb = r.copy(), rb
        rs = g2
        cg = 0
        while cg < int(min(l, p)) + 10:
            if not rs > 1e-20 * g2:
                break
            xd = Dv * (X @ pw + pb)
            qb = xd.sum() + bpen * pb
            qw = X.T @ xd + pw
            pq = pw @ qw + pb * qb
            if not pq > 0.0:
                break
            a = rs / pq
            dw += a * pw
            r -= a * qw
            db += a * pb
            rb -= a * qb
            rn = r @ r + rb * rb
            pw = r + (rn / rs) * pw
            pb = rb + (rn / rs) * pb
            rs = rn
            cg += 1
        if counts is not None:
            counts.append(cg)
        xd = X @ dw + db
        wd = w @ dw + bpen * b * db
        dd = dw @ dw + bpen * db * db
        gd = t @ xd + wd
        step, ok = 1.0, False
        for _ in range(40):
            f1 = 0.5 * (ww + 2.0 * step * wd + step * step * dd) + C * _log1pexp(-y * (z + step * xd)).sum()
            if f1 <= f0 + 1e-4 * step * gd:
                ok = True
                break
            step *= 0.5
        if not ok:
            break
        w += step * dw
        z += step * xd
        b += step * db
        newton += 1
    return w, float(b), newton


def grad_l2(X, y01, w, b, C, pen):
    """The gradient of 0.5 (w'w [+ b^2]) + C sum log(1 + exp(-y (x.w + b))) over (w, b) at the rows given: p + 1 values."""
    X = np.asarray(X, dtype=np.float64)
    y = 2.0 * np.asarray(y01, dtype=np.float64) - 1.0
    t = -C * y / (1.0 + np.exp(y * (X @ w + b)))
    return np.concatenate([X.T @ t + w, [t.sum() + (b if pen else 0.0)]])


def grad_rounding(X, w, C):
    """n eps (|w|_inf + C max_j sum_i |x_ij|): the worst-case rounding of one entry of the gradient's own sum (n terms of at
    most C |x_ij| each, the intercept's among them when the design has a column of ones or larger)."""
    X = np.asarray(X, dtype=np.float64)
    colsum = max(float(np.abs(X).sum(axis=0).max()), float(len(X)))
    return len(X) * EPS * (float(np.abs(w).max()) + C * colsum)


def free_stop_bound(X, w, C, tol):
    """The free-intercept contract of psk.h, evaluated on the host: max|grad| <= tol C, plus the gradient's rounding."""
    return tol * C + grad_rounding(X, w, C)


def liblinear_stop_bound(X, y01, w, C, tol):
    """The liblinear contract, evaluated on the host: ||grad||_2 <= tol min(pos, neg)/l ||grad at 0||_2, plus the rounding of
    the p + 1 entries.  Without this the distance bound below says nothing: it holds at any point at all."""
    y01 = np.asarray(y01)
    l, p = np.shape(X)
    mn = max(min(int((y01 == 1).sum()), int((y01 == 0).sum())), 1)
    g0 = np.linalg.norm(grad_l2(X, y01, np.zeros(p), 0.0, C, True))
    return tol * mn / l * g0 + np.sqrt(p + 1.0) * grad_rounding(X, w, C)


def liblinear_error_bound(X, y01, th_a, th_b, C):
    """||theta_a - theta_b||_2 <= ||grad(theta_a)|| + ||grad(theta_b)||: with every coordinate penalised the objective is
    1-strongly convex.  Times 2 for the rounding of the gradients' own evaluation."""
    return 2.0 * sum(np.linalg.norm(grad_l2(X, y01, th[:-1], th[-1], C, True)) for th in (th_a, th_b))


# ---------------------------------------------------------------------------------------------------------------------------
# the fits both test files run
# ---------------------------------------------------------------------------------------------------------------------------
def fold_plan(grid, n_folds):
    """Every fourth grid value on every fold: (fit_param, fit_fold)."""
    return [g for g in grid[::4] for _ in range(n_folds)], [f for _ in grid[::4] for f in range(n_folds)]


def one_class_folds(y01):
    """Fold ids under which fit_fold = 0 trains on the samples of class 1 alone."""
    return np.where(np.asarray(y01) == 0, 0, 1).astype(np.int32)


def grids():
    """(alphas, Cs): the 13-value grids of tests/golden/model_kat.npz."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_kat.npz"))
    return [float(a) for a in z["alphas"]], [float(c) for c in z["Cs"]]


def plans(X, y01, alphas, Cs):
    """The launches of one design: {"ridge": [(fold, fit_param, fit_fold)], "logit": [...]}: the grid on all samples, and on
    the two fold shapes every fourth grid value on 10 contiguous (ridge) or 5 stratified (logistic) folds."""
    from oracle import oracle_model as OM
    n = len(X)
    zero = np.zeros(n, dtype=np.int32)
    out = {"ridge": [(zero, alphas, [-1] * len(alphas))], "logit": [(zero, Cs, [-1] * len(Cs))]}
    if n == 2:      # fold id 0 of fold = [0, 1] leaves one training row: w = 0, intercept = that row's y
        out["ridge"].append((np.array([0, 1], dtype=np.int32), alphas[::4], [0] * len(alphas[::4])))
    if X.shape in FOLD_SHAPES:
        out["ridge"].append((OM.kfold(n, 10).astype(np.int32),) + fold_plan(alphas, 10))
        out["logit"].append((OM.stratified_kfold(y01, 5).astype(np.int32),) + fold_plan(Cs, 5))
    return out


class Oracle:
    """oracle_model's fits, each solved once however many tests ask for it."""

    def __init__(self):
        self._kept = {}

    def _get(self, key, make):
        if key not in self._kept:
            self._kept[key] = make()
        return self._kept[key]

    def ridge(self, name, X, y, fold, tf, alpha):
        from oracle import oracle_model as OM
        tr = fold != tf
        return self._get(("ridge", name, fold.tobytes(), tf, alpha), lambda: OM.ridge_fit(X[tr], y[tr], alpha))

    def logit(self, name, X, y01, fold, tf, C, pen):
        from oracle import oracle_model as OM
        tr = fold != tf
        return self._get(("logit", name, fold.tobytes(), tf, C, pen), lambda: OM.logreg_l2_fit(X[tr], y01[tr], C, pen))


def judge_ridge(oracle, name, X, y, fold, fit_param, fit_fold, coef, icpt, iters):
    """Asserts section by section what a ridge launch owes; returns (largest error / bound, largest residual / bound,
    largest step count, fits that ended at the cap)."""
    n, p = X.shape
    cap = 4 * min(n, p) + 100
    worst_e = worst_r = 0.0
    capped = 0
    for j, (alpha, tf) in enumerate(zip(fit_param, fit_fold)):
        tr = fold != tf
        Xt, yt, w, b, it = X[tr], y[tr], coef[j], float(icpt[j]), int(iters[j])
        what = (name, "alpha=%g" % alpha, "fold=%d" % tf, "steps=%d" % it)
        assert np.all(np.isfinite(w)) and np.isfinite(b), what
        assert 0 <= it <= cap, what
        capped += it == cap
        if tr.sum() == 1:
            assert np.all(w == 0.0) and b == yt[0] and it == 0, what
            continue
        wo, bo = oracle.ridge(name, X, y, fold, tf, alpha)
        res, res_bound = np.linalg.norm(ridge_residual(Xt, yt, w, alpha)), ridge_residual_bound(Xt, yt, w, alpha, it)
        err, err_bound = np.linalg.norm(w - wo), ridge_error_bound(Xt, yt, w, wo, alpha)
        worst_r, worst_e = max(worst_r, res / res_bound if res_bound > 0 else 0.0), max(worst_e, err / err_bound if err_bound > 0 else 0.0)
        assert res <= res_bound, what + ("residual %.3g, bound %.3g" % (res, res_bound),)
        assert err <= err_bound, what + ("error %.3g, bound %.3g" % (err, err_bound),)
        assert abs(b - bo) <= ridge_intercept_bound(Xt, yt, w, wo, alpha), what
        if p > 9:
            one = 2.0 * res / alpha             # ||w - w*|| of this fit alone, w* the optimum itself
            assert w[ZERO_COL] == 0.0, what
            assert abs(w[CONST_COL]) <= one or not np.all(Xt[:, CONST_COL] == 1.0), what       # it centres to zero: w* = 0
            assert abs(w[DUP_COL] - w[p - 1]) <= np.sqrt(2.0) * one, what                       # w* splits the weight evenly
    return worst_e, worst_r, int(np.max(iters)), capped


def judge_logit(oracle, name, X, y01, fold, fit_param, fit_fold, coef, icpt, iters, tol, pen, max_iter=MAX_ITER):
    """The same for a logistic launch; returns (largest error / bound [liblinear] or largest |coef - oracle| / (1e-8 + 1e-6
    |oracle|) [free intercept, tol = 1e-8], largest host-evaluated gradient / stop bound, largest Newton count)."""
    n, p = X.shape
    worst_e = worst_s = 0.0
    for j, (C, tf) in enumerate(zip(fit_param, fit_fold)):
        tr = fold != tf
        Xt, yt, w, b, it = X[tr], y01[tr], coef[j], float(icpt[j]), int(iters[j])
        what = (name, "C=%g" % C, "fold=%d" % tf, "tol=%g" % tol, "pen=%d" % pen, "newton=%d" % it)
        assert np.all(np.isfinite(w)) and np.isfinite(b), what
        assert 0 <= it < max_iter, what
        wo, bo = oracle.logit(name, X, y01, fold, tf, C, pen)
        g = grad_l2(Xt, yt, w, b, C, pen)
        th, tho = np.append(w, b), np.append(wo, bo)
        if pen:
            stop, stop_bound = np.linalg.norm(g), liblinear_stop_bound(Xt, yt, w, C, tol)
            err, err_bound = np.linalg.norm(th - tho), liblinear_error_bound(Xt, yt, th, tho, C)
            worst_e = max(worst_e, err / err_bound if err_bound > 0 else 0.0)
            assert err <= err_bound, what + ("error %.3g, bound %.3g" % (err, err_bound),)
            pair = 2.0 * np.sqrt(2.0) * np.linalg.norm(g)
        else:
            stop, stop_bound = np.abs(g).max(), free_stop_bound(Xt, w, C, tol)
            pair = None
            if tol <= 1e-8:
                worst_e = max(worst_e, float(np.max(np.abs(th - tho) / (1e-8 + 1e-6 * np.abs(tho)))))
                assert np.allclose(th, tho, rtol=1e-6, atol=1e-8), what
                pair = 2.0 * (1e-8 + 1e-6 * abs(wo[p - 1])) if p > 9 else None
        worst_s = max(worst_s, stop / stop_bound if stop_bound > 0 else 0.0)
        assert stop <= stop_bound, what + ("gradient %.3g, bound %.3g" % (stop, stop_bound),)
        if p > 9:
            assert w[ZERO_COL] == 0.0, what
            if pair is not None:
                assert abs(w[DUP_COL] - w[p - 1]) <= pair, what
    return worst_e, worst_s, int(np.max(iters))


def one_step_cases(Cs):
    """[(name, X, y01, Cs)] of the max_iter = 1 tests.  A Newton step's CG solve ends at a relative residual of 1e-10 or at
    its step cap, and what is left of the residual depends on the order of the sums: on count designs with large C, where
    the solve ends at the cap, two orders differ by up to 8e-6 of the step.  So: both designs of the tail-only shapes under
    every C, and the 0/1 designs of the two second-trip shapes under C <= 0.1, where re-ordering the sums moves the step
    by less than 1e-10 (tests/test_l2_host.py::test_max_iter_one_is_one_newton_step)."""
    out = []
    for shape in ((7, 3), (300, 2)):
        out += [(name, X, y01, Cs) for name, X, _, y01 in designs([shape])]
    for shape in ((261, 40), (60, 259)):
        out += [(name, X, y01, [C for C in Cs if C <= 0.1]) for name, X, _, y01 in designs([shape])[:1]]
    return out
