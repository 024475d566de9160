"""The float L1 kernels of csrc/solver.hip -- logreg_newglmnet_kernel, lasso_kernel<EN> -- on count designs and on every
placement of their per-fit state: the designs, the cases, the CPU yardsticks and the bounds that tests/test_l1_float_host.py
(CPU) and tests/test_gpu_l1_float.py (device) share.  No test functions here.

Logistic yardstick: oracle_model.logreg_l1_arbiter from a ZERO hint (max_rounds = 400; it adds the most violated coordinate
each round), certified by its own KKT residual < 1e-10 on the training rows of the fit.  oracle_model.logreg_l1_fit (the CDN
loop) is not used: on 261 x 40 counts at C = 1 it does not end in minutes.
Lasso / elastic-net yardstick: enet_descent below, cyclic coordinate descent of the centred problem in f64 with the kernel's
objective  1/2 |y - Xw - b|^2 + alpha l1_ratio n |w|_1 + 1/2 alpha (1 - l1_ratio) n |w|^2, run until its KKT residual is
below 1e-12 alpha n and certified by enet_certificate.

The constant-1 column of a design and the penalised intercept are the same column: only the SUM of their two coefficients
is unique (|u| + |v| >= |u + v|), so every comparison of coefficients folds the constant column's pattern into the intercept."""
import functools
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "phenotypeseeker_amd", "csrc")
CONST_COL, ZERO_COL, DUP_COL = 3, 5, 7      # with p > 9 (l2_restated.design's rule); the duplicate of DUP_COL is the last column
L1_LDS_MAX = 160 * 1024 - 8192              # PSK_L1_LDS_MAX of solver_l1_plan.h; test_l1_float_host.py holds it to the header
SV_LDS_N = 4096                             # solver_common.h, likewise
BITS_MAX_N = 4096                           # a 0/1 design of up to this many samples takes the bit-packed kernels
ARBITER_ROUNDS = 400
KKT_MAX = 1e-10
SUPPORT_MIN, SUPPORT_MAX = 3, 80


def design(n, p, counts, seed, density=0.4):
    """(X[n][p] float32, y01[n] int32).  Twelve random 0/1 base columns of the given density; every column of X is one of
    them with density / 5 of its cells flipped (base ^ noise, 0.4 and 0.08 as in test_l1_logreg_three_forms_of_the_descent_agree).
    counts: every cell times max(1, Poisson(2)), then five cells set to 200.  p > 9: a constant-1 column, an all-zero column
    and an exact duplicate pair.  y01: base column 0 with 15 % of the labels flipped."""
    rng = np.random.default_rng([seed, n, p, int(bool(counts))])
    base = rng.random((n, 12)) < density
    X = (base[:, rng.integers(0, 12, p)] ^ (rng.random((n, p)) < density / 5)).astype(np.float32)
    if counts:
        X *= np.maximum(1, rng.poisson(2, (n, p))).astype(np.float32)
        X[rng.integers(0, n, 5), rng.integers(0, p, 5)] = 200.0
    if p > 9:
        X[:, CONST_COL] = 1.0
        X[:, ZERO_COL] = 0.0
        X[:, p - 1] = X[:, DUP_COL]
    y = (base[:, 0] ^ (rng.random(n) < 0.15)).astype(np.int32)
    return X, y


def target(X, seed):
    """A continuous phenotype for the Lasso cases: up to six columns times normal weights plus N(0, 0.3)."""
    rng = np.random.default_rng([seed, 77])
    n, p = X.shape
    cols = rng.choice(p, min(6, p), replace=False)
    return X[:, cols].astype(np.float64) @ rng.standard_normal(len(cols)) + 0.3 * rng.standard_normal(n)


def placement(n, p, lds_max=L1_LDS_MAX, feature_bytes=None):
    """(f_lds, s_lds) of logreg_newglmnet_kernel as psk_logreg_l1_fit chooses them: the five feature arrays take 40 (p + 1)
    bytes, the five sample arrays 40 n; both in LDS when they fit together, else the sample arrays, else the feature arrays."""
    fbytes = 5 * (p + 1) * 8 if feature_bytes is None else feature_bytes(p)
    sbytes = 5 * n * 8
    if fbytes + sbytes <= lds_max:
        return 1, 1
    if sbytes <= lds_max:
        return 0, 1
    if fbytes <= lds_max:
        return 1, 0
    return 0, 0


def lasso_use_lds(n, sv_lds_n=SV_LDS_N):
    """lasso_float_fit's rule: the residual in LDS up to 2 SV_LDS_N samples."""
    return 1 if n <= 2 * sv_lds_n else 0


def header_constants():
    """{PSK_L1_LDS_MAX, feature_bytes (a function of p), SV_LDS_N} as csrc/solver_l1_plan.h and solver_common.h spell them,
    and the two lines of solver.hip that apply them."""
    def text(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def arith(expr, **names):
        expr = expr.replace("(size_t)", "")
        assert re.fullmatch(r"[0-9p+\-*/() ]+", expr), expr
        return eval(expr.replace("/", "//"), {"__builtins__": {}}, names)
    plan, common, solver = text("solver_l1_plan.h"), text("solver_common.h"), text("solver.hip")
    lds_max = re.search(r"constexpr size_t PSK_L1_LDS_MAX = ([^;]+);", plan).group(1)
    fbytes = re.search(r"inline size_t psk_l1_feature_bytes\(int p\) \{ return ([^;]+); \}", plan).group(1)
    sv = re.search(r"constexpr int SV_LDS_N = ([^;]+);", common).group(1)
    return {"lds_max": arith(lds_max), "feature_bytes": lambda p: arith(fbytes, p=p), "SV_LDS_N": arith(sv),
            "host_rules": ("const size_t fbytes = psk_l1_feature_bytes(p), sbytes = 5 * n_state * 8;" in solver
                           and "if (fbytes + sbytes <= PSK_L1_LDS_MAX) f_lds = s_lds = 1;" in solver
                           and "else if (sbytes <= PSK_L1_LDS_MAX) s_lds = 1;" in solver
                           and "else if (fbytes <= PSK_L1_LDS_MAX) f_lds = 1;" in solver
                           and "const bool binary = n <= 4096 && design_is_binary(X, (size_t)n * p);" in solver
                           and "const int use_lds = n <= 2 * SV_LDS_N ? 1 : 0;" in solver)}


# The logistic cases: each the smallest shape that lands in its placement.  place: (f_lds, s_lds) of the float kernel, None:
# the bit-packed kernels.  A launch holds the fits Cs x held (held -1: the refit on every row); fold = i % folds.
# tight: the case runs again at tol = 1e-12.  The Cs are chosen so that every fit's certified support has 3..80 patterns
# (test_l1_float_host.py); on the tail shapes, which have fewer than three columns to offer, every pattern there is.
CASES = {
    "A": dict(n=261, p=40, counts=True, density=0.4, seed=1, place=(1, 1), Cs=(0.03, 0.1, 0.3, 1.0, 10.0), folds=5,
              held=(0, 1, 2, 3, 4, -1), tight=True),
    "A-tail-65x3": dict(n=65, p=3, counts=True, density=0.4, seed=1, place=(1, 1), Cs=(0.3, 1.0, 10.0), folds=3, held=(-1, 0, 1),
                        tight=True),
    "A-tail-7x3": dict(n=7, p=3, counts=True, density=0.4, seed=15, place=(1, 1), Cs=(3.0, 10.0, 30.0), folds=3, held=(-1, 0, 1),
                       tight=True),
    "A-tail-64x1": dict(n=64, p=1, counts=True, density=0.4, seed=1, place=(1, 1), Cs=(0.3, 1.0, 10.0), folds=3, held=(-1, 0, 1),
                        tight=True),
    "A-edge": dict(n=200, p=3690, counts=True, density=0.05, seed=1, place=(1, 1), Cs=(0.1, 0.3), folds=1, held=(-1,), tight=False),
    "B-edge": dict(n=200, p=3691, counts=True, density=0.05, seed=1, place=(0, 1), Cs=(0.1, 0.3), folds=1, held=(-1,), tight=False,
                   widen="A-edge"),
    "B": dict(n=130, p=3800, counts=True, density=0.05, seed=1, place=(0, 1), Cs=(0.1, 0.3, 1.0), folds=3, held=(-1, 1), tight=False),
    "C": dict(n=3892, p=12, counts=True, density=0.4, seed=1, place=(1, 0), Cs=(0.01, 0.1, 1.0), folds=3, held=(-1, 1), tight=True),
    "C-bin": dict(n=4097, p=20, counts=False, density=0.4, seed=1, place=(1, 0), Cs=(0.05, 0.1, 1.0), folds=1, held=(-1,), tight=True),
    "C-bin-4096": dict(n=4096, p=20, counts=False, density=0.4, seed=1, place=None, Cs=(0.05, 0.1, 1.0), folds=1, held=(-1,),
                       tight=True, head_of="C-bin"),
    "D": dict(n=3892, p=3892, counts=True, density=0.02, seed=1, place=(0, 0), Cs=(0.02,), folds=3, held=(-1, 1), tight=False,
              two_fits=True),
    # 600 fits in one launch (test e): 20 C x (5 folds + refit), five times over
    "E": dict(n=65, p=30, counts=True, density=0.4, seed=1, place=(1, 1), Cs=tuple(float(c) for c in np.geomspace(0.1, 10.0, 20)),
              folds=5, held=(0, 1, 2, 3, 4, -1), tight=False),
}
TABLE = ("A", "A-tail-65x3", "A-tail-7x3", "A-tail-64x1", "A-edge", "B-edge", "B", "C", "C-bin", "C-bin-4096", "D")

# The Lasso / elastic-net cases (test f): (n, p, counts) -> use_lds; 3 alphas x (refit + one fold of four)
LASSO_CASES = {"8192x6 counts": dict(n=8192, p=6, counts=True, seed=1, use_lds=1),
               "8193x6 counts": dict(n=8193, p=6, counts=True, seed=1, use_lds=0),
               "8193x6 0/1": dict(n=8193, p=6, counts=False, seed=1, use_lds=0)}
LASSO_ALPHAS, LASSO_HELD, LASSO_FOLDS = (0.01, 0.1, 1.0), (-1, 1), 4
LASSO_TOL, LASSO_MAX_ITER = 1e-10, 10000


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X float32, y01 int32, fold int32, fit_param f64, fit_fold int32) of a logistic case; the arrays are read-only."""
    c = CASES[name]
    if "head_of" in c:          # the first rows of its neighbour
        X, y = (a[:c["n"]].copy() for a in case_data(c["head_of"])[:2])
    elif "widen" in c:          # its neighbour's rows with one more column
        X0, y = case_data(c["widen"])[:2]
        extra = design(c["n"], 12, c["counts"], c["seed"] + 1000, c["density"])[0][:, :c["p"] - X0.shape[1]]
        X = np.hstack([X0, extra])
    else:
        X, y = design(c["n"], c["p"], c["counts"], c["seed"], c["density"])
    assert X.shape == (c["n"], c["p"]) and X.dtype == np.float32
    fold = (np.arange(c["n"]) % c["folds"]).astype(np.int32)
    if c.get("two_fits"):
        fp, ff = [c["Cs"][0]] * len(c["held"]), list(c["held"])
    else:
        fp, ff = [C for C in c["Cs"] for _ in c["held"]], [h for _ in c["Cs"] for h in c["held"]]
    out = (X, y, fold, np.array(fp, np.float64), np.array(ff, np.int32))
    for a in out:
        a.setflags(write=False)
    return out


def route_is_float(name):
    X = case_data(name)[0]
    return X.shape[0] > BITS_MAX_N or bool(np.any((X != 0) & (X != 1)))


@functools.lru_cache(maxsize=None)
def certified(name):
    """The arbiter's optimum of every fit of a case, from the zero hint, on the fit's training rows: a tuple of its dicts,
    computed once per process."""
    from oracle import oracle_model as OM
    X, y, fold, fp, ff = case_data(name)
    done, out = {}, []
    for C, h in zip(fp, ff):
        if (C, h) not in done:
            tr = fold != h
            done[(C, h)] = OM.logreg_l1_arbiter(X[tr], y[tr], float(C), np.zeros(X.shape[1]), 0.0, max_rounds=ARBITER_ROUNDS)
        out.append(done[(C, h)])
    return tuple(out)


def const_group(X_train, arb):
    """index of the arbiter's pattern that is the constant-1 column on these rows (the intercept's twin), or None"""
    for j in range(X_train.shape[1]):
        if np.all(X_train[:, j] == 1.0):
            return int(arb["group"][j])
    return None


def folded(X_train, arb, coef=None, icpt=None):
    """(pattern sums, intercept) with the constant column's pattern folded into the intercept: of the arbiter's optimum, or
    of a solver's (coef, icpt)."""
    if coef is None:
        sums, b = arb["w_groups"].copy(), arb["b"]
    else:
        sums, b = np.zeros(len(arb["w_groups"])), float(icpt)
        np.add.at(sums, arb["group"], coef)
    g = const_group(X_train, arb)
    if g is not None:
        b += sums[g]
        sums[g] = 0.0
    return sums, b


def support_size(X_train, arb):
    """distinct patterns of the certified support, the intercept / constant column counting as one"""
    sums, b = folded(X_train, arb)
    return int((sums != 0).sum() + (b != 0))


def expand(arb, p):
    """a coefficient vector of the arbiter's optimum: every pattern's sum on its first column"""
    w, seen = np.zeros(p), set()
    for j, g in enumerate(arb["group"]):
        if g not in seen:
            seen.add(g)
            w[j] = arb["w_groups"][g]
    return w


def stop_rule_violation(X, ypm, fold, C, held, coef, icpt):
    """(||violation||_1 at the point, ||violation||_1 at w = 0, min(#pos, #neg) / l) of liblinear's stopping rule, for the
    true gradient on the fit's training rows"""
    tr = fold != held
    A = np.hstack([X[tr].astype(np.float64), np.ones((tr.sum(), 1))])
    yt = ypm[tr]

    def viol(th):
        g = -C * (A.T @ (yt / (1.0 + np.exp(yt * (A @ th)))))
        return np.where(th > 0, np.abs(g + 1), np.where(th < 0, np.abs(g - 1), np.maximum(0, np.maximum(-(g + 1), g - 1)))).sum()
    th = np.append(coef, icpt)
    return viol(th), viol(np.zeros_like(th)), max(min((yt > 0).sum(), (yt < 0).sum()), 1) / tr.sum()


def stop_rule_holds(X, ypm, fold, fp, ff, coef, icpt, iters, fits, tol=1e-4, slack=1.5):
    """liblinear's stopping rule, for the TRUE gradient at the returned point: ||violation||_1 <= tol min(#pos, #neg) / l x
    the violation at w = 0 (x slack: the solver tests it on its own accumulated quantities).  Returns the largest
    violation / bound."""
    worst = 0.0
    for j in fits:
        v, v0, frac = stop_rule_violation(X, ypm, fold, fp[j], ff[j], coef[j], icpt[j])
        bound = slack * tol * frac * v0 + 1e-9
        worst = max(worst, v / bound)
        assert v <= bound, (j, fp[j], iters[j])
    return worst


def objectives(X, ypm, fold, fp, ff, coef, icpt):
    Z = X.astype(np.float64) @ coef.T + icpt[None, :]
    return np.array([np.abs(coef[j]).sum() + abs(icpt[j]) + fp[j] * np.logaddexp(0.0, -ypm[fold != ff[j]] * Z[fold != ff[j], j]).sum()
                     for j in range(len(fp))])


def judge_logit(what, X, y, fold, fp, ff, coef, icpt, iters, arbs, tol=1e-4):
    """What a launch at the reference's tolerance (tol 1e-4, max_iter 1000) owes the arbiter: fewer than 200 Newton steps,
    liblinear's stop rule for the true gradient (slack 1.5), the objective in [opt (1 - 1e-9), 1.01 opt].  Returns
    (largest violation / bound, largest (objective / opt - 1) / 0.01, most Newton steps)."""
    ypm = 2.0 * np.asarray(y, dtype=np.float64) - 1.0
    assert np.all(np.isfinite(coef)) and np.all(np.isfinite(icpt)), what
    assert iters.max() < 200, (what, iters.tolist())
    stop = stop_rule_holds(X, ypm, fold, fp, ff, coef, icpt, iters, range(len(fp)), tol=tol)
    obj = objectives(X, ypm, fold, fp, ff, coef, icpt)
    gap = 0.0
    for j, a in enumerate(arbs):
        opt = a["objective"]
        assert opt * (1 - 1e-9) <= obj[j] <= opt * 1.01, (what, j, fp[j], ff[j], obj[j] / opt - 1)
        gap = max(gap, (obj[j] / opt - 1) / 0.01)
    return stop, gap, int(iters.max())


def judge_tight(what, X, y, fold, fp, ff, coef, icpt, iters, arbs):
    """What a launch at tol = 1e-12, max_iter 5000 owes the arbiter -- the bounds of
    test_l1_logreg_solver_reaches_liblinear_optimum: pattern sums rtol 1e-6, the same support with exact zeros off it, the
    intercept rel 1e-6 (the constant column folded into it), the linear predictor on the training rows rtol 1e-6 / atol 1e-12,
    the objective rel 1e-12, fewer than 5000 steps.  Every fit's figures are printed before any is refused.  Returns the largest
    (coefficient, predictor, objective) error / bound and the most Newton steps."""
    import pytest
    from oracle import oracle_model as OM
    worst_c = worst_o = worst_l = 0.0
    failed = []
    for j, a in enumerate(arbs):
        tr = fold != ff[j]
        Xt = X[tr].astype(np.float64)
        want, bw = folded(Xt, a)
        got, bg = folded(Xt, a, coef[j], icpt[j])
        nz = want != 0
        ce = float((np.abs(got - want)[nz] / (1e-6 * np.abs(want[nz]))).max()) if nz.any() else 0.0
        if bw != 0:
            ce = max(ce, abs(bg - bw) / (1e-6 * abs(bw)))
        lerr = np.abs(Xt @ coef[j] + icpt[j] - a["linpred"]) / (1e-12 + 1e-6 * np.abs(a["linpred"]))
        i = int(np.argmax(lerr))
        obj = OM.logreg_l1_objective(Xt, y[tr], coef[j], icpt[j], float(fp[j]))
        oe = abs(obj / a["objective"] - 1) / 1e-12
        worst_c, worst_l, worst_o = max(worst_c, ce), max(worst_l, float(lerr[i])), max(worst_o, oe)
        tag = (what, "fit %d" % j, "C=%g" % fp[j], "held=%d" % ff[j], "steps=%d" % iters[j], "coefficient error / bound %.3g" % ce,
               "predictor error / bound %.3g where the predictor is %.3g" % (lerr[i], a["linpred"][i]), "objective error / bound %.3g" % oe)
        try:
            assert iters[j] < 5000, tag
            assert np.array_equal(got == 0, want == 0), tag
            assert np.allclose(got, want, rtol=1e-6, atol=0), tag
            assert bg == pytest.approx(bw, rel=1e-6, abs=0), tag
            assert np.allclose(Xt @ coef[j] + icpt[j], a["linpred"], rtol=1e-6, atol=1e-12), tag
            assert obj == pytest.approx(a["objective"], rel=1e-12), tag
        except AssertionError as e:
            print("MISSED", e)
            failed.append(tag)
    assert not failed, failed
    return worst_c, worst_l, worst_o, int(iters.max())


def garbage(X, y, fold, held, seed=5):
    """(X, y) with the rows of fold `held` overwritten: finite counts up to 1e6, the labels flipped."""
    rng = np.random.default_rng(seed)
    X2, y2 = X.copy(), y.copy()
    rows = np.nonzero(fold == held)[0]
    X2[rows] = rng.integers(0, 1000001, (len(rows), X.shape[1])).astype(X.dtype)
    X2[rows[0], 0] = 1e6
    y2[rows] = 1 - y2[rows] if y.dtype.kind in "iu" else -y2[rows] + 1e6
    return X2, y2


# ---------------------------------------------------------------------------------------------------------------------------
# Lasso and the elastic net
# ---------------------------------------------------------------------------------------------------------------------------
def enet_descent(X, y, alpha, l1_ratio, max_sweeps=100000):
    """X, y: the training rows.  Cyclic coordinate descent of the centred problem in f64 until the KKT residual is below
    1e-12 alpha n.  Returns (coef, intercept, sweeps)."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, p = X.shape
    mean, ym = X.mean(axis=0), y.mean()
    Xc, yc = np.asfortranarray(X - mean), y - ym
    l1, beta = alpha * l1_ratio * n, alpha * (1.0 - l1_ratio) * n
    nrm = (Xc ** 2).sum(axis=0)
    cols = [j for j in range(p) if nrm[j] > 1e-12]
    w, r = np.zeros(p), yc.copy()
    for sweep in range(1, max_sweeps + 1):
        for j in cols:
            rho = Xc[:, j] @ r + nrm[j] * w[j]
            mag = abs(rho) - l1
            nw = (mag if rho > 0 else -mag) / (nrm[j] + beta) if mag > 0.0 else 0.0
            if nw != w[j]:
                r -= (nw - w[j]) * Xc[:, j]
                w[j] = nw
        if sweep % 8 == 0:
            r = yc - Xc @ w
            g = Xc.T @ r - beta * w
            res = np.where(w != 0, np.abs(g - l1 * np.sign(w)), np.maximum(np.abs(g) - l1, 0.0))
            if res[cols].max(initial=0.0) < 1e-12 * alpha * n:
                break
    else:
        raise AssertionError("no convergence in %d sweeps" % max_sweeps)
    return w, float(ym - mean @ w), sweep


def enet_certificate(X, y, w, alpha, l1_ratio):
    """The f64 KKT conditions of (w, the unpenalised intercept at its optimum) on the rows given, r = y_c - X_c w, g = X_c'r -
    beta w, l1 = alpha l1_ratio n:  off the support |g_j| <= l1 (1 + 1e-9); on it g_j = sign(w_j) l1 to 1e-9 relative; and
    scikit-learn's duality gap (enet_restated) below 1e-13 y'y -- a thousandth of where the device stops at tol = 1e-10, a
    thousand times the rounding of the gap's own sums.  Returns (largest |g| / l1 off the support, largest relative defect
    on it, gap / y'y)."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = X.shape[0]
    Xc, yc = X - X.mean(axis=0), y - y.mean()
    l1, beta = alpha * l1_ratio * n, alpha * (1.0 - l1_ratio) * n
    r = yc - Xc @ w
    g = Xc.T @ r - beta * w
    off = float((np.abs(g[w == 0]) / l1).max(initial=0.0))
    on = float((np.abs(g[w != 0] - np.sign(w[w != 0]) * l1) / l1).max(initial=0.0))
    dual, rr = np.abs(g).max(), r @ r
    c = l1 / dual if dual > l1 else 1.0
    gap = (0.5 * rr * (1 + c * c) if dual > l1 else rr) + l1 * np.abs(w).sum() - c * (r @ yc) + 0.5 * beta * (1 + c * c) * (w @ w)
    assert off <= 1 + 1e-9 and on <= 1e-9 and gap <= 1e-13 * (yc @ yc), (off, on, gap / (yc @ yc))
    return off, on, float(gap / (yc @ yc))


@functools.lru_cache(maxsize=None)
def lasso_data(name):
    """(X float32, y f64, fold int32, fit_alpha, fit_fold) of a Lasso case, read-only."""
    c = LASSO_CASES[name]
    X = design(c["n"], c["p"], c["counts"], c["seed"])[0]
    y = target(X, c["seed"])
    fold = (np.arange(c["n"]) % LASSO_FOLDS).astype(np.int32)
    fa = np.array([a for a in LASSO_ALPHAS for _ in LASSO_HELD], np.float64)
    ff = np.array([h for _ in LASSO_ALPHAS for h in LASSO_HELD], np.int32)
    out = (X, y, fold, fa, ff)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lasso_certified(name, l1_ratio):
    """((coef, intercept), ...) of every fit of a Lasso case by enet_descent, each certified."""
    X, y, fold, fa, ff = lasso_data(name)
    out = []
    for alpha, h in zip(fa, ff):
        tr = fold != h
        w, b, _ = enet_descent(X[tr], y[tr], float(alpha), l1_ratio)
        enet_certificate(X[tr], y[tr], w, float(alpha), l1_ratio)
        out.append((w, b))
    return tuple(out)


def judge_lasso(what, coef, icpt, iters, refs, max_iter=LASSO_MAX_ITER):
    """The bounds of enet_restated.judge without the sweep count (the yardstick is the optimum, not scikit-learn's path): every
    coefficient within 1e-6 of the largest, the same support, the intercept to rel 1e-6 / abs 1e-9; the descent ended before
    max_iter.  Returns the largest coefficient error / bound."""
    import pytest
    worst = 0.0
    for j, (w, b) in enumerate(refs):
        tag = (what, j, int(iters[j]))
        assert iters[j] < max_iter, tag
        scale = max(np.abs(w).max(), 1e-300)
        err = np.abs(coef[j] - w).max()
        worst = max(worst, err / (1e-6 * scale))
        assert err <= 1e-6 * scale, tag + (err / scale,)
        assert np.array_equal(coef[j] != 0, w != 0), tag
        assert icpt[j] == pytest.approx(b, rel=1e-6, abs=1e-9), tag
    return worst
