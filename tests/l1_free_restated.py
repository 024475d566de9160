"""L1 logistic regression with a FREE intercept (psk_logreg_l1_free_fit, `--logreg_solver saga`): the objective, liblinear's
stop rule for it, an f64 arbiter and the bounds that tests/test_l1_free_host.py (CPU) and tests/test_gpu_l1_free.py (device)
share.  No test functions here.  Designs, cases and fit lists are those of tests/l1_float_cases.py (three fits of one case
at another C: C_CHANGED).

    objective   ||w||_1 + C sum log(1 + exp(-y (w.x + b)))          (liblinear's adds |b|)

Yardstick: free_arbiter below, oracle_model.logreg_l1_arbiter with the intercept always in the support and without a sign
term: active-set damped Newton on the collapsed column patterns, from a ZERO hint, certified by its own KKT residual below
l1_float_cases.KKT_MAX.  The constant-1 column of a design is the intercept's twin: under a free intercept its pattern has
|gradient| = |d/db| = 0 < 1 at the optimum and comes out at exactly 0 -- the opposite of the folding that the penalised
comparisons need (l1_float_cases.folded), so nothing is folded here.

The bounds are l1_float_cases.judge_logit and judge_tight, restated for this objective."""
import functools

import numpy as np

import l1_float_cases as L

KKT_MAX = L.KKT_MAX
ARBITER_ROUNDS = L.ARBITER_ROUNDS

# The float-kernel cases of the device tests (the issue's table) and the one bit-packed neighbour of the seam at 4,096 samples
FLOAT_CASES = ("A-tail-7x3", "A-tail-64x1", "A-tail-65x3", "A", "A-edge", "B-edge", "C", "C-bin")
SEAM_CASE = "C-bin-4096"


# Fits whose C is changed because free_arbiter does not certify them in ARBITER_ROUNDS at the C of l1_float_cases: 7 x 3 counts
# with fold 0 held out leaves four rows, one of them negative, separable by column 0 alone; at C = 3, 10, 30 the active set
# cycles (column 1, gradient 99.5, enters and is thrown out again) and the KKT residual stays at 99.5.  At C = 0.1, 0.3, 1 it is
# below 2e-15.  The refit and the fits that hold fold 1 out keep C = 3, 10, 30 (w.x beyond 709 on one row at C = 30).
C_CHANGED = {"A-tail-7x3": {(3.0, 0): 0.1, (10.0, 0): 0.3, (30.0, 0): 1.0}}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """l1_float_cases.case_data with the fits of C_CHANGED at their changed C; read-only arrays."""
    X, y, fold, fp, ff = L.case_data(name)
    if name in C_CHANGED:
        fp = np.array([C_CHANGED[name].get((float(C), int(h)), float(C)) for C, h in zip(fp, ff)], np.float64)
        fp.setflags(write=False)
    return X, y, fold, fp, ff


def free_objective(X, y01, w, b, C):
    ypm = 2.0 * np.asarray(y01, dtype=np.float64) - 1.0
    return np.abs(w).sum() + C * np.logaddexp(0.0, -ypm * (np.asarray(X, dtype=np.float64) @ w + b)).sum()


def objectives(X, ypm, fold, fp, ff, coef, icpt):
    Z = X.astype(np.float64) @ coef.T + icpt[None, :]
    return np.array([np.abs(coef[j]).sum() + fp[j] * np.logaddexp(0.0, -ypm[fold != ff[j]] * Z[fold != ff[j], j]).sum()
                     for j in range(len(fp))])


def one_class_fits(y, fold, ff):
    """indices of the fits whose training rows hold one class: no minimiser, refused by the entry point"""
    return [j for j, h in enumerate(ff) if len(np.unique(y[fold != h])) < 2]


def free_arbiter(X, y01, C, max_rounds=ARBITER_ROUNDS):
    """The exact optimum of the free-intercept objective on the rows given: oracle_model.logreg_l1_arbiter's scheme from a zero
    hint.  Identical columns are collapsed (their coefficient SUM is what is unique); the intercept is always in the support
    and has no sign term; the smooth problem  s.theta_A + C sum log(1 + exp(-y A theta))  is solved on the support by damped
    Newton steps until its gradient is below 2e-14 (or no step improves it); then the most violated coordinate off the
    support (|grad| > 1) joins it and the solve repeats.  Returns dict(w_groups, group, b, kkt, objective, linpred)."""
    from oracle import oracle_model as OM
    Xu, group = OM.collapse_columns(X)
    n, pu = Xu.shape
    A = np.hstack([Xu, np.ones((n, 1))])
    ypm = 2.0 * np.asarray(y01, dtype=np.float64) - 1.0
    assert len(np.unique(ypm)) == 2, "one class: the free intercept has no minimiser"
    pen = np.append(np.ones(pu), 0.0)
    th = np.zeros(pu + 1)
    act = np.zeros(pu + 1, dtype=bool)
    act[pu] = True
    sgn = np.zeros(pu + 1)

    def grad_loss(t):
        s = 1.0 / (1.0 + np.exp(ypm * (A @ t)))
        return -C * (A.T @ (ypm * s)), s

    def obj(t):
        return np.abs(t[:pu]).sum() + C * np.logaddexp(0.0, -ypm * (A @ t)).sum()
    for _ in range(max_rounds):
        idx = np.nonzero(act)[0]
        for _it in range(200):
            g, s = grad_loss(th)
            gs = g[idx] + sgn[idx]
            if np.abs(gs).max() < 2e-14:
                break
            Aa = A[:, idx]
            H = C * (Aa.T * (s * (1.0 - s))) @ Aa
            try:
                d = -np.linalg.solve(H, gs)
                if not np.all(np.isfinite(d)):
                    raise np.linalg.LinAlgError
            except np.linalg.LinAlgError:
                d = -np.linalg.lstsq(H, gs, rcond=1e-13)[0]
            t = 1.0
            cross = (th[idx] + d) * sgn[idx] < 0        # (never the intercept: its sign term is 0)
            if cross.any():
                t = min(1.0, float(np.min(-th[idx][cross] / d[cross])))
            f0 = obj(th)
            while t > 1e-14:
                cand = th.copy()
                cand[idx] += t * d
                if obj(cand) <= f0 + 1e-4 * t * (gs @ d) or t * np.abs(d).max() < 1e-15:
                    break
                t *= 0.5
            th = cand
            hit = idx[(np.abs(th[idx]) < 1e-15 * max(1.0, np.abs(th).max())) & (idx != pu)]
            if hit.size and cross.any():
                th[hit] = 0.0
                act[hit] = False
                idx = np.nonzero(act)[0]
        g, _ = grad_loss(th)
        viol_in = (~act) & (np.abs(g) > 1.0 + 1e-12)
        if not viol_in.any():
            break
        j = int(np.argmax(np.where(viol_in, np.abs(g), 0.0)))
        act[j] = True
        sgn[j] = -np.sign(g[j])
    g, _ = grad_loss(th)
    kkt = max(float(np.abs(g[act] + pen[act] * np.sign(th[act])).max()),
              float(np.maximum(np.abs(g[~act]) - 1.0, 0.0).max()) if (~act).any() else 0.0)
    return {"w_groups": th[:pu].copy(), "group": group, "b": float(th[pu]), "kkt": kkt, "objective": obj(th), "linpred": A @ th}


@functools.lru_cache(maxsize=None)
def certified(name):
    """The free arbiter's optimum of every fit of a case of l1_float_cases, on the fit's training rows, once per process."""
    X, y, fold, fp, ff = case_data(name)
    done, out = {}, []
    for C, h in zip(fp, ff):
        if (C, h) not in done:
            tr = fold != h
            done[(C, h)] = free_arbiter(X[tr], y[tr], float(C))
        out.append(done[(C, h)])
    return tuple(out)


def const_group(X_train, arb):
    return L.const_group(X_train, arb)


def stop_rule_violation(X, ypm, fold, C, held, coef, icpt):
    """(||violation||_1 at the point, ||violation||_1 at w = 0, b = 0, min(#pos, #neg) / l) of liblinear's stopping rule with
    a free intercept, for the true gradient on the fit's training rows: the intercept's violation is |d/db|."""
    tr = fold != held
    A = np.hstack([X[tr].astype(np.float64), np.ones((tr.sum(), 1))])
    yt = ypm[tr]
    p = A.shape[1] - 1

    def viol(th):
        g = -C * (A.T @ (yt / (1.0 + np.exp(yt * (A @ th)))))
        v = np.where(th > 0, np.abs(g + 1), np.where(th < 0, np.abs(g - 1), np.maximum(0, np.maximum(-(g + 1), g - 1))))
        return v[:p].sum() + abs(g[p])
    th = np.append(coef, icpt)
    return viol(th), viol(np.zeros_like(th)), max(min((yt > 0).sum(), (yt < 0).sum()), 1) / tr.sum()


def stop_rule_holds(X, ypm, fold, fp, ff, coef, icpt, iters, fits, tol=1e-4, slack=1.5):
    """l1_float_cases.stop_rule_holds for the free objective; returns the largest violation / bound."""
    worst = 0.0
    for j in fits:
        v, v0, frac = stop_rule_violation(X, ypm, fold, fp[j], ff[j], coef[j], icpt[j])
        bound = slack * tol * frac * v0 + 1e-9
        worst = max(worst, v / bound)
        assert v <= bound, (j, fp[j], iters[j], v / bound)
    return worst


def judge_logit(what, X, y, fold, fp, ff, coef, icpt, iters, arbs, tol=1e-4):
    """l1_float_cases.judge_logit for the free objective: fewer than 200 Newton steps, the stop rule for the true gradient
    (slack 1.5), the objective in [opt (1 - 1e-9), 1.01 opt].  arbs: None to leave the arbiter out (the large bit-packed
    designs).  Returns (largest violation / bound, largest (objective / opt - 1) / 0.01, most Newton steps)."""
    ypm = 2.0 * np.asarray(y, dtype=np.float64) - 1.0
    assert np.all(np.isfinite(coef)) and np.all(np.isfinite(icpt)), what
    assert iters.max() < 200, (what, iters.tolist())
    stop = stop_rule_holds(X, ypm, fold, fp, ff, coef, icpt, iters, range(len(fp)), tol=tol)
    gap = 0.0
    if arbs is not None:
        obj = objectives(X, ypm, fold, fp, ff, coef, icpt)
        for j, a in enumerate(arbs):
            opt = a["objective"]
            assert opt * (1 - 1e-9) <= obj[j] <= opt * 1.01, (what, j, fp[j], ff[j], obj[j] / opt - 1)
            gap = max(gap, (obj[j] / opt - 1) / 0.01)
    return stop, gap, int(iters.max())


def judge_tight(what, X, y, fold, fp, ff, coef, icpt, iters, arbs):
    """l1_float_cases.judge_tight for the free objective (tol = 1e-12, max_iter 5000): the same support with exact zeros off
    it -- the constant column's pattern among them --, pattern sums and intercept rtol 1e-6, the training predictor rtol
    1e-6 / atol 1e-12, the objective rel 1e-12, fewer than 5000 steps.  Every fit's figures are printed before any is
    refused.  Returns the largest (coefficient, predictor, objective) error / bound and the most Newton steps."""
    import pytest
    worst_c = worst_o = worst_l = 0.0
    failed = []
    for j, a in enumerate(arbs):
        tr = fold != ff[j]
        Xt = X[tr].astype(np.float64)
        want, bw = a["w_groups"], a["b"]
        got, bg = np.zeros(len(want)), float(icpt[j])
        np.add.at(got, a["group"], coef[j])
        g = const_group(Xt, a)
        nz = want != 0
        ce = float((np.abs(got - want)[nz] / (1e-6 * np.abs(want[nz]))).max()) if nz.any() else 0.0
        if bw != 0:
            ce = max(ce, abs(bg - bw) / (1e-6 * abs(bw)))
        lerr = np.abs(Xt @ coef[j] + icpt[j] - a["linpred"]) / (1e-12 + 1e-6 * np.abs(a["linpred"]))
        i = int(np.argmax(lerr))
        obj = free_objective(Xt, y[tr], coef[j], icpt[j], float(fp[j]))
        oe = abs(obj / a["objective"] - 1) / 1e-12
        worst_c, worst_l, worst_o = max(worst_c, ce), max(worst_l, float(lerr[i])), max(worst_o, oe)
        tag = (what, "fit %d" % j, "C=%g" % fp[j], "held=%d" % ff[j], "steps=%d" % iters[j], "coefficient error / bound %.3g" % ce,
               "predictor error / bound %.3g where the predictor is %.3g" % (lerr[i], a["linpred"][i]), "objective error / bound %.3g" % oe)
        try:
            assert iters[j] < 5000, tag
            assert g is None or (want[g] == 0.0 and got[g] == 0.0), tag + ("the constant column's pattern",)
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


def bits_design(n, p=250):
    """The design of test_gpu_parity.py::test_l1_logreg_three_forms_of_the_descent_agree (p = 250 there) and its five fits."""
    rng = np.random.default_rng(n)
    base = rng.random((n, 12)) < 0.4
    X = (base[:, rng.integers(0, 12, p)] ^ (rng.random((n, p)) < 0.08)).astype(np.float32)
    y = (base[:, 0] ^ (rng.random(n) < 0.15)).astype(np.int32)
    fold = (np.arange(n) % 3).astype(np.int32)
    return X, y, fold, np.array([0.01, 0.01, 0.1, 1.0, 1.0], np.float64), np.array([-1, 0, 1, 2, -1], np.int32)


@functools.lru_cache(maxsize=None)
def bits_certified(n, p):
    X, y, fold, fp, ff = bits_design(n, p)
    return tuple(free_arbiter(X[fold != h], y[fold != h], float(C)) for C, h in zip(fp, ff))
