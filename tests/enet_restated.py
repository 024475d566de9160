"""scikit-learn 1.7.2's ElasticNet(tol, max_iter).fit on a dense design restated in NumPy, f64: the CPU yardstick of
psk_enet_fit (include/psk.h, f14; csrc/solver.hip, csrc/solver_lasso.hip), the designs and the reader of
tests/golden/enet_kat.npz (tools/gen_enet_golden.py), and a stand-in for the engine in host tests.

enet_coordinate_descent on the problem centred over the training rows (X - column means, y - mean), n training rows,
l1 = alpha l1_ratio n, l2 = alpha (1 - l1_ratio) n, w = 0 and R = y at the start; a sweep visits the columns in order and
skips those whose centred norm is 0:
    tmp = X_j'R + w_j |X_j|^2,   w_j <- sign(tmp) max(|tmp| - l1, 0) / (|X_j|^2 + l2),   R -= (w_j - old w_j) X_j  at once.
After a sweep with w_max == 0 or d_w_max / w_max < tol, or the last sweep allowed, the duality gap is evaluated:
    XtA = X'R - l2 w,  dual = max|XtA|,  c = l1 / dual if dual > l1 else 1,
    gap = (dual > l1 ? 1/2 R'R (1 + c^2) : R'R) + l1 ||w||_1 - c R'y + 1/2 l2 (1 + c^2) w'w,
and the descent stops when gap < tol y'y.  intercept = mean y - sum_k mean_k w_k; n_iter = sweeps made.
What differs from the device is the order of every sum, nothing else; so a stop decision that hangs on the last bits of a sum
could fall a sweep apart.  The fixture holds only cases in which none does (MARGIN, tools/gen_enet_golden.py)."""
import os

import numpy as np

import l2_restated

# (n, p, counts): the smallest shapes at which each layout of the three kernels can go wrong -- blocks of 64 columns, four
# waves, register rows of 256 columns, 64-sample words
SHAPES = [(70, 60, False),      # one partial block, a second sample word
          (130, 65, False),     # a second block holding one column
          (96, 128, False),     # blocks exactly full
          (200, 257, False),    # five blocks: wave 0's second register row; one wave steps two blocks in a row at the sweep's wrap
          (90, 1030, False),    # past the covariance form's column rule: the bit-packed route by itself
          (261, 40, True)]      # counts: the float route by itself, a second trip over the samples
ALPHAS = (1e-3, 1e-2, 1e-1, 1.0)
RATIOS = (0.5, 0.1, 1.0)
RATIO_ZERO_SHAPE = (70, 60, False)      # l1_ratio = 0 runs max_iter sweeps by construction: on the smallest design only
HELD = (-1, 2, 7)                       # all rows, and two held-out folds of the 10 contiguous ones
N_FOLDS = 10
TOL, MAX_ITER = 1e-4, 1000
MARGIN = 1e-6                           # how far, relatively, every stop decision of a kept case lies from its threshold
GS_SHAPE, GS_RATIO = (90, 1030, False), 0.5     # the recorded GridSearchCV: above 1,024 columns, where a Lasso's copies are merged
CONST_COL, ZERO_COL, DUP_COL = l2_restated.CONST_COL, l2_restated.ZERO_COL, l2_restated.DUP_COL


def design(n, p, counts, seed):
    """(X[n][p], y[n]): l2_restated.design -- correlated columns, a constant-1 column, an all-zero column, the last column a
    copy of DUP_COL -- with its continuous target."""
    X, yc, _ = l2_restated.design(n, p, counts, seed)
    return X, yc


def kfold(n, k=N_FOLDS):
    """sklearn.model_selection.KFold(k) without shuffling: contiguous folds, the first n % k one longer."""
    sizes = np.full(k, n // k)
    sizes[: n % k] += 1
    return np.repeat(np.arange(k), sizes).astype(np.int32)


def plan():
    """(fit_alpha, fit_held) of one call: every alpha on all rows and on the two held-out folds."""
    return [a for a in ALPHAS for _ in HELD], [h for _ in ALPHAS for h in HELD]


def enet_fit(X, y, alpha, l1_ratio, tol=TOL, max_iter=MAX_ITER, trace=None):
    """X, y: the training rows.  Returns (coef, intercept, n_iter).  trace: a list that receives ("ratio", d_w_max / w_max,
    tol) after every sweep with w_max != 0 and ("gap", gap, tol y'y) at every evaluation."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = X.shape
    mean, ym = X.mean(axis=0), y.mean()
    Xc = np.asfortranarray(X - mean)
    yc = y - ym
    l1 = alpha * l1_ratio * n
    l2 = alpha * (1.0 - l1_ratio) * n
    nrm = (Xc ** 2).sum(axis=0)
    cols = [j for j in range(p) if nrm[j] != 0.0]
    w = np.zeros(p)
    R = yc.copy()
    tol_s = tol * (yc @ yc)
    n_iter = 0
    for it in range(max_iter):
        w_max = d_w_max = 0.0
        for j in cols:
            xj = Xc[:, j]
            wj = w[j]
            tmp = xj @ R + wj * nrm[j]
            mag = abs(tmp) - l1
            nw = (mag if tmp > 0 else -mag) / (nrm[j] + l2) if mag > 0.0 else 0.0
            dd = nw - wj
            if dd != 0.0:
                R -= dd * xj
                w[j] = nw
            d_w_max = max(d_w_max, abs(dd))
            w_max = max(w_max, abs(nw))
        n_iter = it + 1
        if trace is not None and w_max != 0.0:
            trace.append(("ratio", d_w_max / w_max, tol))
        if w_max == 0.0 or d_w_max / w_max < tol or it == max_iter - 1:
            XtA = Xc.T @ R - l2 * w
            dual = np.abs(XtA).max() if p else 0.0
            RR, ww = R @ R, w @ w
            if dual > l1:
                c = l1 / dual
                gap = 0.5 * (RR + RR * (c * c))
            else:
                c = 1.0
                gap = RR
            gap += l1 * np.abs(w).sum() - c * (R @ yc) + 0.5 * l2 * (1.0 + c * c) * ww
            if trace is not None:
                trace.append(("gap", gap, tol_s))
            if gap < tol_s:
                break
    return w, float(ym - mean @ w), n_iter


def decisions_clear(trace, margin=MARGIN):
    """Whether every stop decision of a traced fit lies more than `margin` of its threshold away from it."""
    return all(abs(v - thr) > margin * thr for _, v, thr in trace)


class Engine:
    """Stands in for PskContext.enet_fit / lasso_fit in CPU tests: the same arguments and results, computed here.  `calls`
    keeps the shape of every design it was handed."""

    def __init__(self):
        self.calls = []

    def enet_fit(self, X, y, fold, fit_alpha, fit_fold, l1_ratio=0.5, tol=1e-4, max_iter=1000):
        if not 0.0 <= l1_ratio <= 1.0:
            raise ValueError("l1_ratio must lie in [0, 1]")
        X, y, fold = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(fold)
        self.calls.append(X.shape)
        fits = [enet_fit(X[fold != f], y[fold != f], a, l1_ratio, tol, max_iter) for a, f in zip(fit_alpha, fit_fold)]
        return np.stack([c for c, _, _ in fits]), np.array([b for _, b, _ in fits]), np.array([k for _, _, k in fits], dtype=np.int32)

    def lasso_fit(self, X, y, fold, fit_param, fit_fold, tol=1e-4, max_iter=1000):
        return self.enet_fit(X, y, fold, fit_param, fit_fold, 1.0, tol, max_iter)


class Fixture:
    """tests/golden/enet_kat.npz.  designs[d] = {X (float32), y, fold, n, p, counts, seed}; calls[d] = one dict per l1_ratio
    of the design, {l1_ratio, alpha[], held[], coef[fits][p], icpt[], n_iter[]}: scikit-learn's own, the fits in the order of
    plan().  gs = {design (index), l1_ratio, alphas, split_scores[alpha][fold], best_alpha, coef, icpt}: GridSearchCV(cv=10)."""

    def __init__(self, path=None):
        self.path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enet_kat.npz")
        z = np.load(self.path, allow_pickle=False)
        self.sklearn_version = str(z["sklearn_version"])
        self.tol, self.max_iter = float(z["tol"]), int(z["max_iter"])
        self.designs, self.calls = [], []
        for d in range(int(z["n_designs"])):
            n, p, counts = (int(v) for v in z["shape%d" % d])
            if counts:
                X = z["X%d" % d].astype(np.float32)
            else:
                X = np.unpackbits(z["X%d" % d], axis=1)[:, :p].astype(np.float32)
            self.designs.append(dict(X=X, y=z["y%d" % d], fold=z["fold%d" % d].astype(np.int32), n=n, p=p, counts=bool(counts),
                                     seed=int(z["seed%d" % d])))
            rows = []
            for k, ratio in enumerate(z["ratios%d" % d]):
                tag = "_%d_%d" % (d, k)
                rows.append(dict(l1_ratio=float(ratio), alpha=z["alpha" + tag], held=z["held" + tag].astype(np.int32),
                                 coef=z["coef" + tag], icpt=z["icpt" + tag], n_iter=z["n_iter" + tag].astype(np.int32)))
            self.calls.append(rows)
        self.gs = dict(design=int(z["gs_design"]), l1_ratio=float(z["gs_l1_ratio"]), alphas=z["gs_alphas"],
                       split_scores=z["gs_split_scores"], best_alpha=float(z["gs_best_alpha"]), coef=z["gs_coef"],
                       icpt=float(z["gs_icpt"]))


def judge(what, coef, icpt, iters, call):
    """What every route owes a recorded call (the bounds of test_lasso_covariance_form_walks_sklearns_path): scikit-learn's
    sweep count exactly, the coefficients within 1e-6 of the largest, the same support, the intercept to 1e-6.  Returns the
    largest coefficient error over the largest coefficient."""
    import pytest
    assert np.array_equal(np.asarray(iters), call["n_iter"]), (what, np.asarray(iters).tolist(), call["n_iter"].tolist())
    worst = 0.0
    for j in range(len(call["alpha"])):
        tag = (what, "l1_ratio=%g" % call["l1_ratio"], "alpha=%g" % call["alpha"][j], "held=%d" % call["held"][j], "sweeps=%d" % iters[j])
        scale = max(np.abs(call["coef"][j]).max(), 1e-300)
        err = np.abs(coef[j] - call["coef"][j]).max()
        worst = max(worst, err / scale)
        assert err <= 1e-6 * scale, tag + (err / scale,)
        assert np.array_equal(coef[j] != 0, call["coef"][j] != 0), tag
        assert icpt[j] == pytest.approx(float(call["icpt"][j]), rel=1e-6, abs=1e-9), tag
    return worst
