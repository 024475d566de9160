"""C-SVC over psk_svc_fit, and libsvm's Platt scaling for its probabilities."""
import numpy as np

from . import cv as _cv
from .model_search import _Estimator, _Twin, _fold_scores, _launch_plan, _launch_plan_of_numbers


class SVC(_Estimator):
    """sklearn.svm.SVC for two classes (set_model, modeling.py:1025-1029: SVC(kernel='linear', probability=True,
    max_iter, tol)) over psk_svc_fit: libsvm's solver without shrinking, so a fit stopped at max_iter is libsvm's iterate.
    Fitted attributes carry scikit-learn's sign and order (class 0's support vectors first; decision_function is the
    negative of libsvm's value; dual_coef_ = -y_i alpha_i; intercept_ = rho).  probability=True: libsvm fits the Platt
    sigmoid on decision values of an internal 5-fold split drawn from an unseeded generator; here the split is
    cv.stratified_kfold(y, 5), so the pair (probA_, probB_) is the same in every run.
    kernel='rbf' is searched over {'C', 'gamma'} by RandomizedSearch, as the reference's get_best_model does (:1091-1095);
    random_state is that search's seed and no parameter of the exported scikit-learn SVC.  decision_function, predict and
    predict_proba take an optional engine context: the decision values then come from psk_svc_decision."""
    _is_classifier = True
    _warns_at_max_iter = True   # scikit-learn's ConvergenceWarning when a fit stops there
    PLATT_FOLDS = 5

    def __init__(self, C=1.0, kernel="rbf", gamma="scale", tol=1e-3, max_iter=-1, probability=False, random_state=None):
        if kernel not in ("linear", "rbf"):
            raise ValueError("SVC: kernel must be 'linear' or 'rbf', got %r" % (kernel,))
        self.C, self.kernel, self.gamma, self.tol, self.max_iter, self.probability = C, kernel, gamma, tol, max_iter, probability
        self.random_state = random_state
        self.classes_ = np.array([0, 1])
        self.support_ = None

    @property
    def _randomized(self):
        """The reference puts the rbf kernel under RandomizedSearchCV, the linear one under GridSearchCV (:1086-1095)."""
        return self.kernel == "rbf"

    def __repr__(self):
        parts = []
        if self.C != 1.0:
            parts.append("C=%r" % self.C)
        if self.gamma != "scale":
            parts.append("gamma=%r" % self.gamma)
        if self.kernel != "rbf":
            parts.append("kernel=%r" % self.kernel)
        if repr(self.max_iter) != "-1":
            parts.append("max_iter=%r" % self.max_iter)
        if self.probability:
            parts.append("probability=True")
        if self.tol != 1e-3:
            parts.append("tol=%r" % self.tol)
        return "SVC(%s)" % ", ".join(parts)

    def _clone(self, **params):
        kw = dict(C=self.C, kernel=self.kernel, gamma=self.gamma, tol=self.tol, max_iter=self.max_iter,
                  probability=self.probability, random_state=self.random_state)
        kw.update(params)
        return type(self)(**kw)

    def _gamma_value(self, X):
        """scikit-learn's 'scale' = 1 / (n_features * X.var()), 'auto' = 1 / n_features, or the number given."""
        X = np.asarray(X, dtype=np.float64)
        if isinstance(self.gamma, str):
            if self.gamma == "scale":
                v = X.var()
                return 1.0 / (X.shape[1] * v) if v != 0 else 1.0
            if self.gamma == "auto":
                return 1.0 / X.shape[1]
            raise ValueError("SVC: gamma must be 'scale', 'auto' or a number, got %r" % (self.gamma,))
        return float(self.gamma)

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold, fit_gamma=None):
        """fit_gamma: one gamma per fit (a search over 'gamma'); None: this estimator's own for every fit."""
        y = np.asarray(y)
        if sorted(set(y.tolist())) != [0, 1]:
            raise ValueError("SVC: the two classes must be labelled 0 and 1")
        return ctx.svc_fit(X, y.astype(np.int32), folds, fit_param, fit_fold, kernel=self.kernel,
                           fit_gamma=self._gamma_value(X) if fit_gamma is None else fit_gamma, tol=self.tol,
                           max_iter=int(self.max_iter))

    def fit(self, X, y, engine_ctx):
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y)
        dual, rho, _, iters = self._engine_fit(engine_ctx, X, y, np.zeros(len(y), dtype=np.int32), [float(self.C)], [-1])
        self._set_fit(X, y, dual[0], rho[0], iters[0])
        if self.probability:
            self._fit_platt(engine_ctx, X, y)
        return self

    def _set_fit(self, X, y, dual, rho, iters):
        """dual[n]: y_i alpha_i in libsvm's sign (class 0 positive), 0 off the support."""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y)
        nz = dual != 0
        s0, s1 = np.nonzero(nz & (y == 0))[0], np.nonzero(nz & (y == 1))[0]
        self.support_ = np.concatenate([s0, s1]).astype(np.int32)
        self.support_vectors_ = np.ascontiguousarray(X[self.support_])
        self.n_support_ = np.array([len(s0), len(s1)], dtype=np.int32)
        self.dual_coef_ = -np.asarray(dual, dtype=np.float64)[self.support_].reshape(1, -1)
        self.intercept_ = np.array([float(rho)])
        self._gamma = self._gamma_value(X)
        self.shape_fit_ = tuple(int(v) for v in X.shape)
        self.n_features_in_ = int(X.shape[1])
        self.n_iter_ = np.array([int(iters)], dtype=np.int32)
        self.fit_status_ = int(int(self.max_iter) != -1 and int(iters) >= int(self.max_iter))
        self.probA_, self.probB_ = np.empty(0), np.empty(0)
        if self.kernel == "linear":
            self.coef_ = self.dual_coef_ @ self.support_vectors_
        return self

    def _search(self, ctx, X, y, folds, cand, cv):
        """Every candidate x fold and every candidate's refit in one launch; a fold is scored from the decision values the
        engine returns for every sample, held-out ones included.  Candidates over 'C', or over 'C' and 'gamma' (the rbf
        kernel's grid, :1050-1056): then every fit carries its own gamma, and the refit's Platt step the chosen pair."""
        if all(set(q) == {"C", "gamma"} for q in cand):
            if self.kernel != "rbf":
                raise ValueError("SVC: a grid over 'gamma' needs kernel='rbf'")
            fit_q, fit_fold = _launch_plan(cand, cv)
            fit_param, fit_gamma = [float(q["C"]) for q in fit_q], [float(q["gamma"]) for q in fit_q]
        elif all(set(q) == {"C"} for q in cand):
            (fit_param, fit_fold), fit_gamma = _launch_plan_of_numbers(cand, cv), None
        else:
            raise ValueError("SVC is searched over 'C', or over 'C' and 'gamma'")
        dual, rho, dec, iters = self._engine_fit(ctx, X, y, folds, fit_param, fit_fold, fit_gamma)
        scores = _fold_scores(cand, cv, folds, lambda q, j, te: np.mean(self.classes_[(dec[j][te] <= 0).astype(int)] == y[te]))

        def refit(best):
            j = len(cand) * cv + best
            est = self._clone(**cand[best])._set_fit(X, y, dual[j], rho[j], iters[j])
            return est._fit_platt(ctx, X, y) if est.probability else est
        return scores, refit, dict(n_iter_=iters)

    @property
    def _coef_column(self):
        return self.coef_[0]

    def _sklearn(self, fitted=True):
        """sklearn.svm.SVC and its fitted attributes (its __dict__ after fit, scikit-learn 1.7): the public ones in
        scikit-learn's sign, _dual_coef_ / _intercept_ the libsvm-sign copies its predict reads."""
        params = dict(kernel=self.kernel, gamma=self.gamma, tol=self.tol, max_iter=int(self.max_iter), probability=bool(self.probability))
        if not fitted:
            return _Twin("SVC", "sklearn.svm", params)
        state = dict(_sparse=False, n_features_in_=self.n_features_in_, class_weight_=np.ones(2), classes_=np.array([0, 1]),
                     _gamma=np.float64(self._gamma), support_=self.support_.astype(np.int32),
                     support_vectors_=self.support_vectors_.copy(), _n_support=self.n_support_.astype(np.int32),
                     dual_coef_=self.dual_coef_.copy(), intercept_=self.intercept_.copy(),
                     _probA=np.asarray(self.probA_, dtype=np.float64).copy(), _probB=np.asarray(self.probB_, dtype=np.float64).copy(),
                     fit_status_=int(self.fit_status_), _num_iter=self.n_iter_.astype(np.int32), shape_fit_=tuple(self.shape_fit_),
                     _intercept_=-self.intercept_, _dual_coef_=-self.dual_coef_, n_iter_=self.n_iter_.astype(np.int32))
        return _Twin("SVC", "sklearn.svm", dict(params, C=self.C), state)

    def _kernel(self, X):
        """K(x, support vector) in f64 as libsvm evaluates it."""
        X = np.asarray(X, dtype=np.float64)
        D = X @ self.support_vectors_.T
        if self.kernel == "linear":
            return D
        sx, ss = (X * X).sum(axis=1), (self.support_vectors_ * self.support_vectors_).sum(axis=1)
        return np.exp(-self._gamma * (sx[:, None] + ss[None, :] - 2 * D))

    def _on_device(self, X):
        """psk_svc_decision takes float32: whether X and the support vectors survive the round trip (what this package
        writes always does)."""
        X = np.asarray(X, dtype=np.float64)
        return bool(X.ndim == 2 and X.shape[0] >= 1 and X.shape[1] == self.support_vectors_.shape[1] and len(self.support_)
                    and np.array_equal(X.astype(np.float32).astype(np.float64), X)
                    and np.array_equal(self.support_vectors_.astype(np.float32).astype(np.float64), self.support_vectors_))

    def _libsvm_decision(self, X, engine_ctx=None):
        """sum_j y_j alpha_j K(x_j, x) - rho, the support vectors added one after the other as svm_predict_values does; with
        an engine context on the device (psk_svc_decision), in the same order."""
        if engine_ctx is not None and self._on_device(X):
            return engine_ctx.svc_decision(X, self.support_vectors_, -self.dual_coef_[0], self.intercept_[0], kernel=self.kernel,
                                           gamma=self._gamma if self.kernel == "rbf" else 0.0)
        K = self._kernel(X)
        coef = -self.dual_coef_[0]
        s = np.zeros(K.shape[0])
        for j in range(K.shape[1]):
            s += coef[j] * K[:, j]
        return s - self.intercept_[0]

    def decision_function(self, X, engine_ctx=None):
        return -self._libsvm_decision(X, engine_ctx)

    def predict(self, X, engine_ctx=None):
        # libsvm votes the second class on a decision value of zero
        return self.classes_[(self._libsvm_decision(X, engine_ctx) <= 0).astype(int)]

    def score(self, X, y):
        return np.float64(np.mean(self.predict(X) == np.asarray(y)))

    def _fit_platt(self, ctx, X, y):
        """svm_binary_svc_probability on a deterministic split: decision values of PLATT_FOLDS held-out parts from one more
        psk_svc_fit call at this C, then sigmoid_train.  A sub-fit whose training part lacks a class yields libsvm's constant
        decision values (+1 / -1 / 0)."""
        y = np.asarray(y)
        folds = _cv.stratified_kfold(y, self.PLATT_FOLDS)
        dec = np.zeros(len(y))
        todo = []
        for f in range(self.PLATT_FOLDS):
            tr = folds != f
            n0, n1 = int(np.sum(tr & (y == 0))), int(np.sum(tr & (y == 1)))
            if n0 and n1:
                todo.append(f)
            else:
                dec[~tr] = 1.0 if n0 else (-1.0 if n1 else 0.0)
        if todo:
            _, _, d, _ = self._engine_fit(ctx, X, y, folds, [float(self.C)] * len(todo), todo)
            for k, f in enumerate(todo):
                dec[folds == f] = d[k][folds == f]
        A, B = platt_sigmoid_train(dec, y == 0)
        self.probA_, self.probB_ = np.array([A]), np.array([B])
        return self

    def predict_proba(self, X, engine_ctx=None):
        if not len(getattr(self, "probA_", ())):
            raise AttributeError("predict_proba is not available when probability=False")
        return platt_predict_proba(self._libsvm_decision(X, engine_ctx), self.probA_[0], self.probB_[0])


def platt_sigmoid_train(dec, positive):
    """libsvm's sigmoid_train (Lin, Lin, Weng 2007): (A, B) of P(positive | f) = 1 / (1 + exp(A f + B)) by Newton's method
    with backtracking on the regularised likelihood, targets (N+ + 1)/(N+ + 2) and 1/(N- + 2).  f64, libsvm's constants."""
    dec = np.asarray(dec, dtype=np.float64)
    positive = np.asarray(positive, dtype=bool)
    prior1, prior0 = float(positive.sum()), float((~positive).sum())
    max_iter, min_step, sigma, eps = 100, 1e-10, 1e-12, 1e-5
    t = np.where(positive, (prior1 + 1.0) / (prior1 + 2.0), 1.0 / (prior0 + 2.0))

    def fval_at(A, B):
        f = dec * A + B
        return float(np.where(f >= 0, t * f + np.log1p(np.exp(-np.abs(f))), (t - 1.0) * f + np.log1p(np.exp(-np.abs(f)))).sum())

    A, B = 0.0, float(np.log((prior0 + 1.0) / (prior1 + 1.0)))
    fval = fval_at(A, B)
    for _ in range(max_iter):
        f = dec * A + B
        e = np.exp(-np.abs(f))
        p = np.where(f >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        q = np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        d2 = p * q
        h11, h22, h21 = sigma + float((dec * dec * d2).sum()), sigma + float(d2.sum()), float((dec * d2).sum())
        d1 = t - p
        g1, g2 = float((dec * d1).sum()), float(d1.sum())
        if abs(g1) < eps and abs(g2) < eps:
            break
        det = h11 * h22 - h21 * h21
        dA, dB = -(h22 * g1 - h21 * g2) / det, -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = 1.0
        while step >= min_step:
            nA, nB = A + step * dA, B + step * dB
            nf = fval_at(nA, nB)
            if nf < fval + 0.0001 * step * gd:
                A, B, fval = nA, nB, nf
                break
            step /= 2.0
        if step < min_step:   # the line search failed: libsvm stops here as well
            break
    return A, B


def platt_predict_proba(f, A, B):
    """svm_predict_probability for two classes from libsvm-sign decision values f: the pairwise value
    r = 1 / (1 + exp(A f + B)) clipped to [1e-7, 1 - 1e-7], then libsvm's multiclass_probability iteration (Wu, Lin, Weng
    2004), which scikit-learn runs for two classes as well.  Columns: class 0, class 1."""
    f = np.asarray(f, dtype=np.float64)
    fApB = f * A + B
    e = np.exp(-np.abs(fApB))
    r = np.where(fApB >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    r01 = np.minimum(np.maximum(r, 1e-7), 1 - 1e-7)
    r10 = 1 - r01
    k = 2
    Q00, Q11, Q01 = r10 * r10, r01 * r01, -r10 * r01   # Q[t][t] = sum_{j != t} r[j][t]^2, Q[t][j] = -r[j][t] r[t][j]
    p0, p1 = np.full(len(f), 1.0 / k), np.full(len(f), 1.0 / k)
    live = np.ones(len(f), dtype=bool)
    for _ in range(max(100, k)):
        Qp0, Qp1 = Q00 * p0 + Q01 * p1, Q01 * p0 + Q11 * p1
        pQp = p0 * Qp0 + p1 * Qp1
        live &= np.maximum(np.abs(Qp0 - pQp), np.abs(Qp1 - pQp)) >= 0.005 / k
        if not live.any():
            break
        with np.errstate(all="ignore"):
            diff = (-Qp0 + pQp) / Q00                      # t = 0
            n0 = p0 + diff
            pQp1 = (pQp + diff * (diff * Q00 + 2 * Qp0)) / (1 + diff) / (1 + diff)
            Qp1b = (Qp1 + diff * Q01) / (1 + diff)       # (Qp, pQp are rebuilt from p at the top of the next round)
            n0, n1 = n0 / (1 + diff), p1 / (1 + diff)
            diff = (-Qp1b + pQp1) / Q11                    # t = 1
            m1 = n1 + diff
            m0, m1 = n0 / (1 + diff), m1 / (1 + diff)
        p0, p1 = np.where(live, m0, p0), np.where(live, m1, p1)
    return np.column_stack([p0, p1])
