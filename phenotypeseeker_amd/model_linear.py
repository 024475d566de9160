"""The linear estimators: L1 / L2 logistic regression over psk_logreg_l1_fit / psk_logreg_l2_fit, Lasso, elastic net and
Ridge over psk_lasso_fit / psk_enet_fit / psk_ridge_fit.  All fits of a grid search (grid x folds + the refits) are solved on the GPU in one launch."""
import numpy as np

from .model_search import _Estimator, _Twin, _fold_scores, _launch_plan_of_numbers


class _Linear(_Estimator):
    """What the four have in common: one parameter searched, a (coef, intercept) pair per fit."""
    _dedupe_above = 0

    def _dedupes(self):
        """Whether this estimator's fits may be solved on the distinct columns."""
        return self._dedupe

    def _clone(self, **params):
        return type(self)(**params)

    def _search(self, ctx, X_full, y, folds, cand, cv):
        """Every candidate x fold and every candidate's refit in one launch, on the distinct columns where the penalty allows
        it; a fold is scored by score() of the candidate set to that fit; the best refit is scattered back to all columns."""
        # Identical columns (k-mers of one gene share a presence pattern) are solved once: an L1
        # optimum may place a pattern's weight on any of its copies, here on the first (which is also
        # what cyclic coordinate descent -- scikit-learn's Lasso -- does).
        if self._dedupes() and X_full.shape[1] > self._dedupe_above:
            X, first, _ = _unique_columns(X_full)
        else:  # an L2 optimum spreads a pattern's weight over its copies: every column stays
            X, first = X_full, np.arange(X_full.shape[1])
        fit_param, fit_fold = _launch_plan_of_numbers(cand, cv)
        coef, icpt, iters = self._engine_fit(ctx, X, y, folds, fit_param, fit_fold)
        scores = _fold_scores(cand, cv, folds, lambda q, j, te: self._clone(**q)._set(coef[j], icpt[j]).score(X[te], y[te]))

        def refit(best):
            j = len(cand) * cv + best
            est = self._clone(**cand[best])
            est.tol, est.max_iter = self.tol, self.max_iter
            full = np.zeros(X_full.shape[1])
            full[first] = coef[j]
            return est._set(full, icpt[j])
        return scores, refit, dict(n_unique_columns_=int(X.shape[1]), n_iter_=iters)


class L1LogisticRegression(_Linear):
    """L1 logistic regression, LogisticRegression(penalty='l1', solver=...) (modeling.py:1011-1014).  solver='liblinear':
    ||w||_1 + |b| + C sum log(1+exp(-y(w.x+b))), the intercept a penalised constant feature (psk_logreg_l1_fit);
    solver='saga': ||w||_1 + C sum log(1+exp(-y(w.x+b))), the intercept free (psk_logreg_l1_free_fit) -- another model, not
    another route to the same one.  Either way the fit is the optimum of the objective the solver minimises."""
    _is_classifier = True
    _dedupe = True  # an L1 optimum may sit on any copy of a repeated column: solve each pattern once

    def __init__(self, C=1.0, tol=1e-4, max_iter=1000, solver="liblinear"):
        if solver not in ("liblinear", "saga"):
            raise ValueError("solver must be 'liblinear' or 'saga' for the L1 penalty, got %r" % (solver,))
        self.C, self.tol, self.max_iter = C, tol, max_iter
        self.penalty, self.solver = "l1", solver
        self.classes_ = np.array([0, 1])
        self.coef_ = None
        self.intercept_ = None

    def __repr__(self):
        # scikit-learn prints only the parameters that differ from its defaults, alphabetically
        parts = []
        if self.C != 1.0:
            parts.append("C=%r" % self.C)
        if repr(self.max_iter) != "100":
            parts.append("max_iter=%r" % self.max_iter)
        parts += ["penalty='l1'", "solver=%r" % self.solver]
        if self.tol != 1e-4:
            parts.append("tol=%r" % self.tol)
        return "LogisticRegression(%s)" % ", ".join(parts)

    def _clone(self, **params):
        return type(self)(solver=self.solver, **params)

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold):
        fit = ctx.logreg_l1_free_fit if self.solver == "saga" else ctx.logreg_l1_fit
        return fit(X, y.astype(np.int32), folds, fit_param, fit_fold, self.tol, int(self.max_iter))

    def _set(self, coef, icpt):
        self.coef_ = np.asarray(coef, dtype=np.float64).reshape(1, -1)
        self.intercept_ = np.array([float(icpt)])
        self.n_features_in_ = self.coef_.shape[1]
        return self

    def decision_function(self, X):
        return np.asarray(X, dtype=np.float64) @ self.coef_[0] + self.intercept_[0]

    def predict(self, X):
        return self.classes_[(self.decision_function(X) > 0).astype(int)]

    def predict_proba(self, X):
        p1 = 1.0 / (1.0 + np.exp(-self.decision_function(X)))
        return np.column_stack([1.0 - p1, p1])

    def score(self, X, y):
        return np.float64(np.mean(self.predict(X) == np.asarray(y)))

    @property
    def _coef_column(self):
        return self.coef_[0]

    def _sklearn(self, fitted=True):
        params = dict(penalty=self.penalty, solver=self.solver, tol=self.tol, max_iter=int(self.max_iter))
        if not fitted:
            return _Twin("LogisticRegression", "sklearn.linear_model", params)
        return _Twin("LogisticRegression", "sklearn.linear_model", dict(params, C=self.C),
                     dict(classes_=np.array([0, 1]), coef_=self.coef_.copy(), intercept_=self.intercept_.copy(),
                          n_iter_=np.array([0], dtype=np.int32), n_features_in_=self.n_features_in_))


class L2LogisticRegression(L1LogisticRegression):
    """0.5 w'w + C sum log(1+exp(-y(w.x+b))): LogisticRegression(penalty='l2', solver=...)
    (modeling.py:1015-1019).  The intercept is free for lbfgs / newton-cg / sag / saga and a penalised
    constant feature for liblinear (get_logreg_solver, modeling.py:256-264); the optimum is unique
    either way, so one Newton solver serves all five names."""
    _dedupe = False

    def __init__(self, C=1.0, tol=1e-4, max_iter=1000, solver="lbfgs"):
        super().__init__(C, tol, max_iter)
        self.penalty, self.solver = "l2", solver

    def __repr__(self):
        parts = []
        if self.C != 1.0:
            parts.append("C=%r" % self.C)
        if repr(self.max_iter) != "100":
            parts.append("max_iter=%r" % self.max_iter)
        if self.solver != "lbfgs":
            parts.append("solver=%r" % self.solver)
        if self.tol != 1e-4:
            parts.append("tol=%r" % self.tol)
        return "LogisticRegression(%s)" % ", ".join(parts)

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold):
        return ctx.logreg_l2_fit(X, y.astype(np.int32), folds, fit_param, fit_fold, self.tol, int(self.max_iter),
                                 self.solver == "liblinear")


class LassoRegression(_Linear):
    """(1/2n)||y - Xw - b||^2 + alpha ||w||_1."""
    _is_classifier = False
    # scikit-learn's cyclic descent visits every column, copies included, and a fit that ends at the sweep limit has walked a
    # path the copies were part of (r04: the grid search of a 1,024 x 907 design was 2e-3 off in R^2 on its unconverged row
    # with the copies removed).  Up to 1,024 columns -- the covariance form of solver_lasso.hip -- every column is kept;
    # beyond that (--n_kmers 0 models) each distinct pattern is solved once: the same optimum where the descent converges.
    _dedupe = True
    _dedupe_above = 1024
    _sk_name, _sk_n_iter = "Lasso", 0

    def __init__(self, alpha=1.0, tol=1e-4, max_iter=1000):
        self.alpha, self.tol, self.max_iter = alpha, tol, max_iter
        self.coef_ = None
        self.intercept_ = None

    def __repr__(self):
        parts = []
        if self.alpha != 1.0:
            parts.append("alpha=%r" % self.alpha)
        if repr(self.max_iter) != "1000":
            parts.append("max_iter=%r" % self.max_iter)
        if self.tol != 1e-4:
            parts.append("tol=%r" % self.tol)
        return "%s(%s)" % (self._sk_name, ", ".join(parts))

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold):
        return ctx.lasso_fit(X, y.astype(np.float64), folds, fit_param, fit_fold, self.tol, int(self.max_iter))

    def _set(self, coef, icpt):
        self.coef_ = np.asarray(coef, dtype=np.float64).ravel()
        self.intercept_ = float(icpt)
        self.n_features_in_ = len(self.coef_)
        return self

    def predict(self, X):
        return np.asarray(X, dtype=np.float64) @ self.coef_ + self.intercept_

    def score(self, X, y):
        """R^2 as sklearn.metrics.r2_score returns it (what GridSearchCV scores a regressor with, modeling.py:1208-1216):
        undefined -- nan -- on fewer than two samples (a 10-fold split of fewer than 20 samples has such folds: the
        reference's summary then prints `nan (+/-nan)` for every alpha); a constant target scores 1.0 when it is predicted
        exactly and 0.0 otherwise (force_finite)."""
        y = np.asarray(y, dtype=np.float64)
        if len(y) < 2:
            return np.float64(np.nan)
        res = ((y - self.predict(X)) ** 2).sum()
        tot = ((y - y.mean()) ** 2).sum()
        if tot == 0.0:
            return np.float64(1.0 if res == 0.0 else 0.0)
        return np.float64(1.0 - res / tot)

    @property
    def _coef_column(self):
        return self.coef_

    def _sklearn(self, fitted=True):
        params = dict(tol=self.tol, max_iter=int(self.max_iter))
        if not fitted:
            return _Twin(self._sk_name, "sklearn.linear_model", params)
        return _Twin(self._sk_name, "sklearn.linear_model", dict(params, alpha=self.alpha),
                     dict(coef_=self.coef_.copy(), intercept_=self.intercept_, n_iter_=self._sk_n_iter, n_features_in_=self.n_features_in_))


class ElasticNetRegression(LassoRegression):
    """(1/2n)||y - Xw - b||^2 + alpha l1_ratio ||w||_1 + 1/2 alpha (1 - l1_ratio) ||w||^2: sklearn ElasticNet
    (modeling.py:1003-1006), walked as scikit-learn walks it (psk_enet_fit)."""
    _sk_name = "ElasticNet"

    def __init__(self, alpha=1.0, l1_ratio=0.5, tol=1e-4, max_iter=1000):
        super().__init__(alpha, tol, max_iter)
        self.l1_ratio = l1_ratio

    def __repr__(self):
        parts = []
        if self.alpha != 1.0:
            parts.append("alpha=%r" % self.alpha)
        if self.l1_ratio != 0.5:
            parts.append("l1_ratio=%r" % self.l1_ratio)
        if repr(self.max_iter) != "1000":
            parts.append("max_iter=%r" % self.max_iter)
        if self.tol != 1e-4:
            parts.append("tol=%r" % self.tol)
        return "ElasticNet(%s)" % ", ".join(parts)

    def _clone(self, **params):
        return type(self)(l1_ratio=self.l1_ratio, **params)

    def _dedupes(self):
        # With an L2 term a pattern's copies share its weight, and a walk cut short leaves them at different non-zero values
        # (0.029 / 0.050 on a 70 x 60 design at alpha 1e-3, l1_ratio 0.5): every column stays.  l1_ratio == 1 is the Lasso.
        return self.l1_ratio == 1

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold):
        return ctx.enet_fit(X, y.astype(np.float64), folds, fit_param, fit_fold, self.l1_ratio, self.tol, int(self.max_iter))

    def _sklearn(self, fitted=True):
        twin = super()._sklearn(fitted)
        twin.params["l1_ratio"] = self.l1_ratio
        return twin


class RidgeRegression(LassoRegression):
    """||y - Xw - b||^2 + alpha ||w||^2: sklearn Ridge (modeling.py:1001-1002).  max_iter / tol are
    carried for the repr only -- the dense solve is direct in scikit-learn and converged here."""
    _dedupe = False
    _sk_name, _sk_n_iter = "Ridge", None

    def __repr__(self):
        parts = []
        if self.alpha != 1.0:
            parts.append("alpha=%r" % self.alpha)
        if self.max_iter is not None:
            parts.append("max_iter=%r" % self.max_iter)
        if self.tol != 1e-3:
            parts.append("tol=%r" % self.tol)
        return "Ridge(%s)" % ", ".join(parts)

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold):
        return ctx.ridge_fit(X, y.astype(np.float64), folds, fit_param, fit_fold)


def _unique_columns(X):
    """Distinct columns of X in order of first appearance: (X_unique, first_index[], inverse[])."""
    seen = {}
    first, inverse = [], np.empty(X.shape[1], dtype=np.int64)
    cols = np.ascontiguousarray(X.T)
    for j in range(X.shape[1]):
        key = cols[j].tobytes()
        u = seen.get(key)
        if u is None:
            u = len(first)
            seen[key] = u
            first.append(j)
        inverse[j] = u
    first = np.array(first, dtype=np.int64)
    return np.ascontiguousarray(X[:, first]) if len(first) else X[:, :0], first, inverse
