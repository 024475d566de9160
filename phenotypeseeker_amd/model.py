"""The estimator boundary: picklable stand-ins for what the reference stores in
its .pkl -- a fitted GridSearchCV over LogisticRegression(penalty='l1', solver='liblinear') or
Lasso (modeling.py:994-1014, :1075-1085, :1208-1216, :975-979) -- exposing the attributes the
reference reads: predict / predict_proba / score, cv_results_['mean_test_score' |
'std_test_score' | 'params'], best_params_, best_estimator_.coef_ (modeling.py:1226-1247,
:1427-1436; prediction.py:126-129,:168-172).  All fits of a grid search (grid x folds + the
refit) are solved on the GPU in one psk_logreg_l1_fit / psk_lasso_fit launch.  `--penalty L2`
(modeling.py:1001-1002, :1015-1019) maps to RidgeRegression / L2LogisticRegression over
psk_ridge_fit / psk_logreg_l2_fit in the same way, `-bc SVM` (modeling.py:1025-1029) to SVC over
psk_svc_fit, whose folds are scored from the decision values the engine returns, and `-bc DT` (modeling.py:1032-1033) to
DecisionTree over psk_tree_fit under a two-key grid, scored from the leaves the engine returns for every sample, and `-bc RF`
(modeling.py:1030-1031) to RandomForest over psk_forest_fit under RandomizedSearch: scikit-learn's forest and sampler for a
given seed, the host drawing what NumPy's RandomState draws.
"""
import numpy as np

from . import cv as _cv


class L1LogisticRegression:
    """liblinear-style L1 logistic regression: ||w||_1 + |b| + C sum log(1+exp(-y(w.x+b)))."""
    _is_classifier = True
    _dedupe = True  # an L1 optimum may sit on any copy of a repeated column: solve each pattern once

    def __init__(self, C=1.0, tol=1e-4, max_iter=1000):
        self.C, self.tol, self.max_iter = C, tol, max_iter
        self.penalty, self.solver = "l1", "liblinear"
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
        parts += ["penalty='l1'", "solver='liblinear'"]
        if self.tol != 1e-4:
            parts.append("tol=%r" % self.tol)
        return "LogisticRegression(%s)" % ", ".join(parts)

    def _clone(self, **params):
        return type(self)(**params)

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold):
        return ctx.logreg_l1_fit(X, y.astype(np.int32), folds, fit_param, fit_fold, self.tol, int(self.max_iter))

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

    def _clone(self, **params):
        return type(self)(solver=self.solver, **params)

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold):
        return ctx.logreg_l2_fit(X, y.astype(np.int32), folds, fit_param, fit_fold, self.tol, int(self.max_iter),
                                 self.solver == "liblinear")


class LassoRegression:
    """(1/2n)||y - Xw - b||^2 + alpha ||w||_1."""
    _is_classifier = False
    # scikit-learn's cyclic descent visits every column, copies included, and a fit that ends at the sweep limit has walked a
    # path the copies were part of (r04: the grid search of a 1,024 x 907 design was 2e-3 off in R^2 on its unconverged row
    # with the copies removed).  Up to 1,024 columns -- the covariance form of solver_lasso.hip -- every column is kept;
    # beyond that (--n_kmers 0 models) each distinct pattern is solved once: the same optimum where the descent converges.
    _dedupe = True
    _dedupe_above = 1024
    _sk_name = "Lasso"

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

    def _clone(self, **params):
        return type(self)(**params)

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


class RidgeRegression(LassoRegression):
    """||y - Xw - b||^2 + alpha ||w||^2: sklearn Ridge (modeling.py:1001-1002).  max_iter / tol are
    carried for the repr only -- the dense solve is direct in scikit-learn and converged here."""
    _dedupe = False
    _sk_name = "Ridge"

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


class SVC:
    """sklearn.svm.SVC for two classes (set_model, modeling.py:1025-1029: SVC(kernel='linear', probability=True,
    max_iter, tol)) over psk_svc_fit: libsvm's solver without shrinking, so a fit stopped at max_iter is libsvm's iterate.
    Fitted attributes carry scikit-learn's sign and order (class 0's support vectors first; decision_function is the
    negative of libsvm's value; dual_coef_ = -y_i alpha_i; intercept_ = rho).  probability=True: libsvm fits the Platt
    sigmoid on decision values of an internal 5-fold split drawn from an unseeded generator; here the split is
    cv.stratified_kfold(y, 5), so the pair (probA_, probB_) is the same in every run."""
    _is_classifier = True
    _dedupe = False           # a dual solution depends on every column
    _scores_from_dec = True   # GridSearch scores the folds from psk_svc_fit's decision values
    PLATT_FOLDS = 5

    def __init__(self, C=1.0, kernel="rbf", gamma="scale", tol=1e-3, max_iter=-1, probability=False):
        if kernel not in ("linear", "rbf"):
            raise ValueError("SVC: kernel must be 'linear' or 'rbf', got %r" % (kernel,))
        self.C, self.kernel, self.gamma, self.tol, self.max_iter, self.probability = C, kernel, gamma, tol, max_iter, probability
        self.classes_ = np.array([0, 1])
        self.support_ = None

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
                  probability=self.probability)
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

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold):
        y = np.asarray(y)
        if sorted(set(y.tolist())) != [0, 1]:
            raise ValueError("SVC: the two classes must be labelled 0 and 1")
        return ctx.svc_fit(X, y.astype(np.int32), folds, fit_param, fit_fold, kernel=self.kernel,
                           fit_gamma=self._gamma_value(X), tol=self.tol, max_iter=int(self.max_iter))

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

    def _sklearn_state(self):
        """The fitted attributes of sklearn.svm.SVC (its __dict__ after fit, scikit-learn 1.7): the public ones in
        scikit-learn's sign, _dual_coef_ / _intercept_ the libsvm-sign copies its predict reads."""
        return dict(_sparse=False, n_features_in_=self.n_features_in_, class_weight_=np.ones(2), classes_=np.array([0, 1]),
                    _gamma=np.float64(self._gamma), support_=self.support_.astype(np.int32),
                    support_vectors_=self.support_vectors_.copy(), _n_support=self.n_support_.astype(np.int32),
                    dual_coef_=self.dual_coef_.copy(), intercept_=self.intercept_.copy(),
                    _probA=np.asarray(self.probA_, dtype=np.float64).copy(), _probB=np.asarray(self.probB_, dtype=np.float64).copy(),
                    fit_status_=int(self.fit_status_), _num_iter=self.n_iter_.astype(np.int32), shape_fit_=tuple(self.shape_fit_),
                    _intercept_=-self.intercept_, _dual_coef_=-self.dual_coef_, n_iter_=self.n_iter_.astype(np.int32))

    def _kernel(self, X):
        """K(x, support vector) in f64 as libsvm evaluates it."""
        X = np.asarray(X, dtype=np.float64)
        D = X @ self.support_vectors_.T
        if self.kernel == "linear":
            return D
        sx, ss = (X * X).sum(axis=1), (self.support_vectors_ * self.support_vectors_).sum(axis=1)
        return np.exp(-self._gamma * (sx[:, None] + ss[None, :] - 2 * D))

    def _libsvm_decision(self, X):
        """sum_j y_j alpha_j K(x_j, x) - rho, the support vectors added one after the other as svm_predict_values does."""
        K = self._kernel(X)
        coef = -self.dual_coef_[0]
        s = np.zeros(K.shape[0])
        for j in range(K.shape[1]):
            s += coef[j] * K[:, j]
        return s - self.intercept_[0]

    def decision_function(self, X):
        return -self._libsvm_decision(X)

    def predict(self, X):
        # libsvm votes the second class on a decision value of zero
        return self.classes_[(self._libsvm_decision(X) <= 0).astype(int)]

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

    def predict_proba(self, X):
        if not len(getattr(self, "probA_", ())):
            raise AttributeError("predict_proba is not available when probability=False")
        return platt_predict_proba(self._libsvm_decision(X), self.probA_[0], self.probB_[0])


class Tree:
    """The attributes of scikit-learn's tree_ (sklearn.tree._tree.Tree) for a two-class tree on a 0/1 design: nodes in
    pre-order, threshold 0.5 at a split and -2 at a leaf, value the class fractions ([node_count][1][2], scikit-learn >= 1.3)."""
    n_outputs, max_n_classes = 1, 2

    def __init__(self, n_features, feature, left, right, n_node_samples, counts, impurity, max_depth, weighted_n_node_samples=None):
        """counts: the class counts by node; in a forest's tree they are weighted (bootstrap multiplicities) and
        weighted_n_node_samples is their sum, while n_node_samples counts the distinct samples."""
        self.n_features = int(n_features)
        self.n_classes = np.array([2], dtype=np.int64)
        self.feature = np.asarray(feature, dtype=np.int64)
        self.children_left, self.children_right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
        self.n_node_samples = np.asarray(n_node_samples, dtype=np.int64)
        self.weighted_n_node_samples = (self.n_node_samples.astype(np.float64) if weighted_n_node_samples is None
                                        else np.asarray(weighted_n_node_samples, dtype=np.float64))
        self.impurity = np.asarray(impurity, dtype=np.float64)
        self.threshold = np.where(self.feature >= 0, 0.5, -2.0)
        self.value = (np.asarray(counts, dtype=np.float64) / self.weighted_n_node_samples[:, None]).reshape(-1, 1, 2)
        self.missing_go_to_left = np.zeros(len(self.feature), dtype=np.uint8)
        self.node_count, self.max_depth = len(self.feature), int(max_depth)
        self.capacity = self.node_count

    def apply(self, X):
        """The leaf of every row: x <= threshold goes left."""
        X = np.asarray(X, dtype=np.float64)
        node = np.zeros(X.shape[0], dtype=np.int64)
        rows = np.arange(X.shape[0])
        for _ in range(self.max_depth):
            f = self.feature[node]
            inner = f >= 0
            go_left = X[rows, np.where(inner, f, 0)] <= self.threshold[node]
            node = np.where(inner, np.where(go_left, self.children_left[node], self.children_right[node]), node)
        return node

    def predict(self, X):
        return self.value[self.apply(X), 0, :]

    def compute_feature_importances(self, normalize=True):
        """Tree.compute_feature_importances: the weighted impurity decrease of every split, added per feature in node order,
        divided by the root's weight and, normalised, by their sum (f64 on the host)."""
        imp = np.zeros(self.n_features)
        w, I, L, R = self.weighted_n_node_samples, self.impurity, self.children_left, self.children_right
        for k in range(self.node_count):
            if L[k] != -1:
                imp[self.feature[k]] += w[k] * I[k] - w[L[k]] * I[L[k]] - w[R[k]] * I[R[k]]
        imp /= w[0]
        if normalize:
            total = np.sum(imp)
            if total > 0.0:
                imp /= total
        return imp

    def _sklearn_state(self):
        """Tree.__getstate__ of scikit-learn 1.7: the structured node array (64 bytes a node) and the value array."""
        dt = np.dtype({"names": ["left_child", "right_child", "feature", "threshold", "impurity", "n_node_samples",
                                 "weighted_n_node_samples", "missing_go_to_left"],
                       "formats": ["<i8", "<i8", "<i8", "<f8", "<f8", "<i8", "<f8", "u1"],
                       "offsets": [0, 8, 16, 24, 32, 40, 48, 56], "itemsize": 64})
        nodes = np.zeros(self.node_count, dtype=dt)
        for name, v in (("left_child", self.children_left), ("right_child", self.children_right), ("feature", self.feature),
                        ("threshold", self.threshold), ("impurity", self.impurity), ("n_node_samples", self.n_node_samples),
                        ("weighted_n_node_samples", self.weighted_n_node_samples), ("missing_go_to_left", self.missing_go_to_left)):
            nodes[name] = v
        return dict(max_depth=int(self.max_depth), node_count=int(self.node_count), nodes=nodes,
                    values=np.ascontiguousarray(self.value, dtype=np.float64))

    @classmethod
    def _from_sklearn_state(cls, n_features, state):
        nd, val = state["nodes"], np.asarray(state["values"], dtype=np.float64)
        t = cls(n_features, nd["feature"], nd["left_child"], nd["right_child"], nd["n_node_samples"],
                val[:, 0, :] * np.asarray(nd["weighted_n_node_samples"], dtype=np.float64)[:, None], nd["impurity"], state["max_depth"],
                weighted_n_node_samples=nd["weighted_n_node_samples"])
        t.threshold, t.value = np.asarray(nd["threshold"], dtype=np.float64), val.reshape(-1, 1, val.shape[-1])
        return t


class DecisionTree:
    """sklearn.tree.DecisionTreeClassifier for two classes on a 0/1 design (set_model, modeling.py:1032-1033:
    DecisionTreeClassifier() under {'max_depth': 1..10, 'criterion': ['gini', 'entropy']}) over psk_tree_fit:
    scikit-learn's depth-first best-split builder with its default settings.  scikit-learn breaks ties between equally good
    splits by an unseeded random feature order; here the lowest column index wins."""
    _is_classifier = True
    _fits_trees = True       # GridSearch scores the folds from the leaves psk_tree_fit returns for every sample
    MAX_DEPTH = 10

    def __init__(self, criterion="gini", max_depth=None):
        if criterion not in ("gini", "entropy"):
            raise ValueError("DecisionTree: criterion must be 'gini' or 'entropy', got %r" % (criterion,))
        self.criterion, self.max_depth = criterion, max_depth
        self.classes_ = np.array([0, 1])
        self.tree_ = None

    def __repr__(self):
        parts = []
        if self.criterion != "gini":
            parts.append("criterion=%r" % self.criterion)
        if self.max_depth is not None:
            parts.append("max_depth=%r" % self.max_depth)
        return "DecisionTreeClassifier(%s)" % ", ".join(parts)

    def _clone(self, **params):
        kw = dict(criterion=self.criterion, max_depth=self.max_depth)
        kw.update(params)
        return type(self)(**kw)

    def _engine_fit(self, ctx, X, y, folds, fit_param, fit_fold):
        """fit_param: one dict per fit; keys it lacks come from this estimator."""
        y = np.asarray(y)
        if not set(y.tolist()) <= {0, 1}:
            raise ValueError("DecisionTree: the two classes must be labelled 0 and 1")
        depth = [q.get("max_depth", self.max_depth) for q in fit_param]
        crit = [q.get("criterion", self.criterion) for q in fit_param]
        for dp in depth:
            if dp is None or not 1 <= int(dp) <= self.MAX_DEPTH:
                raise ValueError("DecisionTree: max_depth must be 1..%d on the GPU engine, got %r" % (self.MAX_DEPTH, dp))
        for c in crit:
            if c not in ("gini", "entropy"):
                raise ValueError("DecisionTree: criterion must be 'gini' or 'entropy', got %r" % (c,))
        return ctx.tree_fit(X, y.astype(np.int32), folds, [int(dp) for dp in depth], crit, fit_fold)

    def fit(self, X, y, engine_ctx):
        X = np.asarray(X, dtype=np.float64)
        fits = self._engine_fit(engine_ctx, X, y, np.zeros(len(y), dtype=np.int32), [{}], [-1])
        return self._set_fit(fits[0], X.shape[1])

    def _set_fit(self, fit, n_features):
        self.tree_ = Tree(n_features, fit["feature"], fit["left"], fit["right"], fit["n_node_samples"], fit["counts"],
                          fit["impurity"], fit["max_depth"])
        self.n_features_in_ = int(n_features)
        self.n_outputs_, self.n_classes_, self.max_features_ = 1, np.int64(2), int(n_features)
        return self

    @property
    def feature_importances_(self):
        return self.tree_.compute_feature_importances()

    def _sklearn_state(self):
        """The fitted attributes of sklearn.tree.DecisionTreeClassifier (its __dict__ after fit, scikit-learn 1.7) without
        tree_, which pickles by __reduce__ (skpickle.Reduced)."""
        return dict(n_features_in_=self.n_features_in_, n_outputs_=1, classes_=np.array([0, 1]), n_classes_=np.int64(2),
                    max_features_=self.n_features_in_)

    def predict_proba(self, X):
        return self.tree_.predict(X)

    def predict(self, X):
        # np.argmax: class 0 on equal fractions
        return self.classes_[np.argmax(self.predict_proba(X), axis=1)]

    def score(self, X, y):
        return np.float64(np.mean(self.predict(X) == np.asarray(y)))


def _sk_repr(name, parts, width=80):
    """name(part, part, ...) broken into lines as scikit-learn's estimator printer does (utils/_pprint.py, compact): greedy
    filling of `width` columns, continuation lines indented to the opening parenthesis."""
    indent = len(name) + 1
    room = full = width - indent + 1
    out, delim = [], ""
    for i, rep in enumerate(parts):
        if i == len(parts) - 1:          # the closing parenthesis
            full -= 1
            room -= 1
        w = len(rep) + 2
        if room < w:
            room = full
            if delim:
                delim = ",\n" + " " * indent
        if room >= w:
            room -= w
        out.append(delim + rep)
        delim = ", "
    return "%s(%s)" % (name, "".join(out))


RAND_R_MAX = 2147483647   # sklearn/utils/_random.pxd


class ForestDraws:
    """Everything scikit-learn draws from NumPy's RandomState for RandomForestClassifier(random_state=seed), on the host:
    tree t's seed is the t-th rs.randint(int32 max) of rs = RandomState(seed) (ensemble/_base.py::_set_random_states, drawn in
    tree order before any fit); the splitter's generator state is RandomState(seed_t).randint(0, RAND_R_MAX)
    (_splitter.pyx::Splitter.init); with bootstrap the tree trains on bincount(RandomState(seed_t).randint(0, n_train,
    n_train, dtype=int32)) as sample weights (ensemble/_forest.py::_generate_sample_indices), mapped through the training
    rows.  Draws are kept: the candidates of a search share their trees' seeds (clone keeps an integer random_state)."""

    def __init__(self, seed, n_all):
        self.rs = np.random.RandomState(int(seed))
        self.n_all = int(n_all)
        self.seeds, self.states, self.weights = [], [], {}

    def state(self, t):
        while len(self.seeds) <= t:
            self.seeds.append(int(self.rs.randint(np.iinfo(np.int32).max)))
            self.states.append(int(np.random.RandomState(self.seeds[-1]).randint(0, RAND_R_MAX)))
        return self.states[t]

    def weight(self, t, rows_key, rows, bootstrap):
        """uint16[n_all]: tree t's sample weights when it trains on the (ascending) sample rows `rows`; rows_key names them."""
        key = (t if bootstrap else -1, rows_key)
        w = self.weights.get(key)
        if w is None:
            w = np.zeros(self.n_all, dtype=np.uint16)
            if bootstrap:
                self.state(t)
                idx = np.random.RandomState(self.seeds[t]).randint(0, len(rows), len(rows), dtype=np.int32)
                w[rows] = np.bincount(idx, minlength=len(rows))
            else:
                w[rows] = 1
            self.weights[key] = w
        return w


class ForestTree(DecisionTree):
    """One tree of a RandomForest: a DecisionTree whose tree_ carries weighted class counts (model.Tree with
    weighted_n_node_samples) and which, as in scikit-learn, knows its own seed and the forest's parameters."""

    def __init__(self, criterion="gini", max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features="sqrt", random_state=None):
        super().__init__(criterion, max_depth)
        self.min_samples_split, self.min_samples_leaf, self.max_features, self.random_state = (
            min_samples_split, min_samples_leaf, max_features, random_state)

    def _set_fit(self, fit, n_features):
        self.tree_ = Tree(n_features, fit["feature"], fit["left"], fit["right"], fit["n_node_samples"], fit["counts"],
                          fit["impurity"], fit["max_depth"], weighted_n_node_samples=np.asarray(fit["counts"]).sum(axis=1))
        self.n_features_in_ = int(n_features)
        self.n_outputs_, self.n_classes_ = 1, np.int64(2)
        self.max_features_ = RandomForest.n_max_features(self.max_features, n_features)
        return self

    def _sklearn_state(self):
        return dict(n_features_in_=self.n_features_in_, n_outputs_=1, classes_=np.array([0.0, 1.0]), n_classes_=np.int64(2),
                    max_features_=int(self.max_features_))


class RandomForest:
    """sklearn.ensemble.RandomForestClassifier for two classes on a 0/1 design (set_model, modeling.py:1030-1031) over
    psk_forest_fit: for an integer random_state, scikit-learn 1.7.2's forest to the node.  The seven
    parameters of the reference's grid plus random_state; everything else at scikit-learn's defaults."""
    _is_classifier = True
    _fits_forest = True
    PARAMS = ("bootstrap", "criterion", "max_depth", "max_features", "min_samples_leaf", "min_samples_split", "n_estimators")
    DEFAULTS = dict(bootstrap=True, criterion="gini", max_depth=None, max_features="sqrt", min_samples_leaf=1, min_samples_split=2,
                    n_estimators=100)
    TREE_PARAMS = ("criterion", "max_depth", "min_samples_split", "min_samples_leaf", "min_weight_fraction_leaf", "max_features",
                   "max_leaf_nodes", "min_impurity_decrease", "random_state", "ccp_alpha", "monotonic_cst")   # estimator_params
    SCRATCH_BYTES = 1 << 30   # per engine call: 16 bytes per tree and sample of leaf fractions

    def __init__(self, n_estimators=100, criterion="gini", max_depth=None, min_samples_split=2, min_samples_leaf=1,
                 max_features="sqrt", bootstrap=True, random_state=0):
        self.n_estimators, self.criterion, self.max_depth = n_estimators, criterion, max_depth
        self.min_samples_split, self.min_samples_leaf, self.max_features = min_samples_split, min_samples_leaf, max_features
        self.bootstrap, self.random_state = bootstrap, random_state
        self._check(self.get_params())
        self.classes_ = np.array([0, 1])
        self.estimators_ = None

    @staticmethod
    def _check(q):
        if q["criterion"] not in ("gini", "entropy"):
            raise ValueError("RandomForest: criterion must be 'gini' or 'entropy', got %r" % (q["criterion"],))
        if q["max_features"] not in (None, "sqrt", "log2"):
            raise ValueError("RandomForest: max_features must be None, 'sqrt' or 'log2', got %r" % (q["max_features"],))
        if q["max_depth"] is not None and int(q["max_depth"]) < 1:
            raise ValueError("RandomForest: max_depth must be None or >= 1, got %r" % (q["max_depth"],))
        if int(q["n_estimators"]) < 1 or int(q["min_samples_leaf"]) < 1 or int(q["min_samples_split"]) < 2:
            raise ValueError("RandomForest: n_estimators >= 1, min_samples_leaf >= 1 and min_samples_split >= 2 are required")

    def get_params(self):
        return {k: getattr(self, k) for k in self.PARAMS}

    def __repr__(self):
        parts = ["%s=%r" % (k, getattr(self, k)) for k in self.PARAMS if getattr(self, k) != self.DEFAULTS[k]]
        if self.random_state is not None:
            parts.append("random_state=%r" % (self.random_state,))
        return _sk_repr("RandomForestClassifier", parts)

    def _clone(self, **params):
        kw = dict(self.get_params(), random_state=self.random_state)
        kw.update(params)
        return type(self)(**kw)

    @staticmethod
    def n_max_features(max_features, p):
        """tree/_classes.py: None -> p, 'sqrt' -> max(1, int(sqrt(p))), 'log2' -> max(1, int(log2(p)))."""
        if max_features is None:
            return int(p)
        return max(1, int(np.sqrt(p))) if max_features == "sqrt" else max(1, int(np.log2(p)))

    def _engine_fits(self, ctx, X, y, jobs, export):
        """jobs: (parameter dict, rows_key, training rows) per forest; keys a dict lacks come from this estimator.  Every
        forest's trees go into one psk_forest_fit call, or into several when the leaf fractions of all trees would exceed
        SCRATCH_BYTES on the device.  Returns per job (proba[n][2] of every sample of X, the trees or None)."""
        y = np.asarray(y)
        if not set(y.tolist()) <= {0, 1}:
            raise ValueError("RandomForest: the two classes must be labelled 0 and 1")
        if self.random_state is None:
            raise ValueError("RandomForest: random_state must be an integer (the fit reproduces scikit-learn's for that seed)")
        n, p = X.shape
        draws = ForestDraws(self.random_state, n)
        per_call = max(1, self.SCRATCH_BYTES // (16 * n))
        params = [dict(self.get_params(), **q) for q, _, _ in jobs]
        for q in params:
            self._check(q)
        out, at = [], 0
        while at < len(jobs):
            end, n_trees = at, 0
            while end < len(jobs) and (end == at or n_trees + int(params[end]["n_estimators"]) <= per_call):
                n_trees += int(params[end]["n_estimators"])
                end += 1
            weight, state, tree_fit = [], [], []
            for f in range(at, end):
                q, (_, rows_key, rows) = params[f], jobs[f]
                for t in range(int(q["n_estimators"])):
                    state.append(draws.state(t))
                    weight.append(draws.weight(t, rows_key, rows, bool(q["bootstrap"])))
                    tree_fit.append(f - at)
            chunk = params[at:end]
            s0, s1, trees = ctx.forest_fit(X, y.astype(np.int32), np.array(weight), state, tree_fit, [q["criterion"] for q in chunk],
                                           [q["max_depth"] for q in chunk], [self.n_max_features(q["max_features"], p) for q in chunk],
                                           [int(q["min_samples_leaf"]) for q in chunk], [int(q["min_samples_split"]) for q in chunk],
                                           export=np.full(len(state), bool(export)))
            k = 0
            for f, q in enumerate(chunk):
                T = int(q["n_estimators"])
                out.append((np.column_stack([s0[f] / T, s1[f] / T]), trees[k:k + T] if export else None))
                k += T
            at = end
        return out, draws

    def fit(self, X, y, engine_ctx):
        X = np.asarray(X, dtype=np.float64)
        (res,), draws = self._engine_fits(engine_ctx, X, y, [({}, "all", np.arange(X.shape[0]))], True)
        return self._set_fit(res[1], draws, X.shape[1], X.shape[0])

    def _set_fit(self, trees, draws, n_features, n_samples):
        self.estimators_ = [ForestTree(self.criterion, self.max_depth, self.min_samples_split, self.min_samples_leaf, self.max_features,
                                       draws.seeds[t])._set_fit(fit, n_features) for t, fit in enumerate(trees)]
        self.n_features_in_, self._n_samples = int(n_features), int(n_samples)
        return self

    def predict_proba(self, X):
        """ForestClassifier.predict_proba: the trees' leaf fractions added in tree order, class by class, over their number."""
        X = np.asarray(X, dtype=np.float64)
        total = np.zeros((X.shape[0], 2))
        for e in self.estimators_:
            total += e.predict_proba(X)
        total /= len(self.estimators_)
        return total

    def predict(self, X):
        # np.argmax: class 1 only when its probability is strictly larger
        return self.classes_[np.argmax(self.predict_proba(X), axis=1)]

    def score(self, X, y):
        return np.float64(np.mean(self.predict(X) == np.asarray(y)))

    @property
    def feature_importances_(self):
        """The mean over the trees with more than one node of their normalised importances, renormalised by its sum."""
        rows = [e.tree_.compute_feature_importances() for e in self.estimators_ if e.tree_.node_count > 1]
        if not rows:
            return np.zeros(self.n_features_in_)
        mean = np.mean(rows, axis=0, dtype=np.float64)
        return mean / np.sum(mean)

    def _sklearn_state(self):
        """The fitted attributes of sklearn.ensemble.RandomForestClassifier (scikit-learn 1.7) but estimator / estimator_ /
        estimators_, which hold estimators of their own."""
        return dict(estimator_params=self.TREE_PARAMS, n_features_in_=self.n_features_in_, _n_samples=self._n_samples, n_outputs_=1,
                    classes_=np.array([0, 1]), n_classes_=2, _n_samples_bootstrap=self._n_samples if self.bootstrap else None)


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


class GridSearch:
    """GridSearchCV(model, {'C' | 'alpha': grid}, cv=int) with refit.  `engine_ctx` is only needed
    by fit(); the fitted object pickles without it.  GridSearch(model, {name: values, ...}, cv=int) searches several
    parameters (DecisionTree) in ParameterGrid's order: keys sorted, the last key varying fastest."""

    def __init__(self, estimator, param_name, grid=None, cv=None):
        self.estimator = estimator
        if isinstance(param_name, dict):
            self.param_name = None
            self.param_grid = {k: list(v) for k, v in param_name.items()}
        else:
            self.param_name = param_name
            self.param_grid = {param_name: list(grid)}
        self.cv = int(cv)

    def candidates(self):
        """sklearn.model_selection.ParameterGrid(param_grid) as a list."""
        import itertools
        keys = sorted(self.param_grid)
        return [dict(zip(keys, vals)) for vals in itertools.product(*(self.param_grid[k] for k in keys))]

    def _fit_trees(self, X, y, engine_ctx):
        """The search over an estimator whose engine call returns trees: every candidate x fold and every candidate's
        refit in one launch; a fold is scored from the class-1 fractions the engine returns for its held-out samples."""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y)
        if self.cv < 2:
            raise ValueError("k-fold cross-validation requires at least one train/test split by setting "
                             "n_splits=2 or more, got n_splits=%d." % self.cv)
        cand = self.candidates()
        folds = _cv.stratified_kfold(y, self.cv)
        fit_param = [q for q in cand for _ in range(self.cv)] + list(cand)
        fit_fold = [f for _ in cand for f in range(self.cv)] + [-1] * len(cand)
        fits = self.estimator._engine_fit(engine_ctx, X, y, folds, fit_param, fit_fold)
        scores = np.zeros((len(cand), self.cv))
        for gi in range(len(cand)):
            for f in range(self.cv):
                te = folds == f
                frac1 = fits[gi * self.cv + f]["frac"][te]
                # argmax of (n0 / n, n1 / n): class 1 only when it is the strict majority of the leaf
                scores[gi, f] = np.mean(self.estimator.classes_[(frac1 > 0.5).astype(int)] == y[te])
        self._store(cand, scores)
        best = self.estimator._clone(**cand[self.best_index_])
        self.best_estimator_ = best._set_fit(fits[len(cand) * self.cv + self.best_index_], X.shape[1])
        self.n_unique_columns_ = int(X.shape[1])
        self.n_splits_ = self.cv
        self.test_folds_ = folds
        return self

    def _store(self, cand, scores):
        mean = scores.mean(axis=1)
        self.cv_results_ = {"mean_test_score": mean, "std_test_score": scores.std(axis=1), "params": [dict(q) for q in cand],
                            "rank_test_score": _rank_with_nan(mean)}
        for f in range(self.cv):
            self.cv_results_["split%d_test_score" % f] = scores[:, f]
        self.best_index_ = int(np.argmin(self.cv_results_["rank_test_score"]))
        self.best_params_ = dict(cand[self.best_index_])
        self.best_score_ = float(mean[self.best_index_])

    def fit(self, X, y, engine_ctx):
        if getattr(self.estimator, "_fits_trees", False):
            return self._fit_trees(X, y, engine_ctx)
        if self.param_name is None:
            raise ValueError("a grid over several parameters is searched for tree estimators only")
        X_full = np.asarray(X, dtype=np.float64)
        y = np.asarray(y)
        n = len(y)
        # Identical columns (k-mers of one gene share a presence pattern) are solved once: an L1
        # optimum may place a pattern's weight on any of its copies, here on the first (which is also
        # what cyclic coordinate descent -- scikit-learn's Lasso -- does).
        if self.estimator._dedupe and X_full.shape[1] > getattr(self.estimator, "_dedupe_above", 0):
            X, first, inverse = _unique_columns(X_full)
        else:  # an L2 optimum spreads a pattern's weight over its copies: every column stays
            X, first = X_full, np.arange(X_full.shape[1])
        grid = self.param_grid[self.param_name]
        is_clf = self.estimator._is_classifier
        if self.cv < 2:
            raise ValueError("k-fold cross-validation requires at least one train/test split by setting "
                             "n_splits=2 or more, got n_splits=%d." % self.cv)
        folds = _cv.stratified_kfold(y, self.cv) if is_clf else _cv.kfold(n, self.cv)
        fit_param, fit_fold = [], []
        for g in grid:
            for f in range(self.cv):
                fit_param.append(float(g))
                fit_fold.append(f)
        for g in grid:  # refit candidates on everything: pick after scoring, all in one launch
            fit_param.append(float(g))
            fit_fold.append(-1)
        from_dec = getattr(self.estimator, "_scores_from_dec", False)
        if from_dec:   # SVC: the engine returns every fit's decision values on all samples, held-out ones included
            dual, rho, dec, iters = self.estimator._engine_fit(engine_ctx, X, y, folds, fit_param, fit_fold)
        else:
            coef, icpt, iters = self.estimator._engine_fit(engine_ctx, X, y, folds, fit_param, fit_fold)
        scores = np.zeros((len(grid), self.cv))
        for gi in range(len(grid)):
            for f in range(self.cv):
                j = gi * self.cv + f
                te = folds == f
                if from_dec:
                    scores[gi, f] = np.mean(self.estimator.classes_[(dec[j][te] <= 0).astype(int)] == y[te])
                    continue
                est = self.estimator._clone(**{self.param_name: grid[gi]})._set(coef[j], icpt[j])
                scores[gi, f] = est.score(X[te], y[te])
        mean = scores.mean(axis=1)
        std = scores.std(axis=1)
        self.cv_results_ = {"mean_test_score": mean, "std_test_score": std,
                            "params": [{self.param_name: g} for g in grid],
                            "rank_test_score": _rank_with_nan(mean)}
        for f in range(self.cv):
            self.cv_results_["split%d_test_score" % f] = scores[:, f]
        self.best_index_ = int(np.argmin(self.cv_results_["rank_test_score"]))
        self.best_params_ = {self.param_name: grid[self.best_index_]}
        self.best_score_ = float(mean[self.best_index_])
        j = len(grid) * self.cv + self.best_index_
        best = self.estimator._clone(**{self.param_name: grid[self.best_index_]})
        best.tol, best.max_iter = self.estimator.tol, self.estimator.max_iter
        if from_dec:
            self.best_estimator_ = best._set_fit(X_full, y, dual[j], rho[j], iters[j])
            if best.probability:
                best._fit_platt(engine_ctx, X_full, y)
        else:
            full = np.zeros(X_full.shape[1])
            full[first] = coef[j]
            self.best_estimator_ = best._set(full, icpt[j])
        self.n_unique_columns_ = int(X.shape[1])
        self.n_splits_ = self.cv
        self.n_iter_ = iters
        self.test_folds_ = folds
        return self

    def predict(self, X):
        return self.best_estimator_.predict(X)

    def predict_proba(self, X):
        return self.best_estimator_.predict_proba(X)

    def score(self, X, y):
        return self.best_estimator_.score(X, y)

    def to_sklearn_shell(self):
        """The same model as to_sklearn() builds, described for skpickle.dumps (no scikit-learn import), or None when
        the installed scikit-learn has no template."""
        from . import skpickle as sp
        be = self.best_estimator_
        if isinstance(be, DecisionTree):
            est = sp.make("DecisionTreeClassifier", criterion=be.criterion, max_depth=be.max_depth, **be._sklearn_state())
            if est is not None:
                est.state["tree_"] = sp.Reduced("sklearn.tree._tree", "Tree", (be.n_features_in_, np.array([2], dtype=np.int64), 1),
                                                be.tree_._sklearn_state())
            proto = sp.make("DecisionTreeClassifier", criterion=self.estimator.criterion, max_depth=self.estimator.max_depth)
        elif isinstance(be, SVC):
            kw = dict(kernel=be.kernel, gamma=be.gamma, tol=be.tol, max_iter=int(be.max_iter), probability=bool(be.probability))
            est = sp.make("SVC", C=be.C, **dict(kw, **be._sklearn_state()))
            proto = sp.make("SVC", **kw)
        elif isinstance(be, L1LogisticRegression):
            kw = dict(penalty=be.penalty, solver=be.solver, tol=be.tol, max_iter=int(be.max_iter))
            est = sp.make("LogisticRegression", C=be.C, classes_=np.array([0, 1]), coef_=be.coef_.copy(),
                          intercept_=be.intercept_.copy(), n_iter_=np.array([0], dtype=np.int32),
                          n_features_in_=be.n_features_in_, **kw)
            proto = sp.make("LogisticRegression", **kw)
        else:
            name = "Ridge" if isinstance(be, RidgeRegression) else "Lasso"
            kw = dict(tol=be.tol, max_iter=int(be.max_iter))
            est = sp.make(name, alpha=be.alpha, coef_=be.coef_.copy(), intercept_=be.intercept_,
                          n_iter_=None if name == "Ridge" else 0, n_features_in_=be.n_features_in_, **kw)
            proto = sp.make(name, **kw)
        if est is None or proto is None:
            return None
        return sp.make("GridSearchCV", estimator=proto, param_grid=self.param_grid, cv=self.cv, best_estimator_=est,
                       best_params_=dict(self.best_params_), best_index_=self.best_index_, best_score_=self.best_score_,
                       cv_results_=dict(self.cv_results_), n_splits_=self.n_splits_, refit_time_=0.0, multimetric_=False,
                       scorer_=None)

    def to_sklearn(self):
        """The same fitted model as real scikit-learn objects (for users whose downstream code
        insists on them); needs scikit-learn importable."""
        from sklearn.linear_model import Lasso, LogisticRegression, Ridge
        from sklearn.model_selection import GridSearchCV
        be = self.best_estimator_
        if isinstance(be, DecisionTree):
            from sklearn.tree import DecisionTreeClassifier
            from sklearn.tree._tree import Tree as SkTree
            est = DecisionTreeClassifier(criterion=be.criterion, max_depth=be.max_depth)
            est.__dict__.update(be._sklearn_state())
            est.tree_ = SkTree(be.n_features_in_, np.array([2], dtype=np.intp), 1)
            est.tree_.__setstate__(be.tree_._sklearn_state())
            proto = DecisionTreeClassifier(criterion=self.estimator.criterion, max_depth=self.estimator.max_depth)
        elif isinstance(be, SVC):
            from sklearn.svm import SVC as SkSVC
            kw = dict(kernel=be.kernel, gamma=be.gamma, tol=be.tol, max_iter=int(be.max_iter), probability=bool(be.probability))
            est = SkSVC(C=be.C, **kw)
            est.__dict__.update(be._sklearn_state())
            proto = SkSVC(**kw)
        elif isinstance(be, L1LogisticRegression):
            kw = dict(penalty=be.penalty, solver=be.solver, tol=be.tol, max_iter=int(be.max_iter))
            est = LogisticRegression(C=be.C, **kw)
            est.classes_ = np.array([0, 1])
            est.coef_, est.intercept_ = be.coef_.copy(), be.intercept_.copy()
            est.n_iter_ = np.array([0], dtype=np.int32)
            proto = LogisticRegression(**kw)
        else:
            cls = Ridge if isinstance(be, RidgeRegression) else Lasso
            est = cls(alpha=be.alpha, tol=be.tol, max_iter=int(be.max_iter))
            est.coef_, est.intercept_ = be.coef_.copy(), be.intercept_
            est.n_iter_ = None if cls is Ridge else 0
            proto = cls(tol=be.tol, max_iter=int(be.max_iter))
        if not isinstance(be, (SVC, DecisionTree)):
            est.n_features_in_ = be.n_features_in_
        gs = GridSearchCV(proto, self.param_grid, cv=self.cv)
        gs.best_estimator_, gs.best_params_ = est, dict(self.best_params_)
        gs.best_index_, gs.best_score_ = self.best_index_, self.best_score_
        gs.cv_results_ = dict(self.cv_results_)
        gs.n_splits_, gs.refit_time_, gs.multimetric_ = self.n_splits_, 0.0, False
        gs.scorer_ = None
        return gs


class RandomizedSearch(GridSearch):
    """RandomizedSearchCV(estimator, grid of lists, n_iter, cv=int, random_state=int) with refit, for RandomForest (get_best_model,
    modeling.py:1096-1099).  The candidates are scikit-learn's for that random_state: ParameterGrid(grid)[i] (keys sorted, the
    last key fastest) for the i that sample_without_replacement(grid_size, n_iter, random_state) yields.  Only its tracking
    selection is restated -- the regime n_iter / grid_size < 0.01, where the reference's default 25 of 10,692 lies; another
    n_iter is refused.  Every candidate x fold is fitted first, scored from the forests' sums on the held-out samples;
    only the best candidate is refitted on everything, with its trees returned."""
    TRACKING_RATIO = 0.01

    def __init__(self, estimator, param_grid, n_iter, cv, random_state=0):
        super().__init__(estimator, dict(param_grid), cv=cv)
        self.n_iter, self.random_state = int(n_iter), random_state

    def grid_size(self):
        return int(np.prod([len(v) for v in self.param_grid.values()]))

    @classmethod
    def max_n_iter(cls, grid_size):
        """The largest n_iter of the restated regime: n_iter / grid_size < 0.01."""
        k = int(grid_size * cls.TRACKING_RATIO)
        while k > 0 and not k / grid_size < cls.TRACKING_RATIO:
            k -= 1
        return k

    def grid_point(self, i):
        """ParameterGrid(grid)[i], its keys in ParameterGrid's order (the last sorted key first)."""
        out = {}
        for k in reversed(sorted(self.param_grid)):
            i, r = divmod(i, len(self.param_grid[k]))
            out[k] = self.param_grid[k][r]
        return out

    def sampled_indices(self):
        size = self.grid_size()
        n_iter = min(self.n_iter, size)           # scikit-learn caps n_iter at the grid size (with a warning)
        if n_iter < 1 or not n_iter / size < self.TRACKING_RATIO:
            raise ValueError("RandomizedSearch draws its candidates as scikit-learn does for n_iter / grid size < %g only: "
                             "n_iter must be 1..%d for this grid of %d points, got %d"
                             % (self.TRACKING_RATIO, self.max_n_iter(size), size, self.n_iter))
        rs = np.random.RandomState(int(self.random_state))
        taken, out = set(), []
        for _ in range(n_iter):                   # utils/_random.pyx::_sample_without_replacement_with_tracking_selection
            j = int(rs.randint(size))
            while j in taken:
                j = int(rs.randint(size))
            taken.add(j)
            out.append(j)
        return out

    def candidates(self):
        return [self.grid_point(i) for i in self.sampled_indices()]

    def fit(self, X, y, engine_ctx):
        if not getattr(self.estimator, "_fits_forest", False):
            raise ValueError("RandomizedSearch searches RandomForest only")
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y)
        if self.cv < 2:
            raise ValueError("k-fold cross-validation requires at least one train/test split by setting "
                             "n_splits=2 or more, got n_splits=%d." % self.cv)
        cand = self.candidates()
        folds = _cv.stratified_kfold(y, self.cv)
        rows = [np.nonzero(folds != f)[0] for f in range(self.cv)]
        jobs = [(q, f, rows[f]) for q in cand for f in range(self.cv)]
        fits, _ = self.estimator._engine_fits(engine_ctx, X, y, jobs, False)
        scores = np.zeros((len(cand), self.cv))
        for gi in range(len(cand)):
            for f in range(self.cv):
                te = folds == f
                proba = fits[gi * self.cv + f][0][te]
                scores[gi, f] = np.mean(self.estimator.classes_[np.argmax(proba, axis=1)] == y[te])
        self._store(cand, scores)
        self.best_estimator_ = self.estimator._clone(**cand[self.best_index_]).fit(X, y, engine_ctx)
        self.n_unique_columns_ = int(X.shape[1])
        self.n_splits_ = self.cv
        self.test_folds_ = folds
        return self

    @staticmethod
    def _forest_shell(sp, rf, fitted):
        kw = dict(rf.get_params(), random_state=rf.random_state, estimator=sp.make("DecisionTreeClassifier"),
                  estimator_params=RandomForest.TREE_PARAMS)
        if fitted:
            trees = []
            for e in rf.estimators_:
                t = sp.make("DecisionTreeClassifier", criterion=e.criterion, max_depth=e.max_depth, min_samples_split=e.min_samples_split,
                            min_samples_leaf=e.min_samples_leaf, max_features=e.max_features, random_state=e.random_state,
                            **e._sklearn_state())
                if t is None:
                    return None
                t.state["tree_"] = sp.Reduced("sklearn.tree._tree", "Tree", (e.n_features_in_, np.array([2], dtype=np.int64), 1),
                                              e.tree_._sklearn_state())
                trees.append(t)
            kw.update(rf._sklearn_state(), estimator_=sp.make("DecisionTreeClassifier"), estimators_=trees)
        return None if kw["estimator"] is None else sp.make("RandomForestClassifier", **kw)

    def to_sklearn_shell(self):
        from . import skpickle as sp
        est, proto = self._forest_shell(sp, self.best_estimator_, True), self._forest_shell(sp, self.estimator, False)
        if est is None or proto is None:
            return None
        return sp.make("RandomizedSearchCV", estimator=proto, param_distributions=self.param_grid, n_iter=self.n_iter,
                       random_state=self.random_state, cv=self.cv, best_estimator_=est, best_params_=dict(self.best_params_),
                       best_index_=self.best_index_, best_score_=self.best_score_, cv_results_=dict(self.cv_results_),
                       n_splits_=self.n_splits_, refit_time_=0.0, multimetric_=False, scorer_=None)

    def to_sklearn(self):
        from sklearn.ensemble import RandomForestClassifier
        from sklearn.model_selection import RandomizedSearchCV
        from sklearn.tree import DecisionTreeClassifier
        from sklearn.tree._tree import Tree as SkTree
        be = self.best_estimator_
        est = RandomForestClassifier(random_state=be.random_state, **be.get_params())
        est.__dict__.update({k: v for k, v in be._sklearn_state().items() if k != "estimator_params"})
        est.estimator_, est.estimators_ = DecisionTreeClassifier(), []
        for e in be.estimators_:
            t = DecisionTreeClassifier(criterion=e.criterion, max_depth=e.max_depth, min_samples_split=e.min_samples_split,
                                       min_samples_leaf=e.min_samples_leaf, max_features=e.max_features, random_state=e.random_state)
            t.__dict__.update(e._sklearn_state())
            t.tree_ = SkTree(e.n_features_in_, np.array([2], dtype=np.intp), 1)
            t.tree_.__setstate__(e.tree_._sklearn_state())
            est.estimators_.append(t)
        proto = RandomForestClassifier(random_state=self.estimator.random_state, **self.estimator.get_params())
        rs = RandomizedSearchCV(proto, self.param_grid, n_iter=self.n_iter, cv=self.cv, random_state=self.random_state)
        rs.best_estimator_, rs.best_params_ = est, dict(self.best_params_)
        rs.best_index_, rs.best_score_ = self.best_index_, self.best_score_
        rs.cv_results_ = dict(self.cv_results_)
        rs.n_splits_, rs.refit_time_, rs.multimetric_ = self.n_splits_, 0.0, False
        rs.scorer_ = None
        return rs


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


def _rank_with_nan(mean):
    """GridSearchCV's rank_test_score (sklearn/model_selection/_search.py::_store): rank 1 for everything when every mean
    is nan (the first candidate is then the best one), else nan counts as worse than the worst finite mean."""
    mean = np.asarray(mean, dtype=np.float64)
    if np.isnan(mean).all():
        return np.ones(len(mean), dtype=np.int32)
    return _rank_min(-np.nan_to_num(mean, nan=np.nanmin(mean) - 1.0))


def _rank_min(a):
    """scipy.stats.rankdata(a, method='min') for a 1-D array."""
    a = np.asarray(a)
    order = np.argsort(a, kind="stable")
    ranks = np.empty(len(a), dtype=np.int32)
    r = 0
    for pos, idx in enumerate(order):
        if pos == 0 or a[idx] != a[order[pos - 1]]:
            r = pos + 1
        ranks[idx] = r
    return ranks
