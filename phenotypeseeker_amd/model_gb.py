"""Gradient-boosted trees on a 0/1 design: GradientBoosting over psk_gb_fit / psk_gb_decision.

The reference offers `-bc XGBC` and `-reg XGBR` and completes neither: get_model_name, set_model, set_hyperparameters and
get_best_model (modeling.py:186-207, :994-1103) have no case for them.  The contract here is scikit-learn 1.7.2's
GradientBoostingClassifier() / GradientBoostingRegressor() with their default parameters, fitted directly, no search -- scikit-learn's
gradient boosting, NOT XGBoost's regularised objective.  The engine fits every stage in one launch in a
stated arithmetic (include/psk.h, f16); the initial raw prediction, the loss per stage (train_score_), the importances and the
scikit-learn export are taken here on the host.  A raw prediction is init + the stages' learning_rate * value[leaf] added in stage
order: raw_in_order() below and psk_gb_decision give the same bits, so a prediction does not depend on where it was computed.
With counts=True the design holds k-mer counts (`--real_counts`): psk_gb_fit_counts / psk_gb_decision_counts, and every split
carries scikit-learn's threshold, x <= threshold going left."""
import numpy as np

from .model_search import _Estimator
from .model_trees import Tree

LOSSES = ("squared_error", "log_loss")
MAX_DEPTH, MAX_STAGES = 10, 1000


def raw_in_order(X, node_count, nodes, value, init_raw, learning_rate, max_depth, threshold=None):
    """psk_gb_decision in NumPy: X[n][p] (non-zero = present), the model in the engine's layout -> raw[n].  With threshold
    [n_estimators][cap] psk_gb_decision_counts: X holds counts and x <= threshold goes left."""
    X = np.asarray(X) != 0 if threshold is None else np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    rows = np.arange(n)
    F = np.full(n, float(init_raw))
    for t in range(len(node_count)):
        nd, node = nodes[t], np.zeros(n, dtype=np.int64)
        for _ in range(int(max_depth)):
            f = nd[node, 0]
            inner = f >= 0
            bit = X[rows, np.where(inner, f, 0)]
            if threshold is not None:
                bit = ~(bit <= threshold[t][node])
            node = np.where(inner, np.where(bit, nd[node, 2], nd[node, 1]), node)
        F = F + float(learning_rate) * value[t, node]
    return F


def expit(s):
    """scipy.special.expit without importing scipy, and without the overflow warning of exp(-s) at strongly negative s."""
    s = np.asarray(s, dtype=np.float64)
    e = np.exp(-np.abs(s))
    return np.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def init_raw_prediction(y, loss):
    """_gb.py::_init_raw_predictions over init=None: DummyRegressor(strategy='mean') gives np.average(y); DummyClassifier
    (strategy='prior') the class-1 share, clipped to [eps32, 1 - eps32] and put through the logit link, log(q / (1 - q))."""
    y = np.asarray(y, dtype=np.float64)
    if loss == "squared_error":
        return float(np.average(y))
    eps = np.finfo(np.float32).eps
    q = np.clip(np.bincount(y.astype(np.int64), minlength=2)[1] / len(y), eps, 1 - eps, dtype=np.float64)
    return float(np.log(q / (1 - q)))


def _depth(left, right):
    depth = np.zeros(len(left), dtype=np.int64)
    for k in range(len(left)):                     # pre-order: a child lies behind its parent
        if left[k] != -1:
            depth[left[k]] = depth[right[k]] = depth[k] + 1
    return int(depth.max())


class GradientBoosting(_Estimator):
    """sklearn.ensemble.GradientBoostingClassifier (loss='log_loss', two classes labelled 0 and 1) or GradientBoostingRegressor
    (loss='squared_error') on a 0/1 design; every other parameter at scikit-learn's default (criterion 'friedman_mse',
    subsample 1.0, min_samples_split 2, min_samples_leaf 1, max_features None, init None).  It is not searched: `modeling` fits
    it directly.  scikit-learn breaks ties between equally good splits by random_state; here the lowest column index wins, then
    the lowest threshold.  counts: the design holds k-mer counts (psk_gb_fit_counts); a switch of the engine, not a parameter of
    scikit-learn's: neither the repr nor the exported parameters show it."""

    def __init__(self, loss, n_estimators=100, learning_rate=0.1, max_depth=3, counts=False):
        if loss not in LOSSES:
            raise ValueError("GradientBoosting: loss must be 'squared_error' or 'log_loss', got %r" % (loss,))
        if isinstance(n_estimators, bool) or int(n_estimators) != n_estimators or not 1 <= int(n_estimators) <= MAX_STAGES:
            raise ValueError("GradientBoosting: n_estimators must be 1..%d on the GPU engine, got %r" % (MAX_STAGES, n_estimators))
        if isinstance(max_depth, bool) or max_depth is None or int(max_depth) != max_depth or not 1 <= int(max_depth) <= MAX_DEPTH:
            raise ValueError("GradientBoosting: max_depth must be 1..%d on the GPU engine, got %r" % (MAX_DEPTH, max_depth))
        if not (np.isfinite(learning_rate) and learning_rate > 0):
            raise ValueError("GradientBoosting: learning_rate must be a finite number above 0, got %r" % (learning_rate,))
        self.loss, self.n_estimators, self.learning_rate, self.max_depth = loss, int(n_estimators), float(learning_rate), int(max_depth)
        self.counts, self.threshold_ = bool(counts), None
        self.classes_ = np.array([0, 1]) if self._is_classifier else None

    @property
    def _is_classifier(self):
        return self.loss == "log_loss"

    @property
    def _sk_name(self):
        return "GradientBoostingClassifier" if self._is_classifier else "GradientBoostingRegressor"

    def _sklearn_params(self):
        return dict(n_estimators=self.n_estimators, learning_rate=self.learning_rate, max_depth=self.max_depth)

    def __repr__(self):
        # scikit-learn prints the parameters that differ from their defaults, in alphabetical order
        changed = [(k, v) for k, v in sorted(self._sklearn_params().items()) if v != dict(n_estimators=100, learning_rate=0.1, max_depth=3)[k]]
        return "%s(%s)" % (self._sk_name, ", ".join("%s=%r" % kv for kv in changed))

    def _clone(self, **params):
        kw = dict(self._sklearn_params(), loss=self.loss, counts=self.counts)
        kw.update(params)
        return type(self)(**kw)

    def fit(self, X, y, engine_ctx):
        Xb = np.asarray(X)
        y = np.asarray(y)
        if Xb.ndim != 2 or len(y) != Xb.shape[0]:
            raise ValueError("GradientBoosting: X must be samples x k-mers with one target per sample")
        if self._is_classifier and not set(y.tolist()) <= {0, 1}:
            raise ValueError("GradientBoosting: the two classes must be labelled 0 and 1")
        init = init_raw_prediction(y, self.loss)
        # (the count call takes the float64 values: it checks their range before the rounding to float32 would hide 2^24 + 1)
        engine_fit, Xe = (engine_ctx.gb_fit_counts, Xb.astype(np.float64)) if self.counts else (engine_ctx.gb_fit, Xb.astype(np.float32))
        fit = engine_fit(Xe, y.astype(np.float64), np.zeros(len(y), dtype=np.int32), [-1], self.loss,
                         self.n_estimators, self.learning_rate, self.max_depth, [init], staged=True)[0]
        return self._set_fit(fit, Xb.shape[1], init, y)

    def _set_fit(self, fit, n_features, init, y):
        """The fitted attributes from one dictionary of engine.PskContext.gb_fit; train_score_ from its staged values."""
        self.n_features_in_ = int(n_features)
        self.init_raw_ = float(init)
        self.node_count_ = np.array(fit["node_count"], dtype=np.int32)
        self.nodes_ = np.array(fit["nodes"], dtype=np.int32)
        self.value_ = np.array(fit["value"], dtype=np.float64)
        self.impurity_ = np.array(fit["impurity"], dtype=np.float64)
        self.threshold_ = np.array(fit["threshold"], dtype=np.float64) if self.counts else None
        self.n_estimators_ = len(self.node_count_)
        y = np.asarray(y, dtype=np.float64)
        if self._is_classifier:
            self.class_count_ = np.bincount(y.astype(np.int64), minlength=2)
        self.train_score_ = np.array([self._mean_loss(y, s) for s in fit["staged"]])
        return self

    def _mean_loss(self, y, raw):
        """What _gb.py records per stage: 2 x the mean of sklearn/_loss's half losses, (y - raw)^2 / 2 and log(1 + exp(raw)) - y raw."""
        if not self._is_classifier:
            return float(np.mean((y - raw) ** 2))
        return float(2.0 * np.mean(np.logaddexp(0.0, raw) - y * raw))

    @property
    def estimators_(self):
        """The stages as model_trees.Tree (value[node_count][1][1]: a regression tree's node values)."""
        trees = []
        for t in range(self.n_estimators_):
            k = int(self.node_count_[t])
            nd = self.nodes_[t, :k]
            tree = Tree(self.n_features_in_, nd[:, 0], nd[:, 1], nd[:, 2], nd[:, 3], np.zeros((k, 2)), self.impurity_[t, :k],
                        _depth(nd[:, 1], nd[:, 2]), threshold=self.threshold_[t, :k] if self.counts else None)
            tree.value = self.value_[t, :k].reshape(-1, 1, 1).copy()
            trees.append(tree)
        return trees

    @property
    def feature_importances_(self):
        """BaseGradientBoosting.feature_importances_: the mean over the stages with a split of each tree's unnormalised
        importances, divided by its sum."""
        rel = [t.compute_feature_importances(normalize=False) for t in self.estimators_ if t.node_count > 1]
        if not rel:
            return np.zeros(self.n_features_in_)
        avg = np.mean(rel, axis=0, dtype=np.float64)
        return avg / np.sum(avg)

    @property
    def _coef_column(self):
        return self.feature_importances_      # (modeling.py:1430-1432: importances stand in the coefficient column of tree models)

    def _model(self):
        return self.node_count_, self.nodes_, self.value_, self.init_raw_, self.learning_rate, self.max_depth

    def raw(self, X, engine_ctx=None):
        """raw[n]; on the device (psk_gb_decision, psk_gb_decision_counts for a counts model) when given an engine context, else
        in NumPy in the same order: the same bits."""
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_features_in_:
            raise ValueError("Expected input with %d features, got %d instead" % (self.n_features_in_, X.shape[-1]))
        if self.counts:
            count, nodes, value, init, rate, depth = self._model()
            if engine_ctx is not None:
                return engine_ctx.gb_decision_counts(X.astype(np.float64), count, nodes, value, self.threshold_, init, rate, depth)
            return raw_in_order(X, count, nodes, value, init, rate, depth, self.threshold_)
        if engine_ctx is not None:
            return engine_ctx.gb_decision((X != 0).astype(np.float32), *self._model())
        return raw_in_order(X, *self._model())

    def staged_raw(self, X):
        """[n_estimators][n]: the raw predictions after each stage (NumPy, the order of raw())."""
        count, nodes, value, init, rate, depth = self._model()
        thr = self.threshold_
        return np.array([raw_in_order(X, count[:t + 1], nodes[:t + 1], value[:t + 1], init, rate, depth, None if thr is None else thr[:t + 1])
                         for t in range(self.n_estimators_)])

    def predict_proba(self, X, engine_ctx=None):
        if not self._is_classifier:
            raise AttributeError("predict_proba is the classifier's")
        p1 = expit(self.raw(X, engine_ctx))
        return np.column_stack([1.0 - p1, p1])

    def predict(self, X, engine_ctx=None):
        raw = self.raw(X, engine_ctx)
        # (GradientBoostingClassifier.predict: class 1 from a raw value of 0 on)
        return self.classes_[(raw >= 0).astype(np.int64)] if self._is_classifier else raw

    def score(self, X, y, engine_ctx=None):
        if self._is_classifier:
            return np.float64(np.mean(self.predict(X, engine_ctx) == np.asarray(y)))
        # R^2 as sklearn.metrics.r2_score returns it (model_linear.LassoRegression.score)
        y = np.asarray(y, dtype=np.float64)
        if len(y) < 2:
            return np.float64(np.nan)
        res, tot = ((y - self.predict(X, engine_ctx)) ** 2).sum(), ((y - y.mean()) ** 2).sum()
        if tot == 0.0:
            return np.float64(1.0 if res == 0.0 else 0.0)
        return np.float64(1.0 - res / tot)

    # -- the fitted estimator as scikit-learn's ---------------------------------------------------------------------------
    def _sklearn(self, fitted=True):
        """A real sklearn.ensemble.GradientBoostingClassifier / GradientBoostingRegressor (scikit-learn is imported: there are
        no shells of these classes): estimators_ of real DecisionTreeRegressors on the node arrays, the fitted init_, _loss,
        train_score_ and n_estimators_, as BaseGradientBoosting.fit leaves them."""
        from sklearn import ensemble
        from sklearn.dummy import DummyClassifier, DummyRegressor
        from sklearn.tree import DecisionTreeRegressor
        from sklearn.tree._tree import Tree as SkTree
        from sklearn.utils import check_random_state
        est = getattr(ensemble, self._sk_name)(**self._sklearn_params())
        if not fitted:
            return est
        p = self.n_features_in_
        est.n_features_in_ = p
        if self._is_classifier:
            est.classes_, est.n_classes_ = np.array([0, 1]), 2
            c0, c1 = (int(c) for c in self.class_count_)
            est.init_ = DummyClassifier(strategy="prior").fit(np.zeros((c0 + c1, 1)), np.repeat([0.0, 1.0], [c0, c1]))
            est._loss = est._get_loss(sample_weight=None)
        else:
            est.init_ = DummyRegressor(strategy="mean").fit(np.zeros((1, 1)), np.array([self.init_raw_]))
            est._loss = est._get_loss(sample_weight=None)
        est.init_.n_features_in_ = p
        est.n_trees_per_iteration_, est.max_features_ = 1, p
        est._rng = check_random_state(est.random_state)
        est.estimators_ = np.empty((self.n_estimators_, 1), dtype=object)
        for t, tree in enumerate(self.estimators_):
            reg = DecisionTreeRegressor(criterion="friedman_mse", splitter="best", max_depth=self.max_depth, random_state=est._rng)
            reg.n_features_in_, reg.n_outputs_, reg.max_features_ = p, 1, p
            reg.tree_ = SkTree(p, np.array([1], dtype=np.intp), 1)
            reg.tree_.__setstate__(tree._sklearn_state())
            est.estimators_[t, 0] = reg
        est.train_score_ = self.train_score_.copy()
        est.n_estimators_ = self.n_estimators_
        return est

    def to_sklearn_shell(self):
        """None: skpickle has no shells of the gradient-boosting classes, `modeling` writes to_sklearn() through joblib."""
        return None

    def to_sklearn(self):
        return self._sklearn()


def from_sklearn(est):
    """GradientBoosting from a fitted scikit-learn GradientBoostingClassifier / GradientBoostingRegressor of the kind this
    package writes (two classes 0 / 1 or squared error, init None, one tree per stage, depth and stages within the engine's
    limits): what `prediction` turns a loaded model file into, so that its raw values come from psk_gb_decision -- or, when a
    split's threshold is not 0.5 (a model of a count design), a counts=True model whose raw values come from
    psk_gb_decision_counts.  None for anything else: scikit-learn itself then predicts."""
    try:
        name = type(est).__name__
        if name not in ("GradientBoostingClassifier", "GradientBoostingRegressor"):
            return None
        loss = "log_loss" if name == "GradientBoostingClassifier" else "squared_error"
        if est.loss != loss or est.init is not None or est.estimators_.shape[1] != 1:
            return None
        if loss == "log_loss" and list(est.classes_) != [0, 1]:
            return None
        m = GradientBoosting(loss, n_estimators=len(est.estimators_), learning_rate=est.learning_rate, max_depth=est.max_depth)
        cap, p = (2 << m.max_depth) - 1, int(est.n_features_in_)
        ne = len(est.estimators_)
        count, nodes = np.zeros(ne, dtype=np.int32), np.zeros((ne, cap, 4), dtype=np.int32)
        value, imp, thr = np.zeros((ne, cap)), np.zeros((ne, cap)), np.full((ne, cap), -2.0)
        counts = False
        for t in range(ne):
            tr = est.estimators_[t, 0].tree_
            k = int(tr.node_count)
            split = tr.children_left != -1
            if k > cap or not np.all(np.isfinite(tr.threshold[split])) or np.any(tr.children_left[split] != np.nonzero(split)[0] + 1):
                return None
            thr[t, :k] = np.where(split, tr.threshold, -2.0)
            counts = counts or bool(np.any(tr.threshold[split] != 0.5))
            count[t] = k
            nodes[t, :k, 0] = np.where(split, tr.feature, -2)
            nodes[t, :k, 1], nodes[t, :k, 2], nodes[t, :k, 3] = tr.children_left, tr.children_right, tr.n_node_samples
            value[t, :k], imp[t, :k] = tr.value[:, 0, 0], tr.impurity
        if loss == "log_loss":
            eps = np.finfo(np.float32).eps
            q = np.clip(float(est.init_.class_prior_[1]), eps, 1 - eps)
            init = float(np.log(q / (1 - q)))
        else:
            init = float(np.asarray(est.init_.constant_).reshape(-1)[0])
        m.n_features_in_, m.init_raw_, m.node_count_, m.nodes_, m.value_, m.impurity_ = p, init, count, nodes, value, imp
        m.n_estimators_ = ne
        if counts:
            m.counts, m.threshold_ = True, thr
        m.train_score_ = np.array(est.train_score_, dtype=np.float64)
        return m
    except (AttributeError, IndexError, TypeError, ValueError):
        return None
