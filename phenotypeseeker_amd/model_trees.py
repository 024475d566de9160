"""The tree estimators on a 0/1 design: DecisionTree over psk_tree_fit, RandomForest over psk_forest_fit with everything
scikit-learn draws from NumPy's RandomState drawn on the host (ForestDraws).  With counts=True they take a design of k-mer
counts through psk_tree_fit_counts / psk_forest_fit_counts and their trees carry scikit-learn's thresholds; with real=True a
design of any finite float32 values (the kept principal-component scores of --pca) through psk_tree_fit_real /
psk_forest_fit_real."""
import numpy as np

from .model_search import _Estimator, _Twin, _fold_scores, _launch_plan
from .skpickle import Reduced


class Tree:
    """The attributes of scikit-learn's tree_ (sklearn.tree._tree.Tree) for a two-class tree on a 0/1 design: nodes in
    pre-order, threshold 0.5 at a split and -2 at a leaf, value the class fractions ([node_count][1][2], scikit-learn >= 1.3)."""
    n_outputs, max_n_classes = 1, 2

    def __init__(self, n_features, feature, left, right, n_node_samples, counts, impurity, max_depth, weighted_n_node_samples=None,
                 threshold=None):
        """counts: the class counts by node; in a forest's tree they are weighted (bootstrap multiplicities) and
        weighted_n_node_samples is their sum, while n_node_samples counts the distinct samples.  threshold: by node, for a tree
        on a count design."""
        self.n_features = int(n_features)
        self.n_classes = np.array([2], dtype=np.int64)
        self.feature = np.asarray(feature, dtype=np.int64)
        self.children_left, self.children_right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
        self.n_node_samples = np.asarray(n_node_samples, dtype=np.int64)
        self.weighted_n_node_samples = (self.n_node_samples.astype(np.float64) if weighted_n_node_samples is None
                                        else np.asarray(weighted_n_node_samples, dtype=np.float64))
        self.impurity = np.asarray(impurity, dtype=np.float64)
        self.threshold = np.where(self.feature >= 0, 0.5, -2.0) if threshold is None else np.asarray(threshold, dtype=np.float64)
        self.value = (np.asarray(counts, dtype=np.float64) / self.weighted_n_node_samples[:, None]).reshape(-1, 1, 2)
        self.missing_go_to_left = np.zeros(len(self.feature), dtype=np.uint8)
        self.node_count, self.max_depth = len(self.feature), int(max_depth)
        self.capacity = self.node_count

    def apply(self, X):
        """The leaf of every row: (float32)x <= threshold goes left (scikit-learn's trees read X as float32; 0/1 and count
        values are unchanged by that rounding, principal-component scores are not)."""
        X = np.asarray(X, dtype=np.float32).astype(np.float64)
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


class DecisionTree(_Estimator):
    """sklearn.tree.DecisionTreeClassifier for two classes on a 0/1 design (set_model, modeling.py:1032-1033:
    DecisionTreeClassifier() under {'max_depth': 1..10, 'criterion': ['gini', 'entropy']}) over psk_tree_fit:
    scikit-learn's depth-first best-split builder with its default settings.  scikit-learn breaks ties between equally good
    splits by an unseeded random feature order; here the lowest column index wins.  counts: the design
    holds k-mer counts (psk_tree_fit_counts), real: it holds any finite float32 values (psk_tree_fit_real); switches of the
    engine, not parameters of scikit-learn's: neither the repr nor the exported parameters show them."""
    _is_classifier = True
    MAX_DEPTH = 10

    def __init__(self, criterion="gini", max_depth=None, counts=False, real=False):
        if criterion not in ("gini", "entropy"):
            raise ValueError("DecisionTree: criterion must be 'gini' or 'entropy', got %r" % (criterion,))
        self.criterion, self.max_depth, self.counts, self.real = criterion, max_depth, bool(counts), bool(real)
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
        kw = dict(criterion=self.criterion, max_depth=self.max_depth, counts=self.counts, real=self.real)
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
        engine_fit = ctx.tree_fit_real if self.real else ctx.tree_fit_counts if self.counts else ctx.tree_fit
        return engine_fit(X, y.astype(np.int32), folds, [int(dp) for dp in depth], crit, fit_fold)

    def fit(self, X, y, engine_ctx):
        X = np.asarray(X, dtype=np.float64)
        fits = self._engine_fit(engine_ctx, X, y, np.zeros(len(y), dtype=np.int32), [{}], [-1])
        return self._set_fit(fits[0], X.shape[1])

    def _set_fit(self, fit, n_features):
        self.tree_ = Tree(n_features, fit["feature"], fit["left"], fit["right"], fit["n_node_samples"], fit["counts"],
                          fit["impurity"], fit["max_depth"], threshold=fit.get("threshold"))
        self.n_features_in_ = int(n_features)
        self.n_outputs_, self.n_classes_, self.max_features_ = 1, np.int64(2), int(n_features)
        return self

    def _search(self, ctx, X, y, folds, cand, cv):
        """Every candidate x fold and every candidate's refit in one launch; a fold is scored from the class-1 fractions the
        engine returns for its held-out samples."""
        fit_param, fit_fold = _launch_plan(cand, cv)
        fits = self._engine_fit(ctx, X, y, folds, fit_param, fit_fold)
        # argmax of (n0 / n, n1 / n): class 1 only when it is the strict majority of the leaf
        scores = _fold_scores(cand, cv, folds, lambda q, j, te: np.mean(self.classes_[(fits[j]["frac"][te] > 0.5).astype(int)] == y[te]))
        return scores, lambda best: self._clone(**cand[best])._set_fit(fits[len(cand) * cv + best], X.shape[1]), {}

    @property
    def feature_importances_(self):
        return self.tree_.compute_feature_importances()

    @property
    def _coef_column(self):
        return self.feature_importances_      # (modeling.py:1430-1432: the importances stand in the coefficient column)

    def _sklearn_params(self):
        return dict(criterion=self.criterion, max_depth=self.max_depth)

    def _sklearn(self, fitted=True):
        """sklearn.tree.DecisionTreeClassifier; its tree_ pickles by __reduce__ (skpickle.Reduced)."""
        if not fitted:
            return _Twin("DecisionTreeClassifier", "sklearn.tree", self._sklearn_params())
        tree = Reduced("sklearn.tree._tree", "Tree", (self.n_features_in_, np.array([2], dtype=np.int64), 1), self.tree_._sklearn_state())
        return _Twin("DecisionTreeClassifier", "sklearn.tree", self._sklearn_params(), dict(self._sklearn_state(), tree_=tree))

    def _sklearn_state(self):
        """The fitted attributes of sklearn.tree.DecisionTreeClassifier (its __dict__ after fit, scikit-learn 1.7) without tree_."""
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

    def __init__(self, criterion="gini", max_depth=None, min_samples_split=2, min_samples_leaf=1, max_features="sqrt", random_state=None,
                 counts=False, real=False):
        super().__init__(criterion, max_depth, counts, real)
        self.min_samples_split, self.min_samples_leaf, self.max_features, self.random_state = (
            min_samples_split, min_samples_leaf, max_features, random_state)

    def _set_fit(self, fit, n_features):
        self.tree_ = Tree(n_features, fit["feature"], fit["left"], fit["right"], fit["n_node_samples"], fit["counts"],
                          fit["impurity"], fit["max_depth"], weighted_n_node_samples=np.asarray(fit["counts"]).sum(axis=1),
                          threshold=fit.get("threshold"))
        self.n_features_in_ = int(n_features)
        self.n_outputs_, self.n_classes_ = 1, np.int64(2)
        self.max_features_ = RandomForest.n_max_features(self.max_features, n_features)
        return self

    def _sklearn_params(self):
        return dict(super()._sklearn_params(), min_samples_split=self.min_samples_split, min_samples_leaf=self.min_samples_leaf,
                    max_features=self.max_features, random_state=self.random_state)

    def _sklearn_state(self):
        return dict(n_features_in_=self.n_features_in_, n_outputs_=1, classes_=np.array([0.0, 1.0]), n_classes_=np.int64(2),
                    max_features_=int(self.max_features_))


class RandomForest(_Estimator):
    """sklearn.ensemble.RandomForestClassifier for two classes on a 0/1 design (set_model, modeling.py:1030-1031) over
    psk_forest_fit: for an integer random_state, scikit-learn 1.7.2's forest to the node.  The seven
    parameters of the reference's grid plus random_state; everything else at scikit-learn's defaults.  counts: the design
    holds k-mer counts (psk_forest_fit_counts), real: any finite float32 values (psk_forest_fit_real); the engine switches of
    DecisionTree."""
    _is_classifier = True
    _randomized = True        # the reference searches its forest with RandomizedSearchCV (modeling.py:1096-1099)
    _tracking_draws_only = True    # ... with n_iter / grid size < 0.01, the range its search has always taken
    PARAMS = ("bootstrap", "criterion", "max_depth", "max_features", "min_samples_leaf", "min_samples_split", "n_estimators")
    DEFAULTS = dict(bootstrap=True, criterion="gini", max_depth=None, max_features="sqrt", min_samples_leaf=1, min_samples_split=2,
                    n_estimators=100)
    TREE_PARAMS = ("criterion", "max_depth", "min_samples_split", "min_samples_leaf", "min_weight_fraction_leaf", "max_features",
                   "max_leaf_nodes", "min_impurity_decrease", "random_state", "ccp_alpha", "monotonic_cst")   # estimator_params
    SCRATCH_BYTES = 1 << 30   # per engine call: 16 bytes per tree and sample of leaf fractions

    def __init__(self, n_estimators=100, criterion="gini", max_depth=None, min_samples_split=2, min_samples_leaf=1,
                 max_features="sqrt", bootstrap=True, random_state=0, counts=False, real=False):
        self.n_estimators, self.criterion, self.max_depth = n_estimators, criterion, max_depth
        self.min_samples_split, self.min_samples_leaf, self.max_features = min_samples_split, min_samples_leaf, max_features
        self.bootstrap, self.random_state, self.counts, self.real = bootstrap, random_state, bool(counts), bool(real)
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
        kw = dict(self.get_params(), random_state=self.random_state, counts=self.counts, real=self.real)
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
            engine_fit = ctx.forest_fit_real if self.real else ctx.forest_fit_counts if self.counts else ctx.forest_fit
            s0, s1, trees = engine_fit(X, y.astype(np.int32), np.array(weight), state, tree_fit, [q["criterion"] for q in chunk],
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
                                       draws.seeds[t], self.counts, self.real)._set_fit(fit, n_features) for t, fit in enumerate(trees)]
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

    @property
    def _coef_column(self):
        return self.feature_importances_

    def _search(self, ctx, X, y, folds, cand, cv):
        """Every candidate x fold is fitted first, scored from the forests' sums on the held-out samples; only the best
        candidate is refitted on everything, with its trees returned."""
        rows = [np.nonzero(folds != f)[0] for f in range(cv)]
        fits, _ = self._engine_fits(ctx, X, y, [(q, f, rows[f]) for q in cand for f in range(cv)], False)
        scores = _fold_scores(cand, cv, folds, lambda q, j, te: np.mean(self.classes_[np.argmax(fits[j][0][te], axis=1)] == y[te]))
        return scores, lambda best: self._clone(**cand[best]).fit(X, y, ctx), {}

    def _sklearn(self, fitted=True):
        """sklearn.ensemble.RandomForestClassifier (scikit-learn 1.7); estimator and estimator_params are its constructor's."""
        params = dict(self.get_params(), random_state=self.random_state)
        ctor_sets = dict(estimator=_Twin("DecisionTreeClassifier", "sklearn.tree", {}), estimator_params=self.TREE_PARAMS)
        if not fitted:
            return _Twin("RandomForestClassifier", "sklearn.ensemble", params, ctor_sets=ctor_sets)
        state = dict(n_features_in_=self.n_features_in_, _n_samples=self._n_samples, n_outputs_=1, classes_=np.array([0, 1]), n_classes_=2,
                     _n_samples_bootstrap=self._n_samples if self.bootstrap else None,
                     estimator_=_Twin("DecisionTreeClassifier", "sklearn.tree", {}), estimators_=[e._sklearn() for e in self.estimators_])
        return _Twin("RandomForestClassifier", "sklearn.ensemble", params, state, ctor_sets)
