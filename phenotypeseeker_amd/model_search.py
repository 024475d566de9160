"""The searches -- GridSearch, RandomizedSearch -- and what they ask of an estimator (_Estimator); the export of a fitted
search as its scikit-learn twin (_Twin), through skpickle without importing scikit-learn or as real scikit-learn objects."""
import importlib

import numpy as np

from . import cv as _cv
from . import skpickle as _sp


class _Estimator:
    """What a search asks of an estimator besides _is_classifier, classes_ and _clone(**params):
    _search(ctx, X, y, folds, cand, cv) -> (scores[len(cand)][cv], refit, found): the fold score of every candidate, a function
        from the best candidate's index to that candidate fitted on everything, and the attributes of the search that only
        the estimator knows (n_iter_ where fits iterate, n_unique_columns_ where columns were merged);
    _sklearn(fitted) -> _Twin: its scikit-learn twin, or with fitted=False the prototype a search holds as `estimator`;
    _coef_column: what `modeling` writes into the coefficient column of its k-mer table."""
    _warns_at_max_iter = False     # `modeling` prints scikit-learn's ConvergenceWarning when a fit of the search stopped at max_iter
    _randomized = False            # searched by RandomizedSearch (n_iter candidates drawn from the grid), not by GridSearch
    _tracking_draws_only = False   # a randomized search of it takes n_iter / grid size < 0.01 only (the forest's accepted range)

    def _new_search(self, params, grid, cv, n_iter):
        """The search `modeling` puts this estimator under, as the reference's get_best_model does (modeling.py:1096-1103)."""
        if self._randomized:
            return RandomizedSearch(self, params, n_iter, cv, random_state=self.random_state)
        return GridSearch(self, params, grid, cv)


def _launch_plan(cand, cv):
    """(parameters, held-out fold) of every fit of one launch: candidate gi on fold f is fit gi * cv + f; behind them every
    candidate on everything (fold -1), fit len(cand) * cv + gi: the best one is picked after scoring."""
    return [q for q in cand for _ in range(cv)] + list(cand), [f for _ in cand for f in range(cv)] + [-1] * len(cand)


def _launch_plan_of_numbers(cand, cv):
    """_launch_plan for an estimator that is searched over one number (C, alpha): that number per fit, not a dictionary."""
    if any(len(q) != 1 for q in cand):
        raise ValueError("a grid over several parameters is searched for tree estimators only")
    fit_param, fit_fold = _launch_plan(cand, cv)
    return [float(v) for q in fit_param for v in q.values()], fit_fold


def _fold_scores(cand, cv, folds, score):
    """scores[gi][f] = score(candidate gi, its fit on fold f, the mask of fold f's samples)."""
    scores = np.zeros((len(cand), cv))
    for gi, q in enumerate(cand):
        for f in range(cv):
            scores[gi, f] = score(q, gi * cv + f, folds == f)
    return scores


class _NoTemplate(Exception):
    """skpickle has no template of a class for the installed scikit-learn."""


class _Twin:
    """A scikit-learn object as data: class `name` of `module` built with the keywords `params`, then given the attributes
    `state` (what a fit adds).  `ctor_sets`: attributes the real constructor derives by itself, which a shell has to spell
    out.  A value may be a _Twin, a list of them, or a skpickle.Reduced (an object that pickles by __reduce__)."""

    def __init__(self, name, module, params, state=None, ctor_sets=None):
        self.name, self.module, self.params, self.state, self.ctor_sets = name, module, params, state or {}, ctor_sets or {}

    def shell(self):
        """For skpickle.dumps: no scikit-learn import."""
        attrs = {k: _each_twin(v, _Twin.shell) for k, v in {**self.params, **self.ctor_sets, **self.state}.items()}
        made = _sp.make(self.name, **attrs)
        if made is None:
            raise _NoTemplate(self.name)
        return made

    def real(self):
        """The scikit-learn object itself."""
        obj = getattr(importlib.import_module(self.module), self.name)(**{k: _each_twin(v, _Twin.real) for k, v in self.params.items()})
        obj.__dict__.update({k: _real_reduced(_each_twin(v, _Twin.real)) for k, v in self.state.items()})
        return obj


def _each_twin(v, f):
    if isinstance(v, list):
        return [_each_twin(e, f) for e in v]
    return f(v) if isinstance(v, _Twin) else v


def _real_reduced(v):
    if not isinstance(v, _sp.Reduced):
        return v
    obj = getattr(importlib.import_module(v.module), v.name)(*v.args)
    obj.__setstate__(v.state)
    return obj


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
        """The one search loop; what differs between estimators is their _search."""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y)
        if self.cv < 2:
            raise ValueError("k-fold cross-validation requires at least one train/test split by setting "
                             "n_splits=2 or more, got n_splits=%d." % self.cv)
        cand = self.candidates()
        folds = _cv.stratified_kfold(y, self.cv) if self.estimator._is_classifier else _cv.kfold(len(y), self.cv)
        scores, refit, found = self.estimator._search(engine_ctx, X, y, folds, cand, self.cv)
        self._store(cand, scores)
        self.best_estimator_ = refit(self.best_index_)
        self.n_unique_columns_ = int(X.shape[1])
        self.n_splits_ = self.cv
        self.__dict__.update(found)     # n_unique_columns_ of a de-duplicated design; n_iter_ of fits that iterate
        self.test_folds_ = folds
        return self

    def predict(self, X):
        return self.best_estimator_.predict(X)

    def predict_proba(self, X):
        return self.best_estimator_.predict_proba(X)

    def score(self, X, y):
        return self.best_estimator_.score(X, y)

    # -- the fitted search as scikit-learn's: RandomizedSearch differs in the class and in its constructor's keywords ----------
    _sk_name = "GridSearchCV"

    def _sk_params(self):
        return dict(param_grid=self.param_grid, cv=self.cv)

    def _twin(self):
        return _Twin(self._sk_name, "sklearn.model_selection", dict(estimator=self.estimator._sklearn(fitted=False), **self._sk_params()),
                     dict(best_estimator_=self.best_estimator_._sklearn(), best_params_=dict(self.best_params_),
                          best_index_=self.best_index_, best_score_=self.best_score_, cv_results_=dict(self.cv_results_),
                          n_splits_=self.n_splits_, refit_time_=0.0, multimetric_=False, scorer_=None))

    def to_sklearn_shell(self):
        """The same model as to_sklearn() builds, described for skpickle.dumps (no scikit-learn import), or None when
        the installed scikit-learn has no template."""
        try:
            return self._twin().shell()
        except _NoTemplate:
            return None

    def to_sklearn(self):
        """The same fitted model as real scikit-learn objects (for users whose downstream code
        insists on them); needs scikit-learn importable."""
        return self._twin().real()


class RandomizedSearch(GridSearch):
    """RandomizedSearchCV(estimator, grid of lists, n_iter, cv=int, random_state=int) with refit, for RandomForest and for SVC
    with the rbf kernel (get_best_model, modeling.py:1091-1099).  The candidates are scikit-learn's for that random_state:
    ParameterGrid(grid)[i] (keys sorted, the last key fastest) for the i that sample_without_replacement(grid_size, n_iter,
    random_state) yields, in each of its three selections (sampled_indices): the forest's default 25 of 10,692 is a tracking
    selection, the rbf default 25 of 13 x 13 = 169 a permutation's head.  TRACKING_RATIO / max_n_iter: the range `modeling`
    accepts for the forest."""
    TRACKING_RATIO = 0.01
    _sk_name = "RandomizedSearchCV"

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
        """sklearn.utils.random.sample_without_replacement(grid_size, n_iter, method="auto", random_state) as scikit-learn 1.7
        selects (utils/_random.pyx::_sample_without_replacement), r = n_iter / grid_size in f64:
          0.01 < r < 0.99   the first n_iter entries of RandomState.permutation(grid_size)
          r <= 0.01         tracking selection (r < 0.2 outside the band above): draw, and draw again on a repeat
          r >= 0.99         reservoir sampling: 0 .. n_iter - 1, entry j replaced by i when randint(0, i + 1) gives j < n_iter"""
        size = self.grid_size()
        n_iter = min(self.n_iter, size)           # scikit-learn caps n_iter at the grid size (with a warning)
        if n_iter < 1:
            raise ValueError("RandomizedSearch: n_iter must be at least 1, got %d" % self.n_iter)
        rs = np.random.RandomState(int(self.random_state))
        ratio = n_iter / size
        if 0.01 < ratio < 0.99:
            return [int(i) for i in rs.permutation(size)[:n_iter]]
        if ratio < 0.2:
            taken, out = set(), []
            for _ in range(n_iter):               # _sample_without_replacement_with_tracking_selection
                j = int(rs.randint(size))
                while j in taken:
                    j = int(rs.randint(size))
                taken.add(j)
                out.append(j)
            return out
        out = list(range(n_iter))                 # _sample_without_replacement_with_reservoir_sampling
        for i in range(n_iter, size):
            j = int(rs.randint(0, i + 1))
            if j < n_iter:
                out[j] = i
        return out

    def candidates(self):
        if not self.estimator._randomized:
            raise ValueError("RandomizedSearch searches an estimator that the reference puts under RandomizedSearchCV "
                             "(RandomForest, SVC with the rbf kernel), got %r" % (self.estimator,))
        size = self.grid_size()
        if self.estimator._tracking_draws_only and not (1 <= min(self.n_iter, size) and min(self.n_iter, size) / size < self.TRACKING_RATIO):
            raise ValueError("RandomizedSearch draws this estimator's candidates as scikit-learn does for n_iter / grid size < %g only: "
                             "n_iter must be 1..%d for this grid of %d points, got %d"
                             % (self.TRACKING_RATIO, self.max_n_iter(size), size, self.n_iter))
        return [self.grid_point(i) for i in self.sampled_indices()]

    def _sk_params(self):
        return dict(param_distributions=self.param_grid, n_iter=self.n_iter, random_state=self.random_state, cv=self.cv)


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
