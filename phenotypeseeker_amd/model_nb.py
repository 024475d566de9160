"""The naive-Bayes estimator on a 0/1 design: BernoulliNB over psk_nb_fit / psk_nb_jll.

set_model makes BernoulliNB() for `-bc NB` (modeling.py:1034-1035), but the reference cannot complete that branch:
get_best_model (:1075-1103) has no NB case, best_model stays None (:623) and fit_model (:1216) fails on None.fit.  What the
rest of its code says about NB is consistent -- no grid-score block (:1220), `NA` in the coefficient column (:1440-1441),
the names "Naive Bayes" / "NB" (:204-206) --, so the contract here is scikit-learn 1.7.2's BernoulliNB() with its default
parameters, fitted directly, no search.

The engine counts (psk_nb_fit: integers, exact); the logarithms are taken HERE, in scikit-learn's own expressions, so that
feature_log_prob_ and class_log_prior_ are scikit-learn's attributes bit for bit.  The joint log-likelihood is a sum of
selected f64 values whose ORDER is fixed (include/psk.h, f8): psk_nb_jll on the device and jll_in_order() below give the same
bits, so a prediction does not depend on where it was computed.  scikit-learn's own sum (a BLAS dot, then + (class_log_prior_
+ neg_sum)) is another order of the same p + 2 terms; the two differ by rounding only."""
import numpy as np

from .model_search import _Estimator, _NoTemplate, _Twin

LANES = 64    # partial sums of the stated order: the lanes of a wave


def jll_in_order(Xb, delta, class_log_prior, neg_sum):
    """psk_nb_jll in NumPy for one model: Xb[n][p] booleans, delta[2][p], class_log_prior[2], neg_sum[2] -> jll[n][2].
    Partial sum l starts from +0.0 and adds delta[c][j] for the set columns j = l, l + 64, l + 128, ... in ascending order;
    then a_l = a_l + a_(l xor m) for m = 32, 16, 8, 4, 2, 1 over all l at once; the result is
    (a_0 + class_log_prior[c]) + neg_sum[c]."""
    Xb = np.asarray(Xb, dtype=bool)
    n, p = Xb.shape
    steps = -(-p // LANES)
    x = np.zeros((n, steps * LANES), dtype=bool)
    x[:, :p] = Xb
    d = np.zeros((2, steps * LANES))
    d[:, :p] = delta
    a = np.zeros((2, n, LANES))
    for s in range(steps):
        cols = slice(s * LANES, (s + 1) * LANES)
        for c in range(2):
            a[c] = np.where(x[:, cols], a[c] + d[c, cols], a[c])
    lane = np.arange(LANES)
    for m in (32, 16, 8, 4, 2, 1):
        a = a + a[:, :, lane ^ m]
    return np.stack([(a[c, :, 0] + class_log_prior[c]) + neg_sum[c] for c in range(2)], axis=1)


def logsumexp2(jll):
    """scipy.special.logsumexp(jll, axis=1) for two columns in scipy 1.15's form, without importing scipy: the maximal
    elements (m of them) are taken out of the sum, s = sum(exp(rest - max)) / m, result log1p(s) + log(m) + max."""
    hi, lo = np.max(jll, axis=1), np.min(jll, axis=1)
    tie = hi == lo
    m = np.where(tie, 2.0, 1.0)
    s = np.where(tie, 0.0, np.exp(lo - hi)) / m
    return np.log1p(s) + np.log(m) + hi


class BernoulliNB(_Estimator):
    """sklearn.naive_bayes.BernoulliNB() for two classes labelled 0 and 1: default parameters only (alpha=1.0,
    force_alpha=True, binarize=0.0, fit_prior=True, class_prior=None).  It is not searched: `modeling` fits it directly."""
    _is_classifier = True
    _DEFAULTS = dict(alpha=1.0, force_alpha=True, binarize=0.0, fit_prior=True, class_prior=None)

    def __init__(self, alpha=1.0, force_alpha=True, binarize=0.0, fit_prior=True, class_prior=None):
        given = dict(alpha=alpha, force_alpha=force_alpha, binarize=binarize, fit_prior=fit_prior, class_prior=class_prior)
        for k, v in self._DEFAULTS.items():
            g = given[k]
            # (True / None by identity; a number by value, and True is not the number 1.0)
            same = g is v if isinstance(v, bool) or v is None else isinstance(g, (int, float)) and not isinstance(g, bool) and g == v
            if not same:
                raise ValueError("BernoulliNB on the GPU engine takes scikit-learn's default parameters only: %s must be %r, got %r"
                                 % (k, v, given[k]))
        self.alpha, self.force_alpha, self.binarize, self.fit_prior, self.class_prior = 1.0, True, 0.0, True, None
        self.classes_ = np.array([0, 1])

    def __repr__(self):
        return "BernoulliNB()"

    def _clone(self, **params):
        return type(self)(**params)

    def _binarized(self, X):
        """scikit-learn's binarize(X, threshold=self.binarize): X > threshold."""
        return np.asarray(X) > self.binarize

    def fit(self, X, y, engine_ctx):
        Xb = self._binarized(X)
        y = np.asarray(y)
        if Xb.ndim != 2 or len(y) != Xb.shape[0]:
            raise ValueError("BernoulliNB: X must be samples x k-mers with one label per sample")
        if not set(y.tolist()) <= {0, 1}:
            raise ValueError("BernoulliNB: the two classes must be labelled 0 and 1")
        fc, cc = engine_ctx.nb_fit(Xb.astype(np.float32), y.astype(np.int32), np.zeros(len(y), dtype=np.int32), [-1])
        return self._set_counts(fc[0], cc[0])

    def _set_counts(self, feature_count, class_count):
        """The fitted attributes from the engine's integer counts, in scikit-learn's expressions (_count,
        _update_feature_log_prob, _update_class_log_prior of sklearn/naive_bayes.py)."""
        self.classes_ = np.array([0, 1])
        self.feature_count_ = np.asarray(feature_count, dtype=np.float64).reshape(2, -1)
        self.class_count_ = np.asarray(class_count, dtype=np.float64).reshape(2)
        self.n_features_in_ = int(self.feature_count_.shape[1])
        smoothed_fc = self.feature_count_ + self.alpha
        smoothed_cc = self.class_count_ + self.alpha * 2
        self.feature_log_prob_ = np.log(smoothed_fc) - np.log(smoothed_cc.reshape(-1, 1))
        self.class_log_prior_ = np.log(self.class_count_) - np.log(self.class_count_.sum())
        return self

    def _jll_terms(self):
        """(delta[2][p], class_log_prior[2], neg_sum[2]): what psk_nb_jll takes, as _joint_log_likelihood of scikit-learn
        forms them."""
        neg_prob = np.log(1 - np.exp(self.feature_log_prob_))
        return self.feature_log_prob_ - neg_prob, self.class_log_prior_, neg_prob.sum(axis=1)

    def _joint_log_likelihood(self, X, engine_ctx=None):
        """jll[n][2]; on the device (psk_nb_jll) when given an engine context, else in NumPy, in the same order of summation:
        the two give the same bits."""
        Xb = self._binarized(X)
        if Xb.ndim != 2 or Xb.shape[1] != self.n_features_in_:
            raise ValueError("Expected input with %d features, got %d instead" % (self.n_features_in_, Xb.shape[-1]))
        delta, prior, neg = self._jll_terms()
        if engine_ctx is not None:
            return engine_ctx.nb_jll(Xb.astype(np.float32), delta, prior, neg)
        return jll_in_order(Xb, delta, prior, neg)

    def predict_log_proba(self, X, engine_ctx=None):
        jll = self._joint_log_likelihood(X, engine_ctx)
        return jll - np.atleast_2d(logsumexp2(jll)).T

    def predict_proba(self, X, engine_ctx=None):
        return np.exp(self.predict_log_proba(X, engine_ctx))

    def predict(self, X, engine_ctx=None):
        # np.argmax: class 0 on equal likelihoods
        return self.classes_[np.argmax(self._joint_log_likelihood(X, engine_ctx), axis=1)]

    def score(self, X, y, engine_ctx=None):
        return np.float64(np.mean(self.predict(X, engine_ctx) == np.asarray(y)))

    # -- the fitted estimator as scikit-learn's ---------------------------------------------------------------------------
    def _sklearn(self, fitted=True):
        params = dict(self._DEFAULTS)
        if not fitted:
            return _Twin("BernoulliNB", "sklearn.naive_bayes", params)
        return _Twin("BernoulliNB", "sklearn.naive_bayes", params,
                     dict(n_features_in_=self.n_features_in_, classes_=np.array([0, 1]), class_count_=self.class_count_.copy(),
                          feature_count_=self.feature_count_.copy(), feature_log_prob_=self.feature_log_prob_.copy(),
                          class_log_prior_=self.class_log_prior_.copy()))

    def to_sklearn_shell(self):
        """The fitted model described for skpickle.dumps (no scikit-learn import), or None when the installed scikit-learn
        has no template."""
        try:
            return self._sklearn().shell()
        except _NoTemplate:
            return None

    def to_sklearn(self):
        """The same fitted model as a real sklearn.naive_bayes.BernoulliNB; needs scikit-learn importable."""
        return self._sklearn().real()
