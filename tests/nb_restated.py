"""scikit-learn 1.7.2's BernoulliNB() for a 0/1 design and two classes restated in plain NumPy, with the joint log-likelihood
summed in the order psk_nb_jll states (include/psk.h, f8): the CPU yardstick of psk_nb_fit / psk_nb_jll
(csrc/solver_nb.hip), the reader of tests/golden/nb_kat.npz (tools/gen_nb_golden.py) and a stand-in for the engine in host tests.

  fit (sklearn/naive_bayes.py::_count, _update_feature_log_prob, _update_class_log_prior, alpha = 1):
      feature_count_[c][j] = training samples of class c with column j set; class_count_[c] = training samples of class c;
      feature_log_prob_ = log(feature_count_ + 1) - log(class_count_ + 2); class_log_prior_ = log(class_count_) - log(sum).
  joint log-likelihood (::_joint_log_likelihood): neg = log(1 - exp(feature_log_prob_)), delta = feature_log_prob_ - neg,
      jll = X . delta' + class_log_prior_ + sum_j neg.  scikit-learn adds the p + 2 terms of an element as a BLAS dot followed by
      + (class_log_prior_ + neg sum); the engine adds them in ITS stated order:
          64 partial sums; partial sum l starts from +0.0 and adds delta[c][j] for the set columns j = l, l + 64, l + 128, ...
          ascending; then a_l = a_l + a_(l xor m) for m = 32, 16, 8, 4, 2, 1, all l at once; jll = (a_0 + prior_c) + neg_sum_c.

Tolerance between the two orders (derived, not measured): two f64 summations of the same <= p + 2 terms in different orders
each stay within (p + 1) u sum|terms| of the exact sum (u = 2^-53), so they differ by at most
    tol_ic = 2 (p + 2) 2^-53 (sum_j x_ij |delta_cj| + |class_log_prior_c| + |neg_sum_c|)        -- jll_tolerance()
predict_proba is a function of jll_1 - jll_0 with slope <= 1/4, so tol_i0 + tol_i1 bounds it; labels are compared where
|jll_0 - jll_1| exceeds tol_i0 + tol_i1."""
import os

import numpy as np

LANES = 64
U = 2.0 ** -53


def counts(Xb, y, train):
    """(feature_count[2][p], class_count[2]) int32 over the samples of the boolean mask `train`."""
    Xb, y, train = np.asarray(Xb, dtype=bool), np.asarray(y), np.asarray(train, dtype=bool)
    fc = np.stack([Xb[train & (y == c)].sum(axis=0) for c in (0, 1)]).astype(np.int32)
    cc = np.array([np.count_nonzero(train & (y == c)) for c in (0, 1)], dtype=np.int32)
    return fc, cc


def log_attributes(fc, cc):
    """(feature_log_prob_, class_log_prior_) in scikit-learn's expressions."""
    fc, cc = np.asarray(fc, dtype=np.float64), np.asarray(cc, dtype=np.float64)
    return np.log(fc + 1.0) - np.log((cc + 1.0 * 2).reshape(-1, 1)), np.log(cc) - np.log(cc.sum())


def jll_terms(flp):
    """(delta[2][p], neg_sum[2]) as _joint_log_likelihood forms them."""
    neg = np.log(1 - np.exp(flp))
    return flp - neg, neg.sum(axis=1)


def sum_in_order(Xb, delta_c):
    """sum_j x_ij delta_c[j] for every row in the engine's order: column by column into partial sum j mod 64, then the butterfly."""
    Xb = np.asarray(Xb, dtype=bool)
    n, p = Xb.shape
    a = np.zeros((n, LANES))
    for j in range(p):
        lane = j % LANES
        a[:, lane] = np.where(Xb[:, j], a[:, lane] + delta_c[j], a[:, lane])
    for m in (32, 16, 8, 4, 2, 1):
        a = a + a[:, np.arange(LANES) ^ m]
    return a[:, 0]


def jll_from_terms(Xb, delta, prior, neg_sum):
    return np.stack([(sum_in_order(Xb, delta[c]) + prior[c]) + neg_sum[c] for c in (0, 1)], axis=1)


def jll_in_order(Xb, flp, clp):
    delta, neg_sum = jll_terms(flp)
    return jll_from_terms(Xb, delta, clp, neg_sum)


def jll_tolerance(Xb, flp, clp):
    """tol[n][2]: the bound of the module docstring."""
    Xb = np.asarray(Xb, dtype=bool)
    delta, neg_sum = jll_terms(flp)
    mass = Xb.astype(np.float64) @ np.abs(delta).T + np.abs(clp) + np.abs(neg_sum)
    return 2.0 * (Xb.shape[1] + 2) * U * mass


def logsumexp(jll):
    """Over the two classes, plainly (max + log(sum(exp(jll - max)))): the tests compare probabilities within the bound."""
    hi = jll.max(axis=1)
    return hi + np.log(np.exp(jll - hi[:, None]).sum(axis=1))


def proba(jll):
    return np.exp(jll - logsumexp(jll)[:, None])


class Engine:
    """Stands in for PskContext.nb_fit / nb_jll in CPU tests: the same arguments, results and refusals, computed here."""

    def nb_fit(self, X, y01, fold, fit_fold):
        X, y, fold = np.asarray(X), np.asarray(y01), np.asarray(fold)
        if not np.all((X == 0) | (X == 1)):
            raise ValueError("the design must be 0/1")
        fcs, ccs = [], []
        for f in fit_fold:
            fc, cc = counts(X != 0, y, fold != f)
            if cc.min() == 0:
                raise ValueError("the training samples are of one class")
            fcs.append(fc)
            ccs.append(cc)
        return np.stack(fcs), np.stack(ccs)

    def nb_jll(self, X, delta, class_log_prior, neg_sum):
        X = np.asarray(X)
        if not np.all((X == 0) | (X == 1)):
            raise ValueError("the design must be 0/1")
        delta = np.asarray(delta, dtype=np.float64)
        one = delta.ndim == 2
        delta = delta.reshape(-1, 2, X.shape[1])
        prior, neg = np.asarray(class_log_prior).reshape(-1, 2), np.asarray(neg_sum).reshape(-1, 2)
        out = np.stack([jll_from_terms(X != 0, delta[m], prior[m], neg[m]) for m in range(len(delta))])
        return out[0] if one else out


class Fixture:
    """tests/golden/nb_kat.npz: designs[d] = {X, y, fold, n, p, kind}; cases[d] = four dicts {held (-1: none), train (mask), fc,
    cc, flp, clp, jll, pred, proba}, scikit-learn's own, the last three on ALL rows of the design."""

    def __init__(self, path=None):
        self.path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nb_kat.npz")
        z = np.load(self.path, allow_pickle=False)
        self.sklearn_version = str(z["sklearn_version"])
        self.n_folds = int(z["n_folds"])
        self.designs, self.cases = [], []
        for d in range(int(z["n_designs"])):
            n, p = (int(v) for v in z["shape%d" % d])
            X = np.unpackbits(z["X%d" % d], axis=1)[:, :p].astype(np.float64)
            fold = z["fold%d" % d].astype(np.int32)
            self.designs.append(dict(X=X, y=z["y%d" % d].astype(np.int64), fold=fold, n=n, p=p, kind=str(z["kind"][d])))
            rows = []
            for k, held in enumerate([-1] + list(range(self.n_folds))):
                tag = "_%d_%d" % (d, k)
                rows.append(dict(held=held, train=fold != held, fc=z["fc" + tag], cc=z["cc" + tag], flp=z["flp" + tag], clp=z["clp" + tag],
                                 jll=z["jll" + tag], pred=z["pred" + tag].astype(np.int64), proba=z["proba" + tag]))
            self.cases.append(rows)
