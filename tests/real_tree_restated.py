"""count_tree_restated.py on a design of REAL values (any finite float32): the CPU yardstick of psk_tree_fit_real /
psk_forest_fit_real and the reader of tests/golden/real_tree_kat.npz (tools/gen_real_tree_golden.py).  The rules, as measured
on scikit-learn 1.7.2 (the golden file's probes hold them to what scikit-learn does, not to what its source reads):

  * any two float32 values that compare different are different values: a column is constant in a node when its in-bag values
    all compare equal, a candidate is every place where the sorted in-bag values change; -0.0 and +0.0 compare equal;
  * the threshold is lo / 2.0 + hi / 2.0 in f64, replaced by lo if that equals hi or is infinite; x <= threshold goes left, for
    every sample of the design;
  * inside a column the first strictly larger proxy in ascending order wins.

Everything else is count_tree_restated's: min_samples_leaf on distinct in-bag samples, the single tree's lowest column index,
the forest's Fisher-Yates walk.  The search inside a node is taken for all columns at once (NumPy sorts and integer sums);
the proxies themselves are tree_restated.proxy on Python floats, one evaluation per distinct pair of right-side sums."""
import math
import os

import numpy as np

from count_tree_restated import _Nodes, apply  # noqa: F401
from forest_restated import INT32_MAX, MAX_FEATURES, Xorshift, _params, encode_params, n_max_features, tree_draws, tree_seeds  # noqa: F401
from tree_restated import CRITERIA, EPS, impurity, proxy

CONSTANT, NO_SPLIT = -1, -2


def threshold(lo, hi):
    thr = lo / 2.0 + hi / 2.0
    if thr == hi or math.isinf(thr):
        thr = lo
    return thr


def node_gaps(Xm, w, w1, msl, criterion):
    """The search inside every column of a node.  Xm[m][p], w[m], w1[m]: value, weight and class-1 weight of the node's in-bag
    samples.  Returns per column: state (CONSTANT, NO_SPLIT, or the distinct in-bag samples on the right of the best gap),
    the best proxy, lo, hi, and the weighted / weighted class-1 sums on the right."""
    m, p = Xm.shape                                             # m >= 2: a node of one sample is a leaf before the search
    wn, w1n = int(w.sum()), int(w1.sum())
    order = np.argsort(Xm, axis=0, kind="stable")
    xs = np.take_along_axis(Xm, order, 0)
    change = xs[1:] != xs[:-1]                                  # row i - 1: the right side starts at rank i
    i = np.arange(1, m)[:, None]
    valid = change & (i >= msl) & (m - i >= msl)
    wr, wr1 = wn - np.cumsum(w[order], axis=0)[:-1], w1n - np.cumsum(w1[order], axis=0)[:-1]
    uniq, inv = np.unique((wr * (wn + 1) + wr1)[valid], return_inverse=True)
    vals = np.array([proxy(wn, w1n, int(k) // (wn + 1), int(k) % (wn + 1), criterion) for k in uniq], dtype=np.float64)
    P = np.full((m - 1, p), -np.inf)
    P[valid] = vals[inv.reshape(-1)]
    row, cols = np.argmax(P, axis=0), np.arange(p)              # the first maximum: the lowest threshold among equals
    state = np.where(valid.any(axis=0), m - 1 - row, np.where(change.any(axis=0), NO_SPLIT, CONSTANT))
    return state, P[row, cols], xs[row, cols], xs[row + 1, cols], wr[row, cols], wr1[row, cols]


def _split_or_leaf(lo, hi, c, c1, n_w, n1_w, w_total, node_imp, criterion):
    """Whether the best split is taken: (threshold, imp_r, imp_l) or None (rounding only, as on 0/1)."""
    imp_r = impurity(c - c1, c1, c, criterion)
    imp_l = impurity((n_w - n1_w) - (c - c1), n1_w - c1, n_w - c, criterion)
    improvement = (float(n_w) / float(w_total)) * (node_imp - (float(c) / float(n_w) * imp_r) - (float(n_w - c) / float(n_w) * imp_l))
    if improvement + EPS < 0.0:
        return None
    return threshold(lo, hi), imp_r, imp_l


def _design(X):
    X32 = np.asarray(X, dtype=np.float32)
    if not np.all(np.isfinite(X32)):
        raise ValueError("the design must be finite in float32")
    return X32.astype(np.float64)


def fit(X, y, train, max_depth, criterion):
    """count_tree_restated.fit on a real design (rounded to float32 first)."""
    X = _design(X)
    y1 = np.asarray(y) != 0
    train = np.asarray(train, dtype=bool)
    n_all, p = X.shape
    n_tot, n1_tot = int(train.sum()), int((train & y1).sum())
    nodes, frac = _Nodes(n_all), np.zeros(n_all)
    stack = [(np.ones(n_all, dtype=bool), -1, False, 0, impurity(n_tot - n1_tot, n1_tot, n_tot, criterion))]
    while stack:
        route, parent, is_left, depth, node_imp = stack.pop()
        members = route & train
        n, n1 = int(members.sum()), int((members & y1).sum())
        feat, take = -2, None
        if not (depth >= max_depth or n < 2 or node_imp <= EPS):
            st, P, lo, hi, wr, wr1 = node_gaps(X[members], np.ones(n, dtype=np.int64), y1[members].astype(np.int64), 1, criterion)
            if np.any(st >= 0):
                j = int(np.argmax(np.where(st >= 0, P, -np.inf)))          # the lowest column keeps a bit-equal proxy
                take = _split_or_leaf(float(lo[j]), float(hi[j]), int(wr[j]), int(wr1[j]), n, n1, n_tot, node_imp, criterion)
                if take is not None:
                    feat = j
        nid = nodes.add(parent, is_left, depth, feat, take[0] if take else -2.0, n, n - n1, n1, node_imp)
        if feat < 0:
            nodes.leaf[route] = nid
            frac[route] = float(n1) / float(n)
        else:
            go_left = X[:, feat] <= take[0]
            stack.append((route & ~go_left, nid, False, depth + 1, take[1]))
            stack.append((route & go_left, nid, True, depth + 1, take[2]))
    return nodes.result(frac=frac)


def fit_tree(X, y, weight, state, criterion, max_depth, max_features, min_samples_leaf, min_samples_split):
    """count_tree_restated.fit_tree on a real design (rounded to float32 first)."""
    X = _design(X)
    y1 = np.asarray(y) != 0
    w = np.asarray(weight, dtype=np.int64)
    n_all, p = X.shape
    inbag = w > 0
    w_total = int(w.sum())
    max_depth = INT32_MAX if not max_depth else int(max_depth)
    rng = Xorshift(state)
    features, constant = list(range(p)), [0] * p
    nodes, frac0, frac1 = _Nodes(n_all), np.zeros(n_all), np.zeros(n_all)
    w10 = int(w[y1].sum())
    stack = [(np.ones(n_all, dtype=bool), -1, False, 0, impurity(w_total - w10, w10, w_total, criterion), 0)]
    while stack:
        route, parent, is_left, depth, node_imp, n_known = stack.pop()
        members = route & inbag
        n, wn, w1 = int(members.sum()), int(w[members].sum()), int(w[members & y1].sum())
        feat, take, best = -2, None, -1
        if not (depth >= max_depth or n < min_samples_split or n < 2 * min_samples_leaf or node_imp <= EPS):
            st, P, lo, hi, wr, wr1 = node_gaps(X[members], w[members], (w * y1)[members], min_samples_leaf, criterion)
            f_i, n_visited, n_found, n_drawn, n_total = p, 0, 0, 0, n_known
            while f_i > n_total and (n_visited < max_features or n_visited <= n_found + n_drawn):
                n_visited += 1
                f_j = rng.rand_int(n_drawn, f_i - n_found)
                if f_j < n_known:
                    features[n_drawn], features[f_j] = features[f_j], features[n_drawn]
                    n_drawn += 1
                    continue
                f_j += n_found
                col = features[f_j]
                if st[col] == CONSTANT:
                    features[f_j], features[n_total] = features[n_total], features[f_j]
                    n_found += 1
                    n_total += 1
                    continue
                f_i -= 1
                features[f_i], features[f_j] = features[f_j], features[f_i]
                if st[col] != NO_SPLIT and (best < 0 or P[col] > P[best]):
                    best = col
            features[:n_known] = constant[:n_known]
            constant[n_known:n_known + n_found] = features[n_known:n_known + n_found]
            n_known = n_total
            if best >= 0:
                take = _split_or_leaf(float(lo[best]), float(hi[best]), int(wr[best]), int(wr1[best]), wn, w1, w_total, node_imp, criterion)
                if take is not None:
                    feat = best
        nid = nodes.add(parent, is_left, depth, feat, take[0] if take else -2.0, n, wn - w1, w1, node_imp)
        if feat < 0:
            nodes.leaf[route] = nid
            frac0[route] = float(wn - w1) / float(wn)
            frac1[route] = float(w1) / float(wn)
        else:
            go_left = X[:, feat] <= take[0]
            stack.append((route & ~go_left, nid, False, depth + 1, take[1], n_known))
            stack.append((route & go_left, nid, True, depth + 1, take[2], n_known))
    return nodes.result(frac0=frac0, frac1=frac1)


def seeded_tree(X, y, seed, criterion="gini", max_depth=None):
    """DecisionTreeClassifier(random_state=seed, criterion=..., max_depth=...) on all samples: one tree of unit weights with
    max_features = p whose generator state is RandomState(seed).randint(0, RAND_R_MAX)."""
    n, p = np.asarray(X).shape
    w, state = tree_draws(seed, np.arange(n), n, False)
    return fit_tree(X, y, w, state, criterion, max_depth, p, 1, 2)


class Engine:
    """Stands in for PskContext.tree_fit_real / forest_fit_real in CPU tests."""

    def tree_fit_real(self, X, y01, fold, fit_max_depth, fit_criterion, fit_fold):
        fold = np.asarray(fold)
        return [fit(X, y01, fold != ff, int(d), c if isinstance(c, str) else CRITERIA[int(c)])
                for d, c, ff in zip(fit_max_depth, fit_criterion, fit_fold)]

    def forest_fit_real(self, X, y01, tree_weight, tree_state, tree_fit, fit_criterion, fit_max_depth, fit_max_features,
                        fit_min_samples_leaf, fit_min_samples_split, export=None):
        n_fits, n = len(fit_criterion), np.asarray(X).shape[0]
        sum0, sum1 = np.zeros((n_fits, n)), np.zeros((n_fits, n))
        trees = []
        for t in range(len(tree_state)):
            f = int(tree_fit[t])
            c = fit_criterion[f]
            r = fit_tree(X, y01, tree_weight[t], tree_state[t], c if isinstance(c, str) else CRITERIA[int(c)], fit_max_depth[f],
                         fit_max_features[f], fit_min_samples_leaf[f], fit_min_samples_split[f])
            sum0[f] += r["frac0"]
            sum1[f] += r["frac1"]
            trees.append(r if export is None or export[t] else None)
        return sum0, sum1, trees


class Fixture:
    """tests/golden/real_tree_kat.npz: designs[d] = {X (float32 values as f64), y, n, p}; probes[k] = {x, y, threshold}: the
    root split scikit-learn made of a one-column design; dt[k] = {design, criterion, depth, invariant, tree (scikit-learn's
    under random_state 0)}; deep[k] = {design, seed, criterion, tree}: DecisionTreeClassifier(random_state=seed) at depth None;
    rf[k] = {design, seed, params, trees, proba}; the generator's own counts: n_invariant, n_invariant_3_splits."""

    def __init__(self, path=None):
        path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_tree_kat.npz")
        z = self.z = np.load(path, allow_pickle=False)
        self.sklearn_version = str(z["sklearn_version"])
        self.designs = []
        for d in range(int(z["n_designs"])):
            X32 = z["X%d" % d]
            assert X32.dtype == np.float32
            self.designs.append(dict(X32=X32, X=X32.astype(np.float64), y=z["y%d" % d].astype(np.int64), n=X32.shape[0], p=X32.shape[1]))
        pp = z["probe_ptr"]
        self.probes = [dict(x=z["probe_x"][int(pp[k]):int(pp[k + 1])], y=z["probe_y"][int(pp[k]):int(pp[k + 1])].astype(np.int64),
                            threshold=float(z["probe_threshold"][k])) for k in range(len(pp) - 1)]

        def tree(pre, t):
            a, b = int(z[pre + "node_ptr"][t]), int(z[pre + "node_ptr"][t + 1])
            g = lambda k: z[pre + "node_" + k][a:b]
            return dict(node_count=b - a, max_depth=int(z[pre + "tree_max_depth"][t]), feature=g("feature").astype(np.int64),
                        threshold=g("threshold").astype(np.float64), left=g("left").astype(np.int64), right=g("right").astype(np.int64),
                        n_node_samples=g("n").astype(np.int64), counts=g("counts").astype(np.int64), impurity=g("impurity"))
        self.dt = [dict(design=int(z["dt_design"][k]), criterion=CRITERIA[int(z["dt_criterion"][k])], depth=int(z["dt_depth"][k]),
                        invariant=bool(z["dt_invariant"][k]), tree=tree("dt_", k)) for k in range(len(z["dt_design"]))]
        self.deep = [dict(design=int(z["deep_design"][k]), seed=int(z["deep_seed"][k]), criterion=CRITERIA[int(z["deep_criterion"][k])],
                          tree=tree("deep_", k)) for k in range(len(z["deep_design"]))]
        self.rf, tptr, sptr = [], z["rf_tree_ptr"], z["rf_sample_ptr"]
        for k in range(len(z["rf_design"])):
            self.rf.append(dict(design=int(z["rf_design"][k]), seed=int(z["rf_seed"][k]), params=_params(z["rf_params"][k]),
                                trees=[tree("rf_", t) for t in range(int(tptr[k]), int(tptr[k + 1]))],
                                proba=z["rf_proba"][int(sptr[k]):int(sptr[k + 1])].reshape(-1, 2)))
        self.n_invariant, self.n_invariant_3_splits = int(z["n_invariant"]), int(z["n_invariant_3_splits"])
        self.n_adjacent_thresholds = int(z["n_adjacent_thresholds"])
