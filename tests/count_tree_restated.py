"""tree_restated.py and forest_restated.py on a design of COUNTS (non-negative integers): the CPU yardstick of
psk_tree_fit_counts / psk_forest_fit_counts and the reader of tests/golden/count_tree_kat.npz (tools/gen_count_tree_golden.py).
What changes against the 0/1 builders is _splitter.pyx::node_split_best's search inside one column:

  * a column is constant in a node when the node's in-bag samples share one value;
  * otherwise its candidates are the gaps between consecutive distinct values present among those samples, ascending; a gap
    with fewer than min_samples_leaf distinct in-bag samples on a side is skipped; a candidate replaces the best only with
    a strictly larger proxy, so inside a column the lowest threshold wins among equals;
  * the threshold is lo / 2.0 + hi / 2.0 of the two values around the gap, x <= threshold goes left -- for EVERY sample of
    the design, also one whose value lies between lo and hi because it is held out or sits in another branch.

Across columns nothing changes: the single tree takes the lowest column index among bit-equal proxies, the forest the first
column of its Fisher-Yates walk.  Arithmetic as in tree_restated.py (Python floats, its impurity and proxy)."""
import math
import os

import numpy as np

from forest_restated import INT32_MAX, MAX_FEATURES, Xorshift, _params, encode_params, n_max_features, tree_draws, tree_seeds  # noqa: F401
from tree_restated import CRITERIA, EPS, impurity, proxy

CONSTANT, NO_SPLIT = "constant", "no split"


def best_gap(x, w, w1, msl, criterion, cache):
    """The search inside one column.  x, w, w1: value, weight and class-1 weight of the node's in-bag samples.  Returns
    CONSTANT, NO_SPLIT, or (proxy, lo, hi, distinct / weighted / weighted class-1 samples on the right)."""
    order = np.argsort(x, kind="stable")
    xs = x[order]
    if xs[0] == xs[-1]:
        return CONSTANT
    m, wn, w1n = len(xs), int(w.sum()), int(w1.sum())
    cw, cw1 = np.cumsum(w[order]), np.cumsum(w1[order])
    best = NO_SPLIT
    for i in np.nonzero(xs[1:] != xs[:-1])[0] + 1:         # the first sample of the right side
        if i < msl or m - i < msl:
            continue
        wr, wr1 = wn - int(cw[i - 1]), w1n - int(cw1[i - 1])
        v = cache.get((wr, wr1))
        if v is None:
            v = cache[(wr, wr1)] = proxy(wn, w1n, wr, wr1, criterion)
        if best is NO_SPLIT or v > best[0]:
            best = (v, float(xs[i - 1]), float(xs[i]), m - int(i), wr, wr1)
    return best


class _Nodes:
    """The node arrays both builders fill, in pre-order."""

    def __init__(self, n_all):
        self.feature, self.threshold, self.left, self.right, self.nns, self.counts, self.imp = [], [], [], [], [], [], []
        self.leaf = np.full(n_all, -1, dtype=np.int64)
        self.deepest = 0

    def add(self, parent, is_left, depth, feat, thr, n, c0, c1, node_imp):
        nid = len(self.feature)
        self.deepest = max(self.deepest, depth)
        self.feature.append(feat)
        self.threshold.append(thr if feat >= 0 else -2.0)
        self.left.append(nid + 1 if feat >= 0 else -1)
        self.right.append(-1)
        self.nns.append(n)
        self.counts.append((c0, c1))
        self.imp.append(node_imp)
        if parent >= 0 and not is_left:
            self.right[parent] = nid
        return nid

    def result(self, **more):
        return dict(node_count=len(self.feature), max_depth=self.deepest, feature=np.array(self.feature, dtype=np.int64),
                    threshold=np.array(self.threshold, dtype=np.float64), left=np.array(self.left, dtype=np.int64),
                    right=np.array(self.right, dtype=np.int64), n_node_samples=np.array(self.nns, dtype=np.int64),
                    counts=np.array(self.counts, dtype=np.int64).reshape(-1, 2), impurity=np.array(self.imp, dtype=np.float64),
                    leaf=self.leaf, **more)


def _split_or_leaf(best, n_w, n1_w, w_total, node_imp, criterion):
    """Whether the best split (a best_gap tuple) is taken: (threshold, imp_r, imp_l) or None (rounding only, as on 0/1)."""
    _, lo, hi, _, c, c1 = best
    imp_r = impurity(c - c1, c1, c, criterion)
    imp_l = impurity((n_w - n1_w) - (c - c1), n1_w - c1, n_w - c, criterion)
    improvement = (float(n_w) / float(w_total)) * (node_imp - (float(c) / float(n_w) * imp_r) - (float(n_w - c) / float(n_w) * imp_l))
    if improvement + EPS < 0.0:
        return None
    return lo / 2.0 + hi / 2.0, imp_r, imp_l


def fit(X, y, train, max_depth, criterion):
    """tree_restated.fit on a count design; the result has `threshold` as well."""
    X = np.asarray(X, dtype=np.float64)
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
            w, cache, best = np.ones(n, dtype=np.int64), {}, None
            for j in range(p):                         # ascending: the lowest column keeps a bit-equal proxy
                g = best_gap(X[members, j], w, y1[members].astype(np.int64), 1, criterion, cache)
                if g not in (CONSTANT, NO_SPLIT) and (best is None or g[0] > best[1][0]):
                    best = (j, g)
            if best is not None:
                take = _split_or_leaf(best[1], n, n1, n_tot, node_imp, criterion)
                if take is not None:
                    feat = best[0]
        nid = nodes.add(parent, is_left, depth, feat, take[0] if take else -2.0, n, n - n1, n1, node_imp)
        if feat < 0:
            nodes.leaf[route] = nid
            frac[route] = float(n1) / float(n)
        else:
            go_left = X[:, feat] <= take[0]
            nr, nr1 = best[1][3], best[1][5]
            assert int((members & ~go_left).sum()) == nr and int((members & ~go_left & y1).sum()) == nr1
            stack.append((route & ~go_left, nid, False, depth + 1, take[1]))
            stack.append((route & go_left, nid, True, depth + 1, take[2]))
    return nodes.result(frac=frac)


def fit_tree(X, y, weight, state, criterion, max_depth, max_features, min_samples_leaf, min_samples_split):
    """forest_restated.fit_tree on a count design; the result has `threshold` as well."""
    X = np.asarray(X, dtype=np.float64)
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
        feat, take, best = -2, None, None
        if not (depth >= max_depth or n < min_samples_split or n < 2 * min_samples_leaf or node_imp <= EPS):
            wm, w1m, cache, seen = w[members], (w * y1)[members], {}, {}
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
                g = seen.get(col)
                if g is None:
                    g = seen[col] = best_gap(X[members, col], wm, w1m, min_samples_leaf, criterion, cache)
                if g is CONSTANT:
                    features[f_j], features[n_total] = features[n_total], features[f_j]
                    n_found += 1
                    n_total += 1
                    continue
                f_i -= 1
                features[f_i], features[f_j] = features[f_j], features[f_i]
                if g is not NO_SPLIT and (best is None or g[0] > best[1][0]):
                    best = (col, g)
            features[:n_known] = constant[:n_known]
            constant[n_known:n_known + n_found] = features[n_known:n_known + n_found]
            n_known = n_total
            if best is not None:
                take = _split_or_leaf(best[1], wn, w1, w_total, node_imp, criterion)
                if take is not None:
                    feat = best[0]
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


def apply(t, X):
    """The leaf of every row of X by the tree's thresholds."""
    X = np.asarray(X, dtype=np.float64)
    node = np.zeros(X.shape[0], dtype=np.int64)
    for _ in range(t["max_depth"]):
        f = t["feature"][node]
        inner = f >= 0
        go_left = X[np.arange(X.shape[0]), np.where(inner, f, 0)] <= t["threshold"][node]
        node = np.where(inner, np.where(go_left, t["left"][node], t["right"][node]), node)
    return node


def _check_counts(X):
    X = np.asarray(X, dtype=np.float64)
    if not np.all((X >= 0) & (X <= 1 << 24) & (X == np.floor(X))):
        raise ValueError("the design must hold integers in 0 .. 2^24")
    return X


class Engine:
    """Stands in for PskContext.tree_fit_counts / forest_fit_counts in CPU tests."""

    def tree_fit_counts(self, X, y01, fold, fit_max_depth, fit_criterion, fit_fold):
        X, fold = _check_counts(X), np.asarray(fold)
        return [fit(X, y01, fold != ff, int(d), c if isinstance(c, str) else CRITERIA[int(c)])
                for d, c, ff in zip(fit_max_depth, fit_criterion, fit_fold)]

    def forest_fit_counts(self, X, y01, tree_weight, tree_state, tree_fit, fit_criterion, fit_max_depth, fit_max_features,
                          fit_min_samples_leaf, fit_min_samples_split, export=None):
        X = _check_counts(X)
        n_fits, n = len(fit_criterion), X.shape[0]
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
    """tests/golden/count_tree_kat.npz: designs[d] = {X, y, n, p}; dt[k] = {design, criterion, depth, invariant, tree
    (scikit-learn's under random_state 0, in fit()'s layout without leaf / frac)}; rf[k] = {design, seed, params, trees,
    proba}; search: the recorded RandomizedSearchCV."""

    def __init__(self, path=None):
        path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "count_tree_kat.npz")
        z = self.z = np.load(path, allow_pickle=False)
        self.sklearn_version = str(z["sklearn_version"])
        self.designs = []
        for d in range(int(z["n_designs"])):
            X = z["X%d" % d].astype(np.float64)
            self.designs.append(dict(X=X, y=z["y%d" % d].astype(np.int64), n=X.shape[0], p=X.shape[1]))

        def tree(pre, t):
            a, b = int(z[pre + "node_ptr"][t]), int(z[pre + "node_ptr"][t + 1])
            g = lambda k: z[pre + "node_" + k][a:b]
            return dict(node_count=b - a, max_depth=int(z[pre + "tree_max_depth"][t]), feature=g("feature").astype(np.int64),
                        threshold=g("threshold").astype(np.float64), left=g("left").astype(np.int64), right=g("right").astype(np.int64),
                        n_node_samples=g("n").astype(np.int64), counts=g("counts").astype(np.int64), impurity=g("impurity"))
        self.dt = [dict(design=int(z["dt_design"][k]), criterion=CRITERIA[int(z["dt_criterion"][k])], depth=int(z["dt_depth"][k]),
                        invariant=bool(z["dt_invariant"][k]), tree=tree("dt_", k)) for k in range(len(z["dt_design"]))]
        self.rf, tptr, sptr = [], z["rf_tree_ptr"], z["rf_sample_ptr"]
        for k in range(len(z["rf_design"])):
            self.rf.append(dict(design=int(z["rf_design"][k]), seed=int(z["rf_seed"][k]), params=_params(z["rf_params"][k]),
                                trees=[tree("rf_", t) for t in range(int(tptr[k]), int(tptr[k + 1]))],
                                proba=z["rf_proba"][int(sptr[k]):int(sptr[k + 1])].reshape(-1, 2)))
        self.search = dict(design=int(z["rs_design"]), cv=int(z["rs_cv"]), seed=int(z["rs_seed"]), n_iter=int(z["rs_n_iter"]),
                           grid={"bootstrap": [bool(v) for v in z["rs_grid_bootstrap"]], "criterion": [CRITERIA[int(v)] for v in z["rs_grid_criterion"]],
                                 "max_depth": [int(v) or None for v in z["rs_grid_max_depth"]],
                                 "max_features": [MAX_FEATURES[int(v)] for v in z["rs_grid_max_features"]],
                                 "min_samples_leaf": [int(v) for v in z["rs_grid_min_samples_leaf"]],
                                 "min_samples_split": [int(v) for v in z["rs_grid_min_samples_split"]],
                                 "n_estimators": [int(v) for v in z["rs_grid_n_estimators"]]},
                           params=[_params(r) for r in z["rs_params"]], splits=z["rs_splits"], mean=z["rs_mean"], rank=z["rs_rank"],
                           best=_params(z["rs_best"]), proba=z["rs_proba"])
