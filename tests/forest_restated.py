"""scikit-learn 1.7.2's RandomForestClassifier for a 0/1 design and two classes under a FIXED seed, restated in plain NumPy /
Python floats: the CPU yardstick of psk_forest_fit (csrc/solver_forest.hip) and the reader of tests/golden/forest_kat.npz
(tools/gen_forest_golden.py).  Unlike the single decision tree (tree_restated.py), nothing is left to a tie rule: with a seed
every draw of scikit-learn is determined, and the restatement follows them to the node.

  forest (ensemble/_forest.py, _base.py::_set_random_states): rs = RandomState(S); tree t's seed is
      rs.randint(np.iinfo(np.int32).max), drawn in tree order before any fit.  With bootstrap, tree t's sample weights are
      bincount(RandomState(seed_t).randint(0, n, n, dtype=int32), minlength=n); without, ones.
  tree (tree/_classes.py, _splitter.pyx::Splitter.init): the splitter's generator state is
      RandomState(seed_t).randint(0, 2147483647) of a fresh RandomState.
  draws (utils/_random.pxd::our_rand_r, tree/_utils.pyx::rand_int): a 32-bit xorshift, value = state % 2^31.
  node split (_splitter.pyx::node_split_best): the Fisher-Yates walk over features[] with the n_known / n_drawn / n_found
      constant bookkeeping and the two memcpy's through constant_features[]; the first column in VISIT order with a strictly
      larger proxy wins.
  builder (_tree.pyx::DepthFirstTreeBuilder.build): pre-order, left (bit clear) first; n_node_samples counts distinct in-bag
      samples, class counts / impurities / proxies use the weights.

Arithmetic as in tree_restated.py: Python floats, math.log, scikit-learn's expressions in their order."""
import math
import os

import numpy as np

from tree_restated import CRITERIA, EPS, impurity

RAND_R_MAX = 2147483647
INT32_MAX = int(np.iinfo(np.int32).max)
MAX_FEATURES = (None, "sqrt", "log2")
# set_model's grid of the reference (modeling.py:1057-1068): 10,692 points
REFERENCE_GRID = {"bootstrap": [True, False], "max_depth": [4, 5, 6, 7, 8, 10, 20, 100, None], "max_features": [None, "sqrt", "log2"],
                  "min_samples_leaf": [1, 2, 4], "min_samples_split": [2, 5, 10],
                  "n_estimators": [10, 20, 40, 60, 80, 100, 120, 140, 160, 180, 200], "criterion": ["gini", "entropy"]}


class Xorshift:
    """our_rand_r + rand_int."""

    def __init__(self, state):
        self.s = int(state) & 0xFFFFFFFF

    def rand_int(self, lo, hi):
        s = self.s or 1
        s ^= (s << 13) & 0xFFFFFFFF
        s ^= s >> 17
        s ^= (s << 5) & 0xFFFFFFFF
        self.s = s
        return lo + (s % (RAND_R_MAX + 1)) % (hi - lo)


def n_max_features(max_features, p):
    if max_features is None:
        return p
    if max_features == "sqrt":
        return max(1, int(np.sqrt(p)))
    if max_features == "log2":
        return max(1, int(np.log2(p)))
    return int(max_features)


def fit_tree(X, y, weight, state, criterion, max_depth, max_features, min_samples_leaf, min_samples_split):
    """One tree on the samples of weight[n] > 0 (integer multiplicities) of the 0/1 design X[n][p]; `state` is the splitter's
    generator state, max_depth 0 / None means no limit, max_features a number of columns.  Returns the node arrays in
    pre-order (counts: the weighted class counts), and for EVERY sample, weight 0 included, its leaf and the leaf's two class
    fractions."""
    Xb = np.asarray(X) != 0
    y1 = np.asarray(y) != 0
    w = np.asarray(weight, dtype=np.int64)
    n_all, p = Xb.shape
    inbag = w > 0
    w_total = int(w.sum())
    max_depth = INT32_MAX if not max_depth else int(max_depth)
    rng = Xorshift(state)
    features, constant = list(range(p)), [0] * p
    feature, left, right, nns, counts, imp = [], [], [], [], [], []
    leaf = np.full(n_all, -1, dtype=np.int64)
    frac0, frac1 = np.zeros(n_all), np.zeros(n_all)
    wn0, w10 = w_total, int(w[y1].sum())
    stack = [(np.ones(n_all, dtype=bool), -1, False, 0, impurity(wn0 - w10, w10, wn0, criterion), 0)]
    deepest = 0
    while stack:
        route, parent, is_left, depth, node_imp, n_known = stack.pop()
        members = route & inbag
        n, wn, w1 = int(members.sum()), int(w[members].sum()), int(w[members & y1].sum())
        is_leaf = depth >= max_depth or n < min_samples_split or n < 2 * min_samples_leaf or node_imp <= EPS
        feat = -2
        if not is_leaf:
            Xm = Xb[members]
            nr = Xm.sum(axis=0).astype(np.int64)
            wr = (Xm * w[members][:, None]).sum(axis=0).astype(np.int64)
            wr1 = (Xm * (w * y1)[members][:, None]).sum(axis=0).astype(np.int64)
            f_i, n_visited, n_found, n_drawn, n_total = p, 0, 0, 0, n_known
            best, best_proxy = -1, -math.inf
            while f_i > n_total and (n_visited < max_features or n_visited <= n_found + n_drawn):
                n_visited += 1
                f_j = rng.rand_int(n_drawn, f_i - n_found)
                if f_j < n_known:
                    features[n_drawn], features[f_j] = features[f_j], features[n_drawn]
                    n_drawn += 1
                    continue
                f_j += n_found
                col = features[f_j]
                if nr[col] == 0 or nr[col] == n:
                    features[f_j], features[n_total] = features[n_total], features[f_j]
                    n_found += 1
                    n_total += 1
                    continue
                f_i -= 1
                features[f_i], features[f_j] = features[f_j], features[f_i]
                if n - nr[col] < min_samples_leaf or nr[col] < min_samples_leaf:
                    continue
                c, c1 = int(wr[col]), int(wr1[col])
                ir = impurity(c - c1, c1, c, criterion)
                il = impurity((wn - w1) - (c - c1), w1 - c1, wn - c, criterion)
                proxy = -float(c) * ir - float(wn - c) * il
                if proxy > best_proxy:
                    best_proxy, best = proxy, col
            features[:n_known] = constant[:n_known]
            constant[n_known:n_known + n_found] = features[n_known:n_known + n_found]
            n_known = n_total
            if best < 0:
                is_leaf = True
            else:
                c, c1 = int(wr[best]), int(wr1[best])
                imp_r = impurity(c - c1, c1, c, criterion)
                imp_l = impurity((wn - w1) - (c - c1), w1 - c1, wn - c, criterion)
                improvement = (float(wn) / float(w_total)) * (node_imp - (float(c) / float(wn) * imp_r) - (float(wn - c) / float(wn) * imp_l))
                if improvement + EPS < 0.0:
                    is_leaf = True
                else:
                    feat = best
        nid = len(feature)
        deepest = max(deepest, depth)
        feature.append(feat)
        left.append(-1 if is_leaf else nid + 1)
        right.append(-1)
        nns.append(n)
        counts.append((wn - w1, w1))
        imp.append(node_imp)
        if parent >= 0 and not is_left:
            right[parent] = nid
        if is_leaf:
            leaf[route] = nid
            frac0[route] = float(wn - w1) / float(wn)
            frac1[route] = float(w1) / float(wn)
        else:
            stack.append((route & Xb[:, feat], nid, False, depth + 1, imp_r, n_known))
            stack.append((route & ~Xb[:, feat], nid, True, depth + 1, imp_l, n_known))
    return dict(node_count=len(feature), max_depth=deepest, feature=np.array(feature, dtype=np.int64),
                left=np.array(left, dtype=np.int64), right=np.array(right, dtype=np.int64),
                n_node_samples=np.array(nns, dtype=np.int64), counts=np.array(counts, dtype=np.int64).reshape(-1, 2),
                impurity=np.array(imp, dtype=np.float64), leaf=leaf, frac0=frac0, frac1=frac1)


def tree_seeds(seed, n_trees):
    rs = np.random.RandomState(seed)
    return [int(rs.randint(INT32_MAX)) for _ in range(n_trees)]


def tree_draws(tree_seed, rows, n_all, bootstrap):
    """(weight[n_all], generator state) of one tree trained on the sample rows `rows` (ascending indices into the n_all
    samples of the design)."""
    rows = np.asarray(rows)
    state = int(np.random.RandomState(tree_seed).randint(0, RAND_R_MAX))
    w = np.zeros(n_all, dtype=np.int64)
    if bootstrap:
        idx = np.random.RandomState(tree_seed).randint(0, len(rows), len(rows), dtype=np.int32)
        w[rows] = np.bincount(idx, minlength=len(rows))
    else:
        w[rows] = 1
    return w, state


def fit_forest(X, y, seed, rows=None, n_estimators=100, criterion="gini", max_depth=None, max_features="sqrt",
               min_samples_leaf=1, min_samples_split=2, bootstrap=True):
    """RandomForestClassifier(random_state=seed, ...).fit(X[rows], y[rows]): the trees, and predict_proba of ALL rows of X
    as the two f64 sums in tree order divided by the number of trees."""
    X = np.asarray(X)
    n_all, p = X.shape
    rows = np.arange(n_all) if rows is None else np.asarray(rows)
    trees = []
    s0, s1 = np.zeros(n_all), np.zeros(n_all)
    for ts in tree_seeds(seed, n_estimators):
        w, state = tree_draws(ts, rows, n_all, bootstrap)
        t = fit_tree(X, y, w, state, criterion, max_depth, n_max_features(max_features, p), min_samples_leaf, min_samples_split)
        trees.append(t)
        s0 += t["frac0"]
        s1 += t["frac1"]
    return dict(trees=trees, sum0=s0, sum1=s1, proba=np.column_stack([s0 / n_estimators, s1 / n_estimators]))


def tree_importances(t, p):
    """Tree.compute_feature_importances(normalize=True) with weighted node sizes."""
    out = np.zeros(p)
    w, imp = t["counts"].sum(axis=1).astype(np.float64), t["impurity"]
    for k in range(t["node_count"]):
        if t["left"][k] != -1:
            l, r = t["left"][k], t["right"][k]
            out[t["feature"][k]] += w[k] * imp[k] - w[l] * imp[l] - w[r] * imp[r]
    out /= w[0]
    s = np.sum(out)
    if s > 0.0:
        out /= s
    return out


def forest_importances(trees, p):
    """RandomForestClassifier.feature_importances_: the mean over trees with more than one node, renormalised."""
    rows = [tree_importances(t, p) for t in trees if t["node_count"] > 1]
    if not rows:
        return np.zeros(p)
    m = np.mean(rows, axis=0, dtype=np.float64)
    return m / np.sum(m)


def grid_point(grid, i):
    """ParameterGrid(grid)[i]: keys sorted, the last key fastest."""
    keys = sorted(grid)
    out = {}
    for k in reversed(keys):
        i, r = divmod(i, len(grid[k]))
        out[k] = grid[k][r]
    return {k: out[k] for k in keys}


def grid_size(grid):
    return int(np.prod([len(v) for v in grid.values()]))


def sampled_indices(grid, n_iter, seed):
    """The grid indices ParameterSampler(grid, n_iter, random_state=seed) visits, for n_iter / grid_size < 0.01:
    sample_without_replacement's tracking selection."""
    size = grid_size(grid)
    n_iter = min(n_iter, size)
    assert n_iter / size < 0.01
    rs = np.random.RandomState(seed)
    taken, out = set(), []
    for _ in range(n_iter):
        j = int(rs.randint(size))
        while j in taken:
            j = int(rs.randint(size))
        taken.add(j)
        out.append(j)
    return out


class Engine:
    """Stands in for PskContext.forest_fit in CPU tests: the same arguments and results, computed by fit_tree()."""

    def forest_fit(self, X, y01, tree_weight, tree_state, tree_fit, fit_criterion, fit_max_depth, fit_max_features,
                   fit_min_samples_leaf, fit_min_samples_split, export=None):
        X = np.asarray(X)
        if not np.all((X == 0) | (X == 1)):
            raise ValueError("the design must be 0/1")
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
    """tests/golden/forest_kat.npz: designs[d] = {X, y, n, p, kind}; cases[k] = {design, seed, params, trees (scikit-learn's,
    in fit_tree()'s layout without leaf / frac), proba, importances}; search: the recorded RandomizedSearchCV; draws: the
    first 25 grid indices of the reference's grid for seeds 0-4."""

    def __init__(self, path=None):
        path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forest_kat.npz")
        z = self.z = np.load(path, allow_pickle=False)
        self.sklearn_version = str(z["sklearn_version"])
        self.designs = []
        for d in range(int(z["n_designs"])):
            n, p = (int(v) for v in z["shape%d" % d])
            X = np.unpackbits(z["X%d" % d], axis=1)[:, :p].astype(np.float64)
            self.designs.append(dict(X=X, y=z["y%d" % d].astype(np.int64), n=n, p=p, kind=str(z["kind"][d])))
        nptr, tptr, sptr, pptr = z["node_ptr"], z["tree_ptr"], z["sample_ptr"], z["feat_ptr"]
        self.cases = []
        for k in range(len(z["case_design"])):
            trees = []
            for t in range(int(tptr[k]), int(tptr[k + 1])):
                a, b = int(nptr[t]), int(nptr[t + 1])
                trees.append(dict(node_count=b - a, max_depth=int(z["tree_max_depth"][t]), feature=z["node_feature"][a:b].astype(np.int64),
                                  left=z["node_left"][a:b].astype(np.int64), right=z["node_right"][a:b].astype(np.int64),
                                  n_node_samples=z["node_n"][a:b].astype(np.int64), counts=z["node_counts"][a:b].astype(np.int64),
                                  impurity=z["node_impurity"][a:b]))
            self.cases.append(dict(design=int(z["case_design"][k]), seed=int(z["case_seed"][k]), params=_params(z["case_params"][k]),
                                   trees=trees, proba=z["proba"][int(sptr[k]):int(sptr[k + 1])].reshape(-1, 2),
                                   importances=z["importances"][int(pptr[k]):int(pptr[k + 1])]))
        g = [_params(r) for r in z["rs_params"]]
        self.search = dict(design=int(z["rs_design"]), cv=int(z["rs_cv"]), seed=int(z["rs_seed"]), n_iter=int(z["rs_n_iter"]),
                           grid=_grid(z), params=g, splits=z["rs_splits"], mean=z["rs_mean"], std=z["rs_std"], rank=z["rs_rank"],
                           best=_params(z["rs_best"]), proba=z["rs_proba"], importances=z["rs_importances"])
        self.draws = {int(s): [int(v) for v in row] for s, row in zip(z["draw_seeds"], z["draw_indices"])}


# case_params / rs_params rows: bootstrap, criterion, max_depth (0 = None), max_features (index into MAX_FEATURES),
# min_samples_leaf, min_samples_split, n_estimators
def _params(r):
    return dict(bootstrap=bool(r[0]), criterion=CRITERIA[int(r[1])], max_depth=int(r[2]) or None, max_features=MAX_FEATURES[int(r[3])],
                min_samples_leaf=int(r[4]), min_samples_split=int(r[5]), n_estimators=int(r[6]))


def encode_params(q):
    return [int(q["bootstrap"]), CRITERIA.index(q["criterion"]), q["max_depth"] or 0, MAX_FEATURES.index(q["max_features"]),
            q["min_samples_leaf"], q["min_samples_split"], q["n_estimators"]]


def _grid(z):
    g = {"bootstrap": [bool(v) for v in z["rs_grid_bootstrap"]], "criterion": [CRITERIA[int(v)] for v in z["rs_grid_criterion"]],
         "max_depth": [int(v) or None for v in z["rs_grid_max_depth"]], "max_features": [MAX_FEATURES[int(v)] for v in z["rs_grid_max_features"]],
         "min_samples_leaf": [int(v) for v in z["rs_grid_min_samples_leaf"]], "min_samples_split": [int(v) for v in z["rs_grid_min_samples_split"]],
         "n_estimators": [int(v) for v in z["rs_grid_n_estimators"]]}
    return g

