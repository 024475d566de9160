"""scikit-learn's depth-first best-split tree builder for a 0/1 design and two classes, restated in plain NumPy / Python
floats: the CPU yardstick of psk_tree_fit (csrc/solver_tree.hip) and the reader of tests/golden/tree_kat.npz
(tools/gen_tree_golden.py).  Defaults of DecisionTreeClassifier: min_samples_split 2, min_samples_leaf 1,
min_impurity_decrease 0, every feature, unit weights.  The one rule scikit-learn leaves to chance is fixed: among columns
whose proxy improvement is bit-equal, the LOWEST column index is taken.

Arithmetic: Python floats are IEEE doubles without fused multiply-adds, and math.log is the C library's log that
scikit-learn's Cython calls, so the proxies are scikit-learn's own to the bit (sklearn/tree/_criterion.pyx:
children_impurity, proxy_impurity_improvement, impurity_improvement; _tree.pyx: DepthFirstTreeBuilder.build)."""
import math
import os

import numpy as np

EPS = float(np.finfo(np.float64).eps)
CRITERIA = ("gini", "entropy")


def impurity(c0, c1, n, criterion):
    """node_impurity / children_impurity of Gini and Entropy for class counts (c0, c1) of n samples."""
    c0, c1, n = float(c0), float(c1), float(n)
    if criterion == "gini":
        sq = 0.0
        sq += c0 * c0
        sq += c1 * c1
        return 1.0 - sq / (n * n)
    e = 0.0
    for c in (c0, c1):
        if c > 0.0:
            c /= n
            e -= c * (math.log(c) / math.log(2.0))   # sklearn/tree/_utils.pyx: log(x) = ln(x) / ln(2.0)
    return e


def proxy(n, n1, c, c1, criterion):
    """Criterion.proxy_impurity_improvement of the split that sends c samples (c1 of class 1) right out of n (n1)."""
    wr, wl = float(c), float(n - c)
    ir = impurity(c - c1, c1, c, criterion)
    il = impurity((n - n1) - (c - c1), n1 - c1, n - c, criterion)
    return -wr * ir - wl * il


def node_proxies(Xb, y, members, criterion):
    """The proxy of every column for the node holding the training samples `members` (bool[n]); -inf for a column that is
    constant in the node.  Xb: bool[n][p]."""
    n, n1 = int(members.sum()), int((members & (y != 0)).sum())
    c = Xb[members].sum(axis=0).astype(np.int64)
    c1 = Xb[members & (y != 0)].sum(axis=0).astype(np.int64)
    out = np.full(Xb.shape[1], -np.inf)
    live = (c > 0) & (c < n)
    cache = {}
    for j in np.nonzero(live)[0]:
        key = (int(c[j]), int(c1[j]))
        v = cache.get(key)
        if v is None:
            v = cache[key] = proxy(n, n1, key[0], key[1], criterion)
        out[j] = v
    return out, c, c1, n, n1


def fit(X, y, train, max_depth, criterion):
    """One tree on the samples train[n] (bool) of the 0/1 design X[n][p].  Returns what PskContext.tree_fit returns for a
    fit: node arrays in pre-order, and for every sample -- held-out ones included -- its leaf and the leaf's class-1
    fraction."""
    Xb = np.asarray(X) != 0
    y = np.asarray(y)
    train = np.asarray(train, dtype=bool)
    n_all = Xb.shape[0]
    n_tot = int(train.sum())
    feature, left, right, nns, counts, imp = [], [], [], [], [], []
    leaf, frac = np.full(n_all, -1, dtype=np.int64), np.zeros(n_all)
    n1_tot = int((train & (y != 0)).sum())
    # (routing mask over every sample, parent, is_left, depth, impurity): scikit-learn pushes right, then left
    stack = [(np.ones(n_all, dtype=bool), -1, False, 0, impurity(n_tot - n1_tot, n1_tot, n_tot, criterion))]
    deepest = 0
    while stack:
        route, parent, is_left, depth, node_imp = stack.pop()
        members = route & train
        n, n1 = int(members.sum()), int((members & (y != 0)).sum())
        is_leaf = depth >= max_depth or n < 2 or node_imp <= EPS
        feat = -2
        if not is_leaf:
            pr, c, c1, _, _ = node_proxies(Xb, y, members, criterion)
            j = int(np.argmax(pr))                       # np.argmax: the first -- lowest -- index among equal maxima
            if pr[j] == -np.inf:
                is_leaf = True
            else:
                cr, cr1 = int(c[j]), int(c1[j])
                imp_r = impurity(cr - cr1, cr1, cr, criterion)
                imp_l = impurity((n - n1) - (cr - cr1), n1 - cr1, n - cr, criterion)
                improvement = (float(n) / float(n_tot)) * (node_imp - (float(cr) / float(n) * imp_r) - (float(n - cr) / float(n) * imp_l))
                if improvement + EPS < 0.0:
                    is_leaf = True
                else:
                    feat = j
        nid = len(feature)
        deepest = max(deepest, depth)
        feature.append(feat)
        left.append(-1 if is_leaf else nid + 1)
        right.append(-1)
        nns.append(n)
        counts.append((n - n1, n1))
        imp.append(node_imp)
        if parent >= 0 and not is_left:
            right[parent] = nid
        if is_leaf:
            leaf[route] = nid
            frac[route] = float(n1) / float(n)
        else:
            stack.append((route & Xb[:, feat], nid, False, depth + 1, imp_r))
            stack.append((route & ~Xb[:, feat], nid, True, depth + 1, imp_l))
    return dict(node_count=len(feature), max_depth=deepest, feature=np.array(feature, dtype=np.int64),
                left=np.array(left, dtype=np.int64), right=np.array(right, dtype=np.int64),
                n_node_samples=np.array(nns, dtype=np.int64), counts=np.array(counts, dtype=np.int64).reshape(-1, 2),
                impurity=np.array(imp, dtype=np.float64), leaf=leaf, frac=frac)


def values(t):
    """tree_.value of scikit-learn >= 1.3: class fractions, [node_count][1][2]."""
    return (t["counts"] / t["n_node_samples"][:, None].astype(np.float64)).reshape(-1, 1, 2)


def importances(t, p):
    """Tree.compute_feature_importances(normalize=True)."""
    out = np.zeros(p)
    w, imp = t["n_node_samples"].astype(np.float64), t["impurity"]
    for k in range(t["node_count"]):
        if t["left"][k] != -1:
            l, r = t["left"][k], t["right"][k]
            out[t["feature"][k]] += w[k] * imp[k] - w[l] * imp[l] - w[r] * imp[r]
    out /= w[0]
    s = np.sum(out)
    if s > 0.0:
        out /= s
    return out


def apply(t, X):
    """The leaf of every row of X, walking the node arrays."""
    Xb = np.asarray(X) != 0
    node = np.zeros(Xb.shape[0], dtype=np.int64)
    for _ in range(t["max_depth"]):
        f = t["feature"][node]
        inner = f >= 0
        go_right = Xb[np.arange(Xb.shape[0]), np.where(inner, f, 0)]
        node = np.where(inner, np.where(go_right, t["right"][node], t["left"][node]), node)
    return node


class Engine:
    """Stands in for PskContext.tree_fit in CPU tests: the same arguments and results, computed by fit()."""

    def tree_fit(self, X, y01, fold, fit_max_depth, fit_criterion, fit_fold):
        X = np.asarray(X)
        if not np.all((X == 0) | (X == 1)):
            raise ValueError("the design must be 0/1")
        fold = np.asarray(fold)
        return [fit(X, y01, fold != ff, int(d), c if isinstance(c, str) else CRITERIA[int(c)])
                for d, c, ff in zip(fit_max_depth, fit_criterion, fit_fold)]


class Fixture:
    """tests/golden/tree_kat.npz: designs[d] = {X, y, folds, n, p, kind}; cases[k] = {design, criterion, depth, invariant,
    tree (scikit-learn's, random_state 0, in fit()'s layout without leaf / frac), value, proba, importances}; gs: the recorded
    GridSearchCV run."""

    def __init__(self, path=None):
        path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_kat.npz")
        z = self.z = np.load(path, allow_pickle=False)
        self.designs = []
        for d in range(int(z["n_designs"])):
            n, p = (int(v) for v in z["shape%d" % d])
            X = np.unpackbits(z["X%d" % d], axis=1)[:, :p].astype(np.float64)
            self.designs.append(dict(X=X, y=z["y%d" % d].astype(np.int64), folds=z["folds%d" % d].astype(np.int64), n=n, p=p,
                                     kind=str(z["kind"][d])))
        self.cases = []
        nptr, sptr, pptr = z["node_ptr"], z["sample_ptr"], z["feat_ptr"]
        for k in range(len(z["case_design"])):
            a, b = int(nptr[k]), int(nptr[k + 1])
            cnt = np.rint(z["node_value"][a:b] * z["node_n"][a:b, None]).astype(np.int64)
            tree = dict(node_count=b - a, max_depth=int(z["case_max_depth"][k]), feature=z["node_feature"][a:b].astype(np.int64),
                        left=z["node_left"][a:b].astype(np.int64), right=z["node_right"][a:b].astype(np.int64),
                        n_node_samples=z["node_n"][a:b].astype(np.int64), counts=cnt, impurity=z["node_impurity"][a:b])
            self.cases.append(dict(design=int(z["case_design"][k]), criterion=CRITERIA[int(z["case_criterion"][k])],
                                   depth=int(z["case_depth"][k]), invariant=bool(z["case_invariant"][k]), tree=tree,
                                   value=z["node_value"][a:b].reshape(-1, 1, 2),
                                   proba=z["proba"][int(sptr[k]):int(sptr[k + 1])].reshape(-1, 2),
                                   importances=z["importances"][int(pptr[k]):int(pptr[k + 1])]))
        self.gs = dict(design=int(z["gs_design"]), cv=int(z["gs_cv"]), depths=[int(v) for v in z["gs_depths"]],
                       params=[{"criterion": CRITERIA[int(c)], "max_depth": int(d)} for c, d in z["gs_params"]],
                       splits=z["gs_splits"], mean=z["gs_mean"], std=z["gs_std"], rank=z["gs_rank"],
                       best={"criterion": CRITERIA[int(z["gs_best"][0])], "max_depth": int(z["gs_best"][1])})
