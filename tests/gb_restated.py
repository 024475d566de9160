"""The gradient-boosting contract of include/psk.h (f16) in NumPy: what psk_gb_fit and psk_gb_decision compute, bit for bit.

  * gb_exp mirrors csrc/solver_gb_math.h line for line (IEEE +, -, *, /, rint, ldexp: NumPy evaluates each as the C library and
    the device do)
  * every sum over samples is two-level: np.cumsum along a word of 64 samples (a sequential sum from 0.0; an unset sample adds
    +0.0, which changes nothing: a partial is never -0.0), then np.cumsum over the word partials.  Never np.sum, which adds
    pairwise
  * the leaf rules, the tie rule (np.argmax: the first, hence lowest, column among equal maxima) and the Newton leaf values
  * the decisive-input diagnostic of tools/gen_gb_golden.py: per split the relative margin of the winning proxy over the best
    column with a DIFFERENT partition of the node's in-bag samples, and the smallest impurity of a node whose targets differ
  * Engine: a stand-in for engine.PskContext with gb_fit / gb_decision, for host tests of model.GradientBoosting and `modeling`
"""
import numpy as np

DBL_EPSILON = 2.0 ** -52


def gb_exp(x):
    x = np.asarray(x, dtype=np.float64)
    x = np.where(x > 708.0, 708.0, x)
    x = np.where(x < -708.0, -708.0, x)
    k = np.rint(x * float.fromhex("0x1.71547652b82fep+0"))
    r = (x - k * float.fromhex("0x1.62e42fee00000p-1")) - k * float.fromhex("0x1.a39ef35793c76p-33")
    q = float.fromhex("0x1.6124613a86d09p-33")
    q = q * r + float.fromhex("0x1.1eed8eff8d898p-29")
    q = q * r + float.fromhex("0x1.ae64567f544e4p-26")
    q = q * r + float.fromhex("0x1.27e4fb7789f5cp-22")
    q = q * r + float.fromhex("0x1.71de3a556c734p-19")
    q = q * r + float.fromhex("0x1.a01a01a01a01ap-16")
    q = q * r + float.fromhex("0x1.a01a01a01a01ap-13")
    q = q * r + float.fromhex("0x1.6c16c16c16c17p-10")
    q = q * r + float.fromhex("0x1.1111111111111p-7")
    q = q * r + float.fromhex("0x1.5555555555555p-5")
    q = q * r + float.fromhex("0x1.5555555555555p-3")
    q = q * r + float.fromhex("0x1.0000000000000p-1")
    q = q * r + 1.0
    q = q * r + 1.0
    return np.ldexp(q, k.astype(np.int32))


def gb_expit(x):
    return 1.0 / (1.0 + gb_exp(-np.asarray(x, dtype=np.float64)))


def two_level_sum(v):
    """v[..., W * 64] -> [...]: within a word ascending from 0.0, then the word partials ascending from 0.0."""
    v = np.asarray(v, dtype=np.float64)
    words = np.cumsum(v.reshape(v.shape[:-1] + (-1, 64)), axis=-1)[..., -1]
    return np.cumsum(words, axis=-1)[..., -1]


def node_cap(max_depth):
    return (2 << max_depth) - 1


def fit_one(X, y, in_bag, loss, n_estimators, learning_rate, max_depth, init_raw, diagnose=False):
    """One fit.  X[n][p] 0/1, y[n], in_bag[n] booleans.  Returns a dict in the layout of engine.PskContext.gb_fit: node_count
    [n_estimators], nodes[n_estimators][cap][4], value / impurity[n_estimators][cap], raw[n], staged[n_estimators][n]; with
    `diagnose` also margin (the smallest (P1 - P2) / P1 over the splits) and min_impurity (over the nodes whose in-bag targets
    are not all bit-equal)."""
    X = np.asarray(X) != 0
    n, p = X.shape
    W = -(-n // 64)
    N = W * 64
    Xp = np.zeros((N, p), dtype=bool)
    Xp[:n] = X
    yp = np.zeros(N)
    yp[:n] = np.asarray(y, dtype=np.float64)
    T = np.zeros(N, dtype=bool)
    T[:n] = np.asarray(in_bag, dtype=bool)
    live = np.zeros(N, dtype=bool)
    live[:n] = True
    cap = node_cap(max_depth)
    F = np.zeros(N)
    F[:n] = float(init_raw)
    out = dict(node_count=np.zeros(n_estimators, dtype=np.int32), nodes=np.zeros((n_estimators, cap, 4), dtype=np.int32),
               value=np.zeros((n_estimators, cap)), impurity=np.zeros((n_estimators, cap)), staged=np.zeros((n_estimators, n)))
    diag = dict(margin=np.inf, min_impurity=np.inf)
    lr = float(learning_rate)
    for stage in range(n_estimators):
        r = yp - F if loss == 0 else yp - gb_expit(F)
        nodes, value, impurity = out["nodes"][stage], out["value"][stage], out["impurity"][stage]
        stack, next_id = [(-1, 0, False, live)], 0
        while stack:
            parent, d, is_left, m = stack.pop()
            S = m & T
            w = int(S.sum())
            total = two_level_sum(np.where(S, r, 0.0))
            sq = two_level_sum(np.where(S, r * r, 0.0))
            nw = float(w)
            mean = total / nw
            imp = sq / nw - mean * mean
            all_equal = np.unique(r[S].view(np.uint64)).size == 1
            is_leaf = d >= max_depth or w < 2 or imp <= DBL_EPSILON or all_equal
            if diagnose and d < max_depth and w >= 2 and not all_equal:
                diag["min_impurity"] = min(diag["min_impurity"], float(imp))
            feat = -2
            if not is_leaf:
                cols = Xp & S[:, None]
                c = cols.sum(axis=0)
                sr = two_level_sum(np.where(cols, r[:, None], 0.0).T)
                ok = (c > 0) & (c < w)
                wr, wl = c.astype(np.float64), (w - c).astype(np.float64)
                sl = total - sr
                diff = wr * sl - wl * sr
                with np.errstate(divide="ignore", invalid="ignore"):
                    proxy = np.where(ok, diff * diff / (wl * wr), -np.inf)
                if not ok.any():
                    is_leaf = True
                else:
                    feat = int(np.argmax(proxy))          # the first of equal maxima: the lowest column
                    if diagnose:
                        win = cols[:, feat]
                        other = ok & ~((cols == win[:, None]).all(axis=0) | (cols == (S & ~win)[:, None]).all(axis=0))
                        if other.any():
                            p1, p2 = proxy[feat], proxy[other].max()
                            diag["margin"] = min(diag["margin"], float((p1 - p2) / p1) if p1 > 0.0 else 0.0)
            node_id = next_id
            next_id += 1
            val = mean
            if loss == 1 and is_leaf:
                prob = yp - r
                num, den = total / nw, two_level_sum(np.where(S, prob * (1.0 - prob), 0.0)) / nw
                val = 0.0 if abs(den) < 1e-150 else num / den
            nodes[node_id] = (feat, -1 if is_leaf else node_id + 1, -1, w)
            value[node_id], impurity[node_id] = val, imp
            if parent >= 0 and not is_left:
                nodes[parent, 2] = node_id
            if is_leaf:
                step = lr * val
                F = np.where(m, F + step, F)
            else:
                col = Xp[:, feat]
                stack.append((node_id, d + 1, False, m & col))
                stack.append((node_id, d + 1, True, m & ~col))
        out["node_count"][stage] = next_id
        out["staged"][stage] = F[:n]
    out["raw"] = F[:n].copy()
    if diagnose:
        out.update(diag)
    return out


def fit(X, y, fold, fit_fold, loss, n_estimators, learning_rate, max_depth, init_raw, diagnose=False):
    fold = np.asarray(fold)
    return [fit_one(X, y, fold != ff, loss, n_estimators, learning_rate, max_depth, init_raw[j], diagnose) for j, ff in enumerate(fit_fold)]


def decision(X, node_count, nodes, value, init_raw, learning_rate, max_depth):
    """psk_gb_decision: init_raw, then + learning_rate * value[leaf] in stage order."""
    X = np.asarray(X) != 0
    n = X.shape[0]
    rows = np.arange(n)
    F = np.full(n, float(init_raw))
    for t in range(len(node_count)):
        node = np.zeros(n, dtype=np.int64)
        for _ in range(max_depth):
            f = nodes[t, node, 0]
            inner = f >= 0
            bit = X[rows, np.where(inner, f, 0)]
            node = np.where(inner, np.where(bit, nodes[t, node, 2], nodes[t, node, 1]), node)
        F = F + float(learning_rate) * value[t, node]
    return F


def feature_importances(f, p):
    """BaseGradientBoosting.feature_importances_ from one fit's node arrays: per tree with a split, Tree.
    compute_feature_importances(normalize=False) -- every split's w I - w_l I_l - w_r I_r added to its column in node order,
    divided by the root's weight --, the mean over those trees, divided by its sum."""
    per_tree = []
    for t, k in enumerate(f["node_count"]):
        if k <= 1:
            continue
        nd, I = f["nodes"][t], f["impurity"][t]
        imp = np.zeros(p)
        for i in range(k):
            if nd[i, 1] != -1:
                l, r = nd[i, 1], nd[i, 2]
                imp[nd[i, 0]] += float(nd[i, 3]) * I[i] - float(nd[l, 3]) * I[l] - float(nd[r, 3]) * I[r]
        per_tree.append(imp / float(nd[0, 3]))
    if not per_tree:
        return np.zeros(p)
    avg = np.mean(per_tree, axis=0, dtype=np.float64)
    return avg / np.sum(avg)


def init_raw(y, in_bag, loss):
    """scikit-learn's initial raw prediction (_gb.py::_init_raw_predictions over DummyRegressor(strategy='mean') /
    DummyClassifier(strategy='prior')) of the in-bag samples."""
    yt = np.asarray(y, dtype=np.float64)[np.asarray(in_bag, dtype=bool)]
    if loss == 0:
        return float(np.average(yt))
    eps = np.finfo(np.float32).eps
    q = np.clip(np.bincount(yt.astype(np.int64), minlength=2)[1] / len(yt), eps, 1 - eps, dtype=np.float64)
    return float(np.log(q / (1 - q)))


class Engine:
    """engine.PskContext's gb_fit / gb_decision served by this module."""

    def gb_fit(self, X, y, fold, fit_fold, loss, n_estimators, learning_rate, max_depth, init_raw, staged=True):
        fits = fit(X, y, fold, fit_fold, {"squared_error": 0, "log_loss": 1}.get(loss, loss), n_estimators, learning_rate, max_depth,
                   np.asarray(init_raw, dtype=np.float64).reshape(-1))
        if not staged:
            for f in fits:
                f["staged"] = None
        return fits

    def gb_decision(self, X, node_count, nodes, value, init_raw, learning_rate, max_depth):
        return decision(X, np.asarray(node_count), np.asarray(nodes), np.asarray(value), init_raw, learning_rate, max_depth)
