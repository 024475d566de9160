"""The count-design half of the gradient-boosting contract of include/psk.h (f16) in NumPy: what psk_gb_fit_counts and
psk_gb_decision_counts compute, bit for bit.  Everything that is not about the design is gb_restated.py's (gb_expit, two_level_sum,
the leaf rules, the Newton leaf values); this module restates

  * the threshold planes: per column the distinct values g_0 < g_1 < ... over ALL samples, plane k with bit s = (x_s >= g_(k+1)),
    planes ordered by (column, k), none for a constant column
  * a candidate's sum: two_level_sum of the residuals under the plane's bits within the node's in-bag set, each plane on its own
  * the winner: np.argmax over the planes in index order (the first of equal maxima: the lowest column, then the lowest threshold)
  * the threshold: lo / 2.0 + hi / 2.0 of the largest in-bag value below the winning plane's g and the smallest at or above it
  * routing: x <= threshold goes left, for EVERY sample, held-out ones included
  * the decisive-input diagnostic of tools/gen_gb_count_golden.py: per split the relative margin of the winning proxy over the
    best plane with a DIFFERENT partition of the node's in-bag samples (equal and complementary partitions are one partition), and
    the smallest impurity of a node whose targets differ
  * Engine: gb_restated.Engine with gb_fit_counts / gb_decision_counts, for host tests of model.GradientBoosting(counts=True)
"""
import numpy as np

import gb_restated as R

COUNT_MAX = 2.0 ** 24


def count_design(X, who):
    """engine.PskContext._count_design: the values as float64, ValueError unless every one is an integer in 0 .. 2^24."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or not np.all((X >= 0) & (X <= COUNT_MAX) & (X == np.floor(X))):
        raise ValueError("%s takes a count design: every value must be an integer in 0 .. 2^24" % who)
    return X


def planes(X):
    """X[n][p] -> (bits[n][P] booleans, plane_col[P], plane_val[P]), in the order of csrc/solver_tree_common.h."""
    X = np.asarray(X, dtype=np.float64)
    cols, vals = [], []
    for j in range(X.shape[1]):
        g = np.unique(X[:, j])
        cols += [j] * (len(g) - 1)
        vals += list(g[1:])
    plane_col, plane_val = np.array(cols, dtype=np.int64), np.array(vals, dtype=np.float64)
    return X[:, plane_col] >= plane_val[None, :], plane_col, plane_val


def fit_one(X, y, in_bag, loss, n_estimators, learning_rate, max_depth, init_raw, diagnose=False):
    """One fit.  X[n][p] counts, y[n], in_bag[n] booleans.  Returns gb_restated.fit_one's dictionary (nodes[..][0] the design
    column) plus threshold[n_estimators][cap]: -2.0 at a leaf and behind node_count."""
    X = count_design(X, "gb_count_restated.fit_one")
    n, p = X.shape
    W = -(-n // 64)
    N = W * 64
    B, plane_col, plane_val = planes(X)
    P = len(plane_col)
    Bp = np.zeros((N, P), dtype=bool)
    Bp[:n] = B
    Xp = np.zeros((N, p))
    Xp[:n] = X
    yp = np.zeros(N)
    yp[:n] = np.asarray(y, dtype=np.float64)
    T = np.zeros(N, dtype=bool)
    T[:n] = np.asarray(in_bag, dtype=bool)
    live = np.zeros(N, dtype=bool)
    live[:n] = True
    cap = R.node_cap(max_depth)
    F = np.zeros(N)
    F[:n] = float(init_raw)
    out = dict(node_count=np.zeros(n_estimators, dtype=np.int32), nodes=np.zeros((n_estimators, cap, 4), dtype=np.int32),
               value=np.zeros((n_estimators, cap)), impurity=np.zeros((n_estimators, cap)), staged=np.zeros((n_estimators, n)),
               threshold=np.full((n_estimators, cap), -2.0))
    diag = dict(margin=np.inf, min_impurity=np.inf)
    lr = float(learning_rate)
    for stage in range(n_estimators):
        r = yp - F if loss == 0 else yp - R.gb_expit(F)
        nodes, value, impurity, threshold = out["nodes"][stage], out["value"][stage], out["impurity"][stage], out["threshold"][stage]
        stack, next_id = [(-1, 0, False, live)], 0
        while stack:
            parent, d, is_left, m = stack.pop()
            S = m & T
            w = int(S.sum())
            total = R.two_level_sum(np.where(S, r, 0.0))
            sq = R.two_level_sum(np.where(S, r * r, 0.0))
            nw = float(w)
            mean = total / nw
            imp = sq / nw - mean * mean
            all_equal = np.unique(r[S].view(np.uint64)).size == 1
            is_leaf = d >= max_depth or w < 2 or imp <= R.DBL_EPSILON or all_equal
            if diagnose and d < max_depth and w >= 2 and not all_equal:
                diag["min_impurity"] = min(diag["min_impurity"], float(imp))
            feat, thr = -2, -2.0
            if not is_leaf and P:
                sel = Bp & S[:, None]
                c = sel.sum(axis=0)
                sr = R.two_level_sum(np.where(sel, r[:, None], 0.0).T)       # each plane's sum on its own
                ok = (c > 0) & (c < w)
                wr, wl = c.astype(np.float64), (w - c).astype(np.float64)
                sl = total - sr
                diff = wr * sl - wl * sr
                with np.errstate(divide="ignore", invalid="ignore"):
                    proxy = np.where(ok, diff * diff / (wl * wr), -np.inf)
                if ok.any():
                    q = int(np.argmax(proxy))             # the first of equal maxima: the lowest column, then the lowest threshold
                    feat = int(plane_col[q])
                    x = Xp[S, feat]
                    lo, hi = x[x < plane_val[q]].max(), x[x >= plane_val[q]].min()
                    thr = lo / 2.0 + hi / 2.0
                    if diagnose:
                        win = sel[:, q]
                        other = ok & ~((sel == win[:, None]).all(axis=0) | (sel == (S & ~win)[:, None]).all(axis=0))
                        if other.any():
                            p1, p2 = proxy[q], proxy[other].max()
                            diag["margin"] = min(diag["margin"], float((p1 - p2) / p1) if p1 > 0.0 else 0.0)
            is_leaf = feat < 0
            node_id = next_id
            next_id += 1
            val = mean
            if loss == 1 and is_leaf:
                prob = yp - r
                num, den = total / nw, R.two_level_sum(np.where(S, prob * (1.0 - prob), 0.0)) / nw
                val = 0.0 if abs(den) < 1e-150 else num / den
            nodes[node_id] = (feat, -1 if is_leaf else node_id + 1, -1, w)
            value[node_id], impurity[node_id], threshold[node_id] = val, imp, thr
            if parent >= 0 and not is_left:
                nodes[parent, 2] = node_id
            if is_leaf:
                step = lr * val
                F = np.where(m, F + step, F)
            else:
                right = Xp[:, feat] > thr                 # every sample by the threshold, not by the plane that won
                stack.append((node_id, d + 1, False, m & right))
                stack.append((node_id, d + 1, True, m & ~right))
        out["node_count"][stage] = next_id
        out["staged"][stage] = F[:n]
    out["raw"] = F[:n].copy()
    if diagnose:
        out.update(diag)
    return out


def fit(X, y, fold, fit_fold, loss, n_estimators, learning_rate, max_depth, init_raw, diagnose=False):
    fold = np.asarray(fold)
    return [fit_one(X, y, fold != ff, loss, n_estimators, learning_rate, max_depth, init_raw[j], diagnose) for j, ff in enumerate(fit_fold)]


def decision(X, node_count, nodes, value, threshold, init_raw, learning_rate, max_depth):
    """psk_gb_decision_counts: init_raw, then + learning_rate * value[leaf] in stage order; x <= threshold goes left."""
    X = count_design(X, "gb_count_restated.decision")
    n = X.shape[0]
    rows = np.arange(n)
    F = np.full(n, float(init_raw))
    for t in range(len(node_count)):
        node = np.zeros(n, dtype=np.int64)
        for _ in range(max_depth):
            f = nodes[t, node, 0]
            inner = f >= 0
            left = X[rows, np.where(inner, f, 0)] <= threshold[t, node]
            node = np.where(inner, np.where(left, nodes[t, node, 1], nodes[t, node, 2]), node)
        F = F + float(learning_rate) * value[t, node]
    return F


class Engine(R.Engine):
    """engine.PskContext's gb_fit / gb_decision and gb_fit_counts / gb_decision_counts served by the two restatements."""

    def gb_fit_counts(self, X, y, fold, fit_fold, loss, n_estimators, learning_rate, max_depth, init_raw, staged=True):
        fits = fit(count_design(X, "gb_fit_counts"), y, fold, fit_fold, {"squared_error": 0, "log_loss": 1}.get(loss, loss), n_estimators,
                   learning_rate, max_depth, np.asarray(init_raw, dtype=np.float64).reshape(-1))
        if not staged:
            for f in fits:
                f["staged"] = None
        return fits

    def gb_decision_counts(self, X, node_count, nodes, value, threshold, init_raw, learning_rate, max_depth):
        return decision(count_design(X, "gb_decision_counts"), np.asarray(node_count), np.asarray(nodes), np.asarray(value),
                        np.asarray(threshold), init_raw, learning_rate, max_depth)
