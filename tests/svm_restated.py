"""libsvm's C-SVC solver (Solver::Solve, WSS2 working sets, no shrinking) restated in NumPy, f64: the CPU yardstick of
the SVM tests.  Step for step what scikit-learn's SVC(shrinking=False) runs, so that a fit stopped at max_iter is the
same iterate:
  * solver index order: the training samples of class 0, then those of class 1, input order kept within a class;
  * i = the LAST index with the largest -y_t G_t over I_up; j = the LAST index with the smallest
    -(Gmax + y_j G_j)^2 / max(QD_i + QD_j - 2 y_i y_j Q_ij, 1e-12) over I_low with a positive numerator;
  * Q entries rounded to float (libsvm's Qfloat), everything else double;
  * rho = mean of y_i G_i over the free variables, else the midpoint of the bounds.
Signs are libsvm's: class 0 is +1, the decision value is sum_j dual_j K(x_j, x) - rho (scikit-learn's decision_function
is its negative, dual_coef_ the negative of the duals at the support vectors, intercept_ = rho)."""
import numpy as np

TAU = 1e-12


def kernel_matrix(X, kernel, gamma=0.0):
    """K[i][j] in f64 as libsvm evaluates it: x_i . x_j, or exp(-gamma (|x_i|^2 + |x_j|^2 - 2 x_i . x_j))."""
    X = np.asarray(X, dtype=np.float64)
    D = X @ X.T
    if kernel == "linear":
        return D
    sq = np.diag(D)
    return np.exp(-gamma * (sq[:, None] + sq[None, :] - 2 * D))


def smo(K, y01, C, eps, max_iter):
    """K over the training samples in SOLVER order (class 0 first).  Returns (alpha, y, G, rho, iterations)."""
    n = len(y01)
    y = np.where(np.asarray(y01) == 0, 1.0, -1.0)
    Q = (np.outer(y, y) * K).astype(np.float32).astype(np.float64)
    QD = np.diag(K).astype(np.float64).copy()
    a = np.zeros(n)
    G = -np.ones(n)
    it = 0
    while True:
        if max_iter != -1 and it >= max_iter:
            break
        up = ((y > 0) & (a < C)) | ((y < 0) & (a > 0))
        low = ((y > 0) & (a > 0)) | ((y < 0) & (a < C))
        v = np.where(up, -y * G, -np.inf)
        Gmax = v.max()
        i = n - 1 - int(np.argmax(v[::-1]))                 # '>=' keeps the LAST maximal index
        Gmax2 = np.where(low, y * G, -np.inf).max()
        gd = Gmax + y * G
        qc = QD[i] + QD - 2.0 * y[i] * y * Q[i]
        qc = np.where(qc > 0, qc, TAU)
        od = np.where(low & (gd > 0), -(gd * gd) / qc, np.inf)
        if Gmax + Gmax2 < eps or not np.isfinite(od.min()):
            break
        j = n - 1 - int(np.argmin(od[::-1]))                # '<=' keeps the LAST minimal index
        it += 1
        oi, oj = a[i], a[j]
        if y[i] != y[j]:
            q = QD[i] + QD[j] + 2 * Q[i, j]
            q = q if q > 0 else TAU
            d = (-G[i] - G[j]) / q
            diff = a[i] - a[j]
            a[i] += d
            a[j] += d
            if diff > 0:
                if a[j] < 0:
                    a[j] = 0
                    a[i] = diff
            else:
                if a[i] < 0:
                    a[i] = 0
                    a[j] = -diff
            if diff > 0:
                if a[i] > C:
                    a[i] = C
                    a[j] = C - diff
            else:
                if a[j] > C:
                    a[j] = C
                    a[i] = C + diff
        else:
            q = QD[i] + QD[j] - 2 * Q[i, j]
            q = q if q > 0 else TAU
            d = (G[i] - G[j]) / q
            s = a[i] + a[j]
            a[i] -= d
            a[j] += d
            if s > C:
                if a[i] > C:
                    a[i] = C
                    a[j] = s - C
            else:
                if a[j] < 0:
                    a[j] = 0
                    a[i] = s
            if s > C:
                if a[j] > C:
                    a[j] = C
                    a[i] = s - C
            else:
                if a[i] < 0:
                    a[i] = 0
                    a[j] = s
        G += Q[i] * (a[i] - oi) + Q[j] * (a[j] - oj)
    yG = y * G
    ub = ((a >= C) & (y < 0)) | ((a <= 0) & (y > 0))
    lb = ((a >= C) & (y > 0)) | ((a <= 0) & (y < 0))
    free = (a > 0) & (a < C)
    if free.any():
        rho = yG[free].sum() / free.sum()
    else:
        rho = (yG[ub].min() + yG[lb].max()) / 2
    return a, y, G, rho, it


def fit(X, y01, train, C, kernel="linear", gamma=0.0, tol=1e-3, max_iter=-1):
    """One fit on the samples train[] (bool mask) of X.  Returns (dual[n] = y_i alpha_i, 0 off the training set; rho;
    dec[n] for every sample; iterations)."""
    y01 = np.asarray(y01)
    train = np.asarray(train, dtype=bool)
    order = np.concatenate([np.nonzero(train & (y01 == 0))[0], np.nonzero(train & (y01 != 0))[0]])
    K = kernel_matrix(X, kernel, gamma)
    a, y, _, rho, it = smo(K[np.ix_(order, order)], y01[order], C, tol, max_iter)
    dual = np.zeros(len(y01))
    dual[order] = a * y
    sv = order[a != 0]
    dec = K[:, sv] @ dual[sv] - rho
    return dual, rho, dec, it


def optimality(K, y01, dual, C):
    """(Gmax + Gmax2, |y'a|) of a solution, recomputed from the exact kernel matrix in f64: libsvm's stopping quantity."""
    y = np.where(np.asarray(y01) == 0, 1.0, -1.0)
    a = np.abs(dual)
    G = (np.outer(y, y) * K) @ a - 1.0
    up = ((y > 0) & (a < C)) | ((y < 0) & (a > 0))
    low = ((y > 0) & (a > 0)) | ((y < 0) & (a < C))
    gmax = np.where(up, -y * G, -np.inf).max()
    gmax2 = np.where(low, y * G, -np.inf).max()
    return gmax + gmax2, abs(float(dual.sum()))


class Fixture:
    """tests/golden/svm_kat.npz (tools/gen_svm_golden.py): designs unpacked, one dict per fit with both records."""

    def __init__(self, path=None):
        import os
        z = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svm_kat.npz"))
        self.z = z
        self.Cs, self.tol, self.max_iter = z["Cs"], float(z["tol"]), int(z["max_iter"])
        self.designs = []
        for d in range(int(z["n_designs"])):
            n, p = (int(v) for v in z["shape%d" % d])
            X = np.unpackbits(z["X%d" % d], axis=1)[:, :p].astype(np.float64)
            self.designs.append({"X": X, "y": z["y%d" % d].astype(np.int64), "folds": z["folds%d" % d].astype(np.int32),
                                 "n": n, "p": p})
        on_of = {int(f): k for k, f in enumerate(z["on_fit"])}
        self.fits = []
        for j in range(len(z["fit_design"])):
            n = self.designs[int(z["fit_design"][j])]["n"]

            def dual(idx, val, ptr, k):
                out = np.zeros(n)
                out[idx[ptr[k]:ptr[k + 1]].astype(np.int64)] = val[ptr[k]:ptr[k + 1]]
                return out
            off = {"iters": int(z["fit_iters_off"][j]), "rho": float(z["fit_rho_off"][j]),
                   "dec": z["dec_off"][z["dec_ptr"][j]:z["dec_ptr"][j + 1]], "dual": dual(z["sv_idx"], z["sv_val"], z["sv_ptr"], j)}
            if j in on_of:
                k = on_of[j]
                on = {"iters": int(z["fit_iters_on"][j]), "rho": float(z["fit_rho_on"][j]),
                      "dec": z["dec_on"][z["on_dec_ptr"][k]:z["on_dec_ptr"][k + 1]],
                      "dual": dual(z["on_sv_idx"], z["on_sv_val"], z["on_sv_ptr"], k)}
            else:
                on = off
            self.fits.append({"design": int(z["fit_design"][j]), "kernel": "rbf" if z["fit_kernel"][j] else "linear",
                              "C": float(z["fit_C"][j]), "gamma": float(z["fit_gamma"][j]), "fold": int(z["fit_fold"][j]),
                              "same": bool(z["fit_same"][j]), "admissible": bool(z["fit_admissible"][j]), "off": off, "on": on})

    def train_mask(self, fit):
        return self.designs[fit["design"]]["folds"] != fit["fold"]


def platt_objective_gradient(dec, labels_pos, A, B):
    """Gradient (dA, dB) of libsvm's regularised Platt likelihood (sigmoid_train; Lin, Lin, Weng 2007) at (A, B):
    targets (N+ + 1)/(N+ + 2) for the positive class and 1/(N- + 2) for the other."""
    dec = np.asarray(dec, dtype=np.float64)
    pos = np.asarray(labels_pos, dtype=bool)
    npos, nneg = pos.sum(), (~pos).sum()
    t = np.where(pos, (npos + 1.0) / (npos + 2.0), 1.0 / (nneg + 2.0))
    fApB = dec * A + B
    p = np.where(fApB >= 0, np.exp(-np.abs(fApB)) / (1.0 + np.exp(-np.abs(fApB))), 1.0 / (1.0 + np.exp(-np.abs(fApB))))
    d1 = t - p
    return float((dec * d1).sum()), float(d1.sum())
