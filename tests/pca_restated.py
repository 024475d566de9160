"""scikit-learn 1.7.2's StandardScaler() + PCA() restated in plain NumPy along the route psk_pca_fit takes (csrc/pca.hip): column
moments, the standardised design Z, the Gram matrix G = Z Z', numpy.linalg.eigh of it, the leading components S^-1 U' Z, the
sign rule and the rank floor; and psk_pca_transform's product summed in the order include/psk.h (f11) states.  The CPU yardstick
of the two entry points, the reader of tests/golden/pca_kat.npz (tools/gen_pca_golden.py) and a stand-in for the engine in host
tests.

Bounds (derived here, not measured; u = 2^-53; the tests print the share of each that is used):

  tol_var[j] = 2 ((n + 4) u var_j + (n u |mean_j|)^2)                                                  -- var_tolerance()
      A variance is two sums of n terms.  The mean carries a relative error delta <= n u (a sum of n terms and a division);
      the centred values then all shift by eps = mean delta, and sum (d_i - eps)^2 = sum d_i^2 + n eps^2 because the d_i add to
      zero: the shift enters in the second order only.  The sum of n squares, each squared after a rounded subtraction, and
      the division by n add (n + 3) u var.  The factor 2: scikit-learn's side carries an error of the same size.

  tol_lambda = K (n + p) u lambda_1,  K = rho + 16,  rho = || |Z| ||_2^2 / lambda_1 >= 1                 -- lambda_tolerance()
      Weyl: |lambda_i(G + E) - lambda_i(G)| <= ||E||_2.  Three sources of E:
      (a) the scale of a column is known to 2 (n + 2) u relative (tol_var, and the square root halves it: taken whole here);
          that is a column scaling Z (I + D), so E = Z (2 D + D^2) Z' and ||E||_2 <= 4 (n + 2) u lambda_1 for the two sides
          together: the 4 of K;
      (b) an entry of G is a sum of p products: |E_ik| <= p u sum_j |z_ij| |z_kj| (Higham, Accuracy and Stability, 3.1), hence
          ||E||_2 <= p u || |Z| |Z|' ||_2 = p u rho lambda_1.  Only this side forms G (scikit-learn decomposes Z itself):
          the rho of K;
      (c) the eigen-decomposition on either side (LAPACK there, Jacobi here) is backward stable, ||E||_2 <= q(n) u lambda_1
          with q a modest linear function of n (Golub and Van Loan, Matrix Computations, 8.4 and 8.5); q(n) = 6 n is taken
          for each of the two: the 12 of K.
      (n + 2) and p are both below n + p.  rho is a property of the design (computed from the restatement's Z); it is 4.5 to 7.7
      for the fixture's designs (K = 20.5 to 23.7).  The same bound serves the eigen-residual ||Z'(Z v_i) - lambda_i v_i||_2: v_i = Z' u_i / s_i,
      so the residual is Z' r_i / s_i with r_i = G u_i - lambda_i u_i, ||r_i||_2 <= ||E||_2.

  tol_v[i] = 2 * 2 tol_lambda / gap_i,  gap_i = the distance from lambda_i to the nearest other eigenvalue   -- vector_tolerance()
      Davis-Kahan (sin theta <= ||E||_2 / gap for a simple eigenvalue, in the form with the gap of the unperturbed matrix and
      ||E||_2 <= gap / 2: the first 2); the inner 2 because both sides carry an error.  ||v - v'||_2 <= sqrt(2) sin theta
      <= 2 sin theta is absorbed by taking ||E||_2 = tol_lambda, which already counts both sides.

  transform: |sum_j z_ij v_cj in one order - in another| <= 2 (p + 4) u sum_j |z_ij| |v_cj|         -- transform_tolerance()
      two summations of the same p products, each product of a z with 3 roundings (subtraction, division, product).
  a score of the fit is s_c u_ic, not a sum over the columns: Z v_c = G u_c / s_c = s_c u_c + r_c / s_c, so it agrees with
      Z v_c within transform_tolerance + tol_lambda / s_c                                           -- fit_score_tolerance()
  orthonormality: v_i . v_k = u_i' G u_k / (s_i s_k), so |v_i . v_k - delta_ik| <= 2 tol_lambda / (s_i s_k) + (p + 2) u
                                                                                                     -- gram_tolerance()
  scores against scikit-learn's: Z (v - v') has norm <= sqrt(lambda_1) tol_v[i], plus the transform bound of n entries.
"""
import os

import numpy as np

LANES = 64
U = 2.0 ** -53
MAX_N = 4096
K_FIXED = 16.0     # 4 (two standardisations) + 12 (two eigen-decompositions), see above


def moments(X):
    """(mean[p], var[p], scale[p]): the sums over the samples in ascending order, as pca_moments_kernel adds them."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    s = np.zeros(X.shape[1])
    for i in range(n):
        s = s + X[i]
    mean = s / n
    q = np.zeros(X.shape[1])
    for i in range(n):
        d = X[i] - mean
        q = q + d * d
    var = q / n
    return mean, var, np.where(var == 0.0, 1.0, np.sqrt(var))


def standardise(X, mean, scale):
    return (np.asarray(X, dtype=np.float64) - mean) / scale


def rank_floor(n, p, lam1):
    """numpy.linalg.matrix_rank's rule for the Gram matrix: at or below it a component is written as zeros."""
    return max(n, p) * 2.0 ** -52 * lam1


def apply_sign_rule(components, scores):
    """svd_flip(u_based_decision=False): the entry of largest magnitude of every row positive, the lowest column among equals."""
    for c in range(components.shape[0]):
        if components[c, np.argmax(np.abs(components[c]))] < 0:
            components[c] = -components[c]
            scores[:, c] = -scores[:, c]


def fit(X, n_comp=None):
    """psk_pca_fit restated: the dictionary PskContext.pca_fit returns (sweeps = 0: eigh has none)."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    k = min(n, p) if n_comp is None else int(n_comp)
    mean, var, scale = moments(X)
    Z = standardise(X, mean, scale)
    lam, vec = np.linalg.eigh(Z @ Z.T)
    order = np.argsort(-lam, kind="stable")
    lam, vec = np.maximum(lam[order], 0.0), vec[:, order]
    floor = rank_floor(n, p, lam[0])
    sv = np.where(lam[:k] > floor, np.sqrt(lam[:k]), 0.0)
    comp = np.zeros((k, p))
    live = sv > 0
    comp[live] = (vec[:, :k][:, live].T @ Z) / sv[live][:, None]
    scores = vec[:, :k] * sv
    apply_sign_rule(comp, scores)
    return {"mean": mean, "var": var, "scale": scale, "lambda": lam[:min(n, p)], "scores": scores, "components": comp, "sweeps": 0, "Z": Z}


def transform_in_order(X, center, scale, components):
    """psk_pca_transform restated: partial sum l starts from +0.0 and adds z_j * components[c][j] for j = l, l + 64, ... ascending;
    then a_l = a_l + a_(l xor m) for m = 32, 16, 8, 4, 2, 1; a_0 is the score."""
    z = (np.asarray(X, dtype=np.float64) - center) / scale
    m, p = z.shape
    out = np.zeros((m, len(components)))
    lane = np.arange(LANES)
    for c, row in enumerate(np.asarray(components, dtype=np.float64)):
        a = np.zeros((m, LANES))
        for j in range(p):
            a[:, j % LANES] = a[:, j % LANES] + z[:, j] * row[j]
        for s in (32, 16, 8, 4, 2, 1):
            a = a + a[:, lane ^ s]
        out[:, c] = a[:, 0]
    return out


# ---- bounds (module docstring) ---------------------------------------------------------------------------------------------
def var_tolerance(n, mean, var):
    return 2.0 * ((n + 4) * U * var + (n * U * np.abs(mean)) ** 2)


def rho(Z, lam1):
    return float(np.linalg.norm(np.abs(Z), 2) ** 2 / lam1)


def lambda_tolerance(Z, lam1):
    n, p = Z.shape
    return (rho(Z, lam1) + K_FIXED) * (n + p) * U * lam1


def gaps(lam):
    """gap_i over ALL min(n, p) eigenvalues, the numerically zero ones included."""
    lam = np.asarray(lam, dtype=np.float64)
    d = np.abs(lam[:, None] - lam[None, :])
    np.fill_diagonal(d, np.inf)
    return d.min(axis=1)


def vector_tolerance(lam, tol_lambda):
    with np.errstate(divide="ignore"):     # (two eigenvalues clamped at 0 have no gap: no bound, and nothing compares them)
        return 2.0 * 2.0 * tol_lambda / gaps(lam)


def transform_tolerance(Z, components):
    return 2.0 * (Z.shape[1] + 4) * U * (np.abs(Z) @ np.abs(components).T)


def fit_score_tolerance(Z, components, lam, tol_lambda):
    sv = np.sqrt(np.asarray(lam, dtype=np.float64)[:len(components)])
    with np.errstate(divide="ignore"):
        return transform_tolerance(Z, components) + np.where(sv > 0, tol_lambda / sv, 0.0)[None, :]


def gram_tolerance(lam, tol_lambda, p):
    sv = np.sqrt(np.asarray(lam, dtype=np.float64))
    return 2.0 * tol_lambda / (sv[:, None] * sv[None, :]) + (p + 2) * U


def kept_prefix(lam, n):
    """explained_variance_ > 0.9: a prefix, explained variance being sorted."""
    return np.asarray(lam, dtype=np.float64) / (n - 1) > 0.9


class Engine:
    """Stands in for PskContext.pca_fit / pca_transform in CPU tests: the same arguments, results and refusals, computed here."""

    def pca_fit(self, X, n_comp=None):
        X = np.asarray(X, dtype=np.float32)
        n, p = X.shape
        k = min(n, p) if n_comp is None else int(n_comp)
        if n < 2 or n > MAX_N or p < 1 or not 1 <= k <= min(n, p):
            raise ValueError("psk_pca_fit: bad n, p or n_comp")
        if not np.all(np.isfinite(X)):
            raise ValueError("psk_pca_fit: X has an entry that is not finite")
        out = fit(X, k)
        out.pop("Z")
        return out

    def pca_transform(self, X, center, scale, components):
        return transform_in_order(np.asarray(X, dtype=np.float32), center, scale, components)


class Fixture:
    """tests/golden/pca_kat.npz: per design d (names[d] = A .. E) the dictionary
    X[n][p], y[n] (labels), w[n] (weights), solver (scikit-learn's _fit_svd_solver), mean, var, scale (StandardScaler),
    ev, evr, sv (PCA: explained_variance_, explained_variance_ratio_, singular_values_, all min(n, p)), n_stored, components
    [n_stored][p] and scores[n][n_stored] (the rows above the rank floor), keep_ev (explained variance > 0.9), ttest[kept][5]
    (oracle.ttest_row per component of keep_ev: t, p, mean_x, mean_y, n_with) and keep (PCs_to_keep, min(n, p) booleans)."""

    def __init__(self, path=None):
        self.path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_kat.npz")
        z = np.load(self.path, allow_pickle=False)
        self.sklearn_version = str(z["sklearn_version"])
        self.names = [str(s) for s in z["names"]]
        self.designs = {}
        for name in self.names:
            d = {k: z["%s_%s" % (name, k)] for k in ("X", "y", "w", "mean", "var", "scale", "ev", "evr", "sv", "components", "scores",
                                                     "keep_ev", "ttest", "keep")}
            d["X"] = d["X"].astype(np.float64)
            d["y"] = d["y"].astype(np.int64)
            d["solver"] = str(z["%s_solver" % name])
            d["n"], d["p"] = d["X"].shape
            d["n_stored"] = len(d["components"])
            d["lambda"] = d["sv"] ** 2
            self.designs[name] = d
