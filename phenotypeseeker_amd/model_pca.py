"""The `--pca` branch: StandardScaler and PCA over psk_pca_fit / psk_pca_transform.

PCA_analysis (modeling.py:1147-1206) runs StandardScaler().fit/transform and PCA().fit/transform on the k-mer columns, keeps the
components with explained_variance_ > 0.9, then those whose scores differ between the two phenotype classes (a GSC-weighted
Welch t-test, p < 0.01), and fits the model on them; prediction.py:131-163 applies scaler.transform, pca_model.transform and
[:, PCs_to_keep].  The reference cannot complete that branch -- PCA_analysis calls self.t_test (:1184), which does not exist;
only conduct_t_test (:716) does --, so the contract is scikit-learn 1.7.2's StandardScaler() and PCA() with their default
parameters, and the t-test as conduct_t_test makes it.

The engine fits both at once (psk_pca_fit: moments, the Gram matrix of the standardised design, a Jacobi eigen-solver, the sign
rule of svd_flip(u_based_decision=False)).  The scores of new samples are a sum whose ORDER is fixed (include/psk.h, f11):
psk_pca_transform on the device and scores_in_order() below give the same bits, so a prediction does not depend on where it
was computed.  scikit-learn's own transform (two BLAS products) is another order of the same terms."""
import numpy as np

from .model_search import _NoTemplate, _Twin

LANES = 64    # partial sums of the stated order: the lanes of a wave


def scores_in_order(X, center, scale, components):
    """psk_pca_transform in NumPy: z_j = (X[i][j] - center[j]) / scale[j]; partial sum l starts from +0.0 and adds the rounded
    products z_j * components[c][j] for j = l, l + 64, l + 128, ... in ascending order; then a_l = a_l + a_(l xor m) for m = 32,
    16, 8, 4, 2, 1 over all l at once; a_0 is scores[i][c].  X is taken as the device takes it: rounded to float32."""
    z = (np.asarray(X, dtype=np.float32).astype(np.float64) - center) / scale
    m, p = z.shape
    components = np.asarray(components, dtype=np.float64)
    steps = -(-p // LANES)
    zp = np.zeros((m, steps * LANES))
    zp[:, :p] = z
    cp = np.zeros((len(components), steps * LANES))     # (a padded column adds the product +0.0 to a sum that started at +0.0)
    cp[:, :p] = components
    out = np.zeros((m, len(components)))
    lane = np.arange(LANES)
    for c in range(len(components)):
        a = np.zeros((m, LANES))
        for s in range(steps):
            cols = slice(s * LANES, (s + 1) * LANES)
            a = a + zp[:, cols] * cp[c, cols]
        for s in (32, 16, 8, 4, 2, 1):
            a = a + a[:, lane ^ s]
        out[:, c] = a[:, 0]
    return out


class _Exported:
    """A fitted transformer that goes into the model file as its scikit-learn twin."""

    def to_sklearn_shell(self):
        """The fitted object described for skpickle.dumps (no scikit-learn import), or None when the installed scikit-learn
        has no template."""
        try:
            return self._sklearn().shell()
        except _NoTemplate:
            return None

    def to_sklearn(self):
        """The same fitted object as real scikit-learn's; needs scikit-learn importable."""
        return self._sklearn().real()


class StandardScaler(_Exported):
    """sklearn.preprocessing.StandardScaler() with its default parameters, the fitted attributes from psk_pca_fit."""

    def _set(self, mean, var, scale, n_samples):
        self.mean_, self.var_, self.scale_ = (np.asarray(a, dtype=np.float64).copy() for a in (mean, var, scale))
        self.n_samples_seen_ = np.int64(n_samples)
        self.n_features_in_ = int(len(self.mean_))
        return self

    def transform(self, X, engine_ctx=None):
        """(X - mean_) / scale_, X rounded to float32 as every design of this library is.  On the device when given an engine
        context (psk_pca_transform with unit vectors for components, 512 columns at a time: z * 1 plus products that are zero),
        else in NumPy: one subtraction and one division per entry either way, so the two give the same bits."""
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_features_in_:
            raise ValueError("Expected input with %d features, got %d instead" % (self.n_features_in_, X.shape[-1]))
        X32 = np.asarray(X, dtype=np.float32)
        if engine_ctx is None:
            return (X32.astype(np.float64) - self.mean_) / self.scale_
        out = np.zeros(X32.shape)
        for lo in range(0, X32.shape[1], 512):
            hi = min(lo + 512, X32.shape[1])
            out[:, lo:hi] = engine_ctx.pca_transform(X32[:, lo:hi], self.mean_[lo:hi], self.scale_[lo:hi], np.eye(hi - lo))
        return out

    def _sklearn(self):
        return _Twin("StandardScaler", "sklearn.preprocessing", dict(copy=True, with_mean=True, with_std=True),
                     dict(n_features_in_=self.n_features_in_, n_samples_seen_=self.n_samples_seen_, mean_=self.mean_.copy(),
                          var_=self.var_.copy(), scale_=self.scale_.copy()))


class PCA(_Exported):
    """sklearn.decomposition.PCA() with its default parameters (all min(n, p) components, no whitening), the fitted attributes
    from psk_pca_fit.  Its input is the scaler's output, whose columns have mean zero up to rounding: mean_ is zeros."""

    def _set(self, lam, components, n_samples):
        lam = np.asarray(lam, dtype=np.float64)
        self.components_ = np.asarray(components, dtype=np.float64).copy()
        self.explained_variance_ = lam / (n_samples - 1)
        total = self.explained_variance_.sum()
        self.explained_variance_ratio_ = self.explained_variance_ / total if total > 0 else np.zeros_like(lam)
        self.singular_values_ = np.sqrt(lam)
        self.mean_ = np.zeros(self.components_.shape[1])
        self.n_components_ = int(len(lam))
        self.n_samples_ = int(n_samples)
        self.noise_variance_ = 0.0
        self.n_features_in_ = int(self.components_.shape[1])
        return self

    def transform(self, X, engine_ctx=None):
        """scikit-learn's PCA.transform of an already standardised X: (X - mean_) . components_' in the stated order, on the
        device when given an engine context, in NumPy otherwise: the same bits.  psk_pca_transform takes a float32 design, so X
        is rounded to float32 on BOTH routes: exact for the designs of this library, a loss of 6e-8 relative for a standardised
        matrix.  The pipeline does not come this way: project() hands the device the k-mer design itself."""
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_features_in_:
            raise ValueError("Expected input with %d features, got %d instead" % (self.n_features_in_, X.shape[-1]))
        ones = np.ones(self.n_features_in_)
        if engine_ctx is not None:
            return engine_ctx.pca_transform(X.astype(np.float32), self.mean_, ones, self.components_)
        return scores_in_order(X, self.mean_, ones, self.components_)

    def _sklearn(self):
        return _Twin("PCA", "sklearn.decomposition", {},
                     dict(n_features_in_=self.n_features_in_, _fit_svd_solver="full", mean_=self.mean_.copy(), n_samples_=self.n_samples_,
                          components_=self.components_.copy(), n_components_=self.n_components_,
                          explained_variance_=self.explained_variance_.copy(), explained_variance_ratio_=self.explained_variance_ratio_.copy(),
                          singular_values_=self.singular_values_.copy(), noise_variance_=self.noise_variance_))


def fit(engine_ctx, X):
    """(scaler, pca, scores[n][min(n, p)]) of the design X[n][p]: one psk_pca_fit."""
    X = np.asarray(X)
    r = engine_ctx.pca_fit(X.astype(np.float32))
    n = X.shape[0]
    return StandardScaler()._set(r["mean"], r["var"], r["scale"], n), PCA()._set(r["lambda"], r["components"], n), r["scores"]


def project(scaler, pca, X, keep=None, engine_ctx=None):
    """pca.transform(scaler.transform(X))[:, keep] as ONE sum per score in the stated order: the centre of the two steps together
    is scaler.mean_ + scaler.scale_ * pca.mean_.  On the device when given an engine context, else in NumPy: the same bits.
    Only the components of `keep` (a boolean mask or indices; all when None) are computed: a score depends on its own
    component only."""
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[1] != scaler.n_features_in_:
        raise ValueError("Expected input with %d features, got %d instead" % (scaler.n_features_in_, X.shape[-1]))
    comp = np.asarray(pca.components_, dtype=np.float64)
    if keep is not None:
        comp = comp[np.asarray(keep)]
    center = np.asarray(scaler.mean_, dtype=np.float64) + np.asarray(scaler.scale_, dtype=np.float64) * np.asarray(pca.mean_, dtype=np.float64)
    if comp.shape[0] == 0:
        return np.zeros((X.shape[0], 0))
    if engine_ctx is not None:
        return engine_ctx.pca_transform(X.astype(np.float32), center, scaler.scale_, comp)
    return scores_in_order(X, center, scaler.scale_, comp)


def from_state(scaler_stub, pca_stub):
    """(StandardScaler, PCA) of this module from the attribute dictionaries of a fitted sklearn StandardScaler and PCA as the
    stub reader keeps them; None for anything this module does not serve (a scaler without mean or scale, a whitening PCA)."""
    s, q = scaler_stub.__dict__, pca_stub.__dict__
    if s.get("with_mean") is not True or s.get("with_std") is not True or q.get("whiten") is not False:
        return None
    if any(s.get(k) is None for k in ("mean_", "var_", "scale_")) or any(q.get(k) is None for k in ("components_", "mean_", "singular_values_")):
        return None
    scaler = StandardScaler()._set(s["mean_"], s["var_"], s["scale_"], s.get("n_samples_seen_", 0))
    pca = PCA()
    pca.__dict__.update({k: v for k, v in q.items() if k.endswith("_") and not k.startswith("_")})
    pca.components_, pca.mean_ = np.asarray(q["components_"], dtype=np.float64), np.asarray(q["mean_"], dtype=np.float64)
    pca.n_features_in_ = int(pca.components_.shape[1])
    if pca.n_features_in_ != scaler.n_features_in_:
        return None
    return scaler, pca
