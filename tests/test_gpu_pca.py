"""GPU tests of the `--pca` path (-m gpu): psk_pca_fit, psk_pca_transform, model_pca on the device and `modeling --pca` /
`prediction` end to end.  Yardsticks: scikit-learn's recorded StandardScaler() + PCA() fits of the designs A .. E
(tests/golden/pca_kat.npz, tools/gen_pca_golden.py) and the NumPy restatement (tests/pca_restated.py), which also derives every
bound used here (tol_var, tol_lambda = K (n + p) 2^-53 lambda_1, tol_v = 4 tol_lambda / gap, the transform bound).  The
transform is == the restatement, which adds in the order include/psk.h states.  Every test prints the worst share of its bounds."""
import os

import numpy as np
import pytest

import pca_restated as R

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -4
DESIGNS = ["A", "B", "C", "D", "E"]


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


@pytest.fixture(scope="module")
def restated(fx):
    """Per design the restatement's fit (its Z is the f64 design the certificates use) and tol_lambda; computed once."""
    out = {}
    for name in fx.names:
        r = R.fit(fx.designs[name]["X"])
        r["tol_lambda"] = R.lambda_tolerance(r["Z"], r["lambda"][0])
        out[name] = r
    return out


@pytest.fixture(scope="module")
def fits(ctx, fx):
    """One psk_pca_fit per design with all min(n, p) components; shared by the tests and left unchanged."""
    return {name: ctx.pca_fit(fx.designs[name]["X"]) for name in fx.names}


@pytest.mark.parametrize("name", DESIGNS)
def test_moments(fx, restated, fits, name):
    D, r, g = fx.designs[name], restated[name], fits[name]
    assert np.array_equal(g["mean"], D["mean"])                       # integer designs have exact sums: bit for bit
    tol = R.var_tolerance(D["n"], r["mean"], r["var"])
    err = np.abs(g["var"] - D["var"])
    print("design %s: worst |var - sklearn| / tol_var = %.3g" % (name, float((err / np.maximum(tol, 1e-300)).max())))
    assert np.all(err <= tol)
    assert np.array_equal(g["scale"], np.where(g["var"] == 0.0, 1.0, np.sqrt(g["var"])))
    if name == "C":
        assert g["var"][-1] == 0.0 and g["scale"][-1] == 1.0           # the constant column
    assert np.count_nonzero(g["var"] == 0.0) == (1 if name == "C" else 0)


@pytest.mark.parametrize("name", DESIGNS)
def test_eigenvalues(fx, restated, fits, name):
    D, r, g = fx.designs[name], restated[name], fits[name]
    n, p, lam = D["n"], D["p"], g["lambda"]
    assert lam.shape == (min(n, p),) and np.all(np.diff(lam) <= 0) and lam.min() >= 0.0
    err = np.abs(lam - D["lambda"])
    print("design %s: %d sweeps; worst |lambda - sklearn| / tol_lambda = %.3g (K = %.2f)"
          % (name, g["sweeps"], float(err.max() / r["tol_lambda"]), R.rho(r["Z"], r["lambda"][0]) + R.K_FIXED))
    assert np.all(err <= r["tol_lambda"])
    assert 1 <= g["sweeps"] < 60
    dead = lam <= R.rank_floor(n, p, lam[0])
    assert dead.sum() == min(n, p) - D["n_stored"]                     # the numerical rank is scikit-learn's
    assert not g["components"][dead].any() and not g["scores"][:, dead].any()
    assert np.all(np.abs(g["components"][~dead]).max(axis=1) > 0)


@pytest.mark.parametrize("name", DESIGNS)
def test_gap_free_certificate(fx, restated, fits, name):
    """What holds of every component above the rank floor whatever the gaps: it is an eigenvector of Z'Z to tol_lambda, the rows
    are orthonormal, and the scores are Z V'."""
    D, r, g = fx.designs[name], restated[name], fits[name]
    Z, lam, tol_lambda = r["Z"], g["lambda"], r["tol_lambda"]
    live = lam > R.rank_floor(D["n"], D["p"], lam[0])
    V, lam_l = g["components"][live], lam[live]
    res = np.linalg.norm((Z.T @ (Z @ V.T)).T - lam_l[:, None] * V, axis=1)
    gram = np.abs(V @ V.T - np.eye(len(V)))
    tol_g = R.gram_tolerance(lam_l, tol_lambda, D["p"])
    tol_s = R.fit_score_tolerance(Z, V, lam_l, tol_lambda)
    err_s = np.abs(g["scores"][:, live] - Z @ V.T)
    print("design %s: worst shares: eigen-residual %.3g, V V' - I %.3g, scores - Z V' %.3g"
          % (name, float(res.max() / tol_lambda), float((gram / tol_g).max()), float((err_s / tol_s).max())))
    assert np.all(res <= tol_lambda)
    assert np.all(gram <= tol_g)
    assert np.all(err_s <= tol_s)


@pytest.mark.parametrize("name", DESIGNS)
def test_against_scikit_learn(fx, restated, fits, name):
    """Every component with explained variance > 0.9, none left out, the sign included; then the two masks."""
    from phenotypeseeker_amd import _stats
    D, r, g = fx.designs[name], restated[name], fits[name]
    n, lam = D["n"], g["lambda"]
    keep_ev = lam / (n - 1) > 0.9
    assert np.array_equal(keep_ev, D["keep_ev"])
    k = int(keep_ev.sum())
    tol_v = R.vector_tolerance(r["lambda"], r["tol_lambda"])[:k]
    assert np.all(tol_v <= 1e-6)
    dv = np.linalg.norm(g["components"][:k] - D["components"][:k], axis=1)
    tol_s = np.sqrt(r["lambda"][0]) * tol_v + np.sqrt(n) * R.fit_score_tolerance(r["Z"], D["components"][:k], r["lambda"], r["tol_lambda"]).max(axis=0)
    ds = np.linalg.norm(g["scores"][:, :k] - D["scores"][:, :k], axis=0)
    print("design %s: %d components > 0.9; worst shares: components %.3g of tol_v (largest tol_v %.2g), scores %.3g"
          % (name, k, float((dv / tol_v).max()), float(tol_v.max()), float((ds / tol_s).max())))
    assert np.all(dv <= tol_v)
    assert np.all(ds <= tol_s)
    y, w = D["y"], D["w"]
    keep = np.zeros(len(lam), dtype=bool)
    for c in range(k):
        s = g["scores"][:, c]
        keep[c] = _stats.welch_weighted(s[y == 1], s[y == 0], w[y == 1], w[y == 0])[1] < 0.01
    assert np.array_equal(keep, D["keep"])


@pytest.mark.parametrize("name", DESIGNS)
def test_sign_rule_determinism_and_n_comp(ctx, fx, fits, name):
    D, g = fx.designs[name], fits[name]
    comp = g["components"]
    live = np.abs(comp).max(axis=1) > 0
    top = np.argmax(np.abs(comp), axis=1)                              # (the first among equal magnitudes)
    assert np.all(comp[np.arange(len(comp)), top][live] > 0)
    again = ctx.pca_fit(D["X"])
    for key in ("mean", "var", "scale", "lambda", "scores", "components"):
        assert np.array_equal(again[key], g[key]), key                 # a pure function of the arguments: identical bits
    assert again["sweeps"] == g["sweeps"]
    one = ctx.pca_fit(D["X"], 1)
    assert one["components"].shape == (1, D["p"]) and one["scores"].shape == (D["n"], 1)
    assert np.array_equal(one["components"][0], comp[0]) and np.array_equal(one["scores"][:, 0], g["scores"][:, 0])
    assert np.array_equal(one["lambda"], g["lambda"])


@pytest.mark.parametrize("name", DESIGNS)
def test_transform(ctx, fx, restated, fits, name):
    from phenotypeseeker_amd import model_pca
    D, r, g = fx.designs[name], restated[name], fits[name]
    X, n = D["X"], D["n"]
    live = g["lambda"] > R.rank_floor(n, D["p"], g["lambda"][0])
    comp = g["components"][live]
    got = ctx.pca_transform(X, g["mean"], g["scale"], comp)
    Z = R.standardise(X, g["mean"], g["scale"])
    tol = R.fit_score_tolerance(Z, comp, g["lambda"][live], r["tol_lambda"])
    err = np.abs(got - g["scores"][:, live])
    print("design %s: worst |transform - scores of the fit| / bound = %.3g" % (name, float((err / tol).max())))
    assert np.all(err <= tol)
    assert np.array_equal(got, R.transform_in_order(X, g["mean"], g["scale"], comp))       # the stated order, bit for bit
    hi = min(n, 70)
    assert np.array_equal(ctx.pca_transform(X[3:hi], g["mean"], g["scale"], comp), got[3:hi])
    assert np.array_equal(ctx.pca_transform(X[-1:], g["mean"], g["scale"], comp), got[-1:])
    assert np.array_equal(ctx.pca_transform(X, g["mean"], g["scale"], comp[1:2]), got[:, 1:2])  # nor on the other components
    # model_pca: the device route equals its NumPy route
    scaler, pca, scores = model_pca.fit(ctx, X)
    assert np.array_equal(scores, g["scores"]) and np.array_equal(pca.components_, g["components"])
    keep = D["keep"]
    on_device, on_host = model_pca.project(scaler, pca, X, keep, ctx), model_pca.project(scaler, pca, X, keep)
    assert on_device.shape == (n, int(keep.sum())) and np.array_equal(on_device, on_host)
    assert np.array_equal(on_device, got[:, keep[live]])
    assert np.array_equal(scaler.transform(X[:5], ctx), scaler.transform(X[:5]))
    assert np.array_equal(pca.transform(X[:5], ctx), pca.transform(X[:5]))


def test_either_side_of_the_single_workgroup_threshold(ctx, fx, restated, fits):
    """Up to 96 samples the eigen-solver is one workgroup with the matrices in LDS (design B sits on the threshold), from 97 on a
    launch per round: design B with its first row repeated takes the other form.  Yardstick: the restatement of that design,
    under the same bounds (both sides carry an error, as scikit-learn's does)."""
    X = np.vstack([fx.designs["B"]["X"], fx.designs["B"]["X"][:1]])
    n, p = X.shape
    assert n == 97
    r, g = R.fit(X), ctx.pca_fit(X)
    Z, tol_lambda = r["Z"], R.lambda_tolerance(r["Z"], r["lambda"][0])
    assert np.array_equal(g["mean"], r["mean"]) and np.all(np.abs(g["var"] - r["var"]) <= R.var_tolerance(n, r["mean"], r["var"]))
    assert np.all(np.abs(g["lambda"] - r["lambda"]) <= tol_lambda)
    live = g["lambda"] > R.rank_floor(n, p, g["lambda"][0])
    assert np.array_equal(live, r["lambda"] > R.rank_floor(n, p, r["lambda"][0])) and not g["components"][~live].any()
    V, lam = g["components"][live], g["lambda"][live]
    res = np.linalg.norm((Z.T @ (Z @ V.T)).T - lam[:, None] * V, axis=1)
    k = int(R.kept_prefix(r["lambda"], n).sum())
    tol_v = R.vector_tolerance(r["lambda"], tol_lambda)[:k]
    dv = np.linalg.norm(g["components"][:k] - r["components"][:k], axis=1)
    print("n = 97: %d sweeps (n = 96: %d); worst shares: lambda %.3g, eigen-residual %.3g, %d kept components %.3g of tol_v"
          % (g["sweeps"], fits["B"]["sweeps"], float(np.abs(g["lambda"] - r["lambda"]).max() / tol_lambda), float(res.max() / tol_lambda),
             k, float((dv / tol_v).max())))
    assert np.all(res <= tol_lambda) and np.all(tol_v <= 1e-6) and np.all(dv <= tol_v)
    again = ctx.pca_fit(X)
    assert np.array_equal(again["components"], g["components"]) and np.array_equal(again["scores"], g["scores"])


def test_error_paths(ctx, fx, fits):
    from phenotypeseeker_amd._lib import PskError
    D = fx.designs["A"]
    for X, n_comp, code, word in ((D["X"][:1], 1, EINVAL, "n="), (np.zeros((4097, 3), dtype=np.float32), 1, ERANGE, "n="),
                                  (D["X"], 0, EINVAL, "n_comp="), (D["X"], 25, EINVAL, "n_comp=")):
        with pytest.raises(PskError) as e:
            ctx.pca_fit(X, n_comp)
        assert e.value.code == code and word in str(e.value), (code, word, str(e.value))
    bad = D["X"].copy()
    bad[5, 7] = np.nan
    with pytest.raises(PskError) as e:
        ctx.pca_fit(bad)
    assert e.value.code == EINVAL and "X" in str(e.value) and "not finite" in str(e.value)
    with pytest.raises(PskError) as e:
        ctx.pca_transform(np.zeros((0, 3), dtype=np.float32), np.zeros(3), np.ones(3), np.zeros((1, 3)))
    assert e.value.code == EINVAL and "m=" in str(e.value)
    again = ctx.pca_fit(D["X"])                                       # the context serves the next call
    assert np.array_equal(again["components"], fits["A"]["components"])


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


@pytest.mark.parametrize("extra", [[], ["-w"]])
def test_cli_end_to_end(tmp_path, monkeypatch, extra):
    """PSK_PCA=1 phenotypeseeker modeling -bc log --pca writes the summary, the PCs_ file and the .pkl; the .pkl goes through
    `phenotypeseeker prediction` on the same samples, by the stub reader and by joblib (scikit-learn's objects), and reproduces
    the summary's training predictions with identical output files."""
    import joblib
    from helpers import load_dataset
    from test_host_modeling import _write_dataset
    monkeypatch.setenv("PSK_PCA", "1")
    ds = load_dataset("ds_omitB")
    names = ["summary_of_log_reg_analysis_Pheno.txt", "PCs_and_coefficients_in_log_reg_model_Pheno.txt", "log_reg_model_Pheno.pkl"]
    wd = tmp_path / "run"
    wd.mkdir()
    _write_dataset(ds, str(wd))
    _run(wd, ["modeling", "data.pheno", "-bc", "log", "--pca", "--omit_B_correction", "--n_kmers", "100"] + extra)
    for nm in names:
        assert (wd / nm).exists(), nm
    assert not (wd / "k-mers_and_coefficients_in_log_reg_model_Pheno.txt").exists()
    summary = (wd / names[0]).read_text()
    block = summary.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: ln.split()[2] for ln in block.splitlines()}
    assert len(trained) == sum(1 for v in ds["pheno"] if v != "NA")
    lines = (wd / names[1]).read_text().splitlines()
    assert lines[0] == "PC\tcoef._in_log_reg_model\texplained_variance\texplained_variance_ratio\tt-test_statistic\tt-test_pvalue"
    pkg = joblib.load(wd / names[2])
    assert set(pkg) == {"model", "kmers", "pca", "pred_scale", "scaler", "pca_model", "PCs_to_keep"} and pkg["pca"] is True
    keep = pkg["PCs_to_keep"]
    assert keep.dtype == bool and len(keep) == pkg["pca_model"].n_components_ and keep.any()
    assert [ln.split("\t")[0] for ln in lines[1:]] == ["PC_%d" % (c + 1) for c in np.nonzero(keep)[0]]
    for ln, c in zip(lines[1:], np.nonzero(keep)[0]):
        cells = ln.split("\t")
        assert len(cells) == 6 and float(cells[2]) > 0.9 and float(cells[5]) < 0.01
        assert cells[2] == f"{pkg['pca_model'].explained_variance_[c]}"
    assert len(pkg["kmers"]) == pkg["scaler"].n_features_in_ == pkg["pca_model"].n_features_in_
    os.chdir(wd)
    with open("samples.txt", "w") as f:
        for line in open("data.pheno").read().splitlines()[1:]:
            if line.strip():
                f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    monkeypatch.delenv("PSK_PCA")
    with pytest.raises(SystemExit) as e:                               # without the knob the refusal stays
        _run(wd, ["prediction", "samples.txt", "phenos.txt"])
    assert str(e.value) == "PCA models are outside the accelerated path."
    monkeypatch.setenv("PSK_PCA", "1")
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("PSK_JOBLIB_LOAD", flag)
        _run(wd, ["prediction", "samples.txt", "phenos.txt"])
        out = open("predictions_Pheno.txt").read().splitlines()
        assert out[0] == "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class"
        pred = {ln.split("\t")[0]: ln.split("\t")[1] for ln in out[1:]}
        assert {k: pred[k] for k in trained} == trained
        outs.append(out)
    assert outs[0] == outs[1]
