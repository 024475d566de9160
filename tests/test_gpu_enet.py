"""GPU tests of the elastic-net path (-m gpu): psk_enet_fit on its three routes, model.ElasticNetRegression under GridSearch
and `--penalty L1+L2` end to end.  Yardstick: scikit-learn's recorded fits (tests/golden/enet_kat.npz,
tools/gen_enet_golden.py), with the bounds of test_gpu_parity.py::test_lasso_covariance_form_walks_sklearns_path
(enet_restated.judge): the sweep count ==, the coefficients within 1e-6 of the largest, the same support, the intercept to
rel 1e-6 / abs 1e-9."""
import os

import numpy as np
import pytest

import enet_restated as R

pytestmark = pytest.mark.gpu

EINVAL = -1
KNOBS = ("PSK_NO_LASSO_COV", "PSK_NO_LASSO_BITS")


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


@pytest.fixture(autouse=True)
def no_route_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _name(D):
    return "%dx%d%s" % (D["n"], D["p"], " counts" if D["counts"] else "")


def _fit_all(ctx, fx, D, call):
    return ctx.enet_fit(D["X"], D["y"], D["fold"], call["alpha"], call["held"], call["l1_ratio"], fx.tol, fx.max_iter)


@pytest.mark.parametrize("d", range(len(R.SHAPES)), ids=["%dx%d" % s[:2] for s in R.SHAPES])
def test_every_recorded_fit_on_its_natural_route(ctx, fx, d):
    """One call per design and l1_ratio carries all its fits: the covariance form up to 1,024 columns, the bit-packed kernel at
    90 x 1030, the float kernel on the count design."""
    D = fx.designs[d]
    for call in fx.calls[d]:
        coef, icpt, iters = _fit_all(ctx, fx, D, call)
        worst = R.judge(_name(D), coef, icpt, iters, call)
        print("%s l1_ratio=%g: sweeps %d..%d, worst coefficient error / largest %.3g" % (_name(D), call["l1_ratio"], iters.min(), iters.max(), worst))


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("d", [d for d, s in enumerate(R.SHAPES) if not s[2]], ids=["%dx%d" % s[:2] for s in R.SHAPES if not s[2]])
def test_the_residual_routes_walk_the_same_path(ctx, fx, d, knob, monkeypatch):
    """The 0/1 designs again on the four-wave bit-packed kernel (PSK_NO_LASSO_COV=1) and on the float kernel
    (PSK_NO_LASSO_BITS=1), with the same bounds."""
    monkeypatch.setenv(knob, "1")
    D = fx.designs[d]
    for call in fx.calls[d]:
        coef, icpt, iters = _fit_all(ctx, fx, D, call)
        R.judge(_name(D) + " " + knob, coef, icpt, iters, call)


@pytest.mark.parametrize("knob", (None,) + KNOBS)
def test_l1_ratio_one_is_the_lasso_bit_for_bit(ctx, fx, knob, monkeypatch):
    """With l1_ratio = 1 every term the elastic net adds is an exact +0.0: psk_lasso_fit's coefficients, intercepts and sweep
    counts, on each route (the natural one of every design, then the two residual routes on the 0/1 designs)."""
    if knob:
        monkeypatch.setenv(knob, "1")
    alpha, held = R.plan()
    for D in fx.designs:
        if knob and D["counts"]:
            continue
        a = ctx.enet_fit(D["X"], D["y"], D["fold"], alpha, held, 1.0, fx.tol, fx.max_iter)
        b = ctx.lasso_fit(D["X"], D["y"], D["fold"], alpha, held, fx.tol, fx.max_iter)
        for u, v, what in zip(a, b, ("coef", "intercept", "sweeps")):
            assert np.array_equal(u, v), (_name(D), knob, what)


def test_grid_search_keeps_every_column(ctx, fx):
    """GridSearch(ElasticNetRegression(l1_ratio=0.5), "alpha", ..., 10) on the 90 x 1030 design -- above the 1,024 columns from
    which a Lasso's copies are solved once -- against the recorded GridSearchCV: every split score (Lasso's bound), the best
    alpha, the refit; and the duplicate pair's two coefficients are scikit-learn's two, which differ (the no-dedupe rule)."""
    from phenotypeseeker_amd.model import ElasticNetRegression, GridSearch
    g = fx.gs
    D = fx.designs[g["design"]]
    gs = GridSearch(ElasticNetRegression(l1_ratio=g["l1_ratio"], tol=fx.tol, max_iter=fx.max_iter), "alpha",
                    [float(a) for a in g["alphas"]], R.N_FOLDS).fit(D["X"], D["y"], ctx)
    assert np.array_equal(gs.test_folds_, D["fold"])
    assert gs.n_unique_columns_ == D["p"]
    ours = np.array([gs.cv_results_["split%d_test_score" % f] for f in range(R.N_FOLDS)]).T
    print("largest split score difference %.3g" % np.abs(ours - g["split_scores"]).max())
    assert np.allclose(ours, g["split_scores"], rtol=1e-5, atol=1e-7), np.abs(ours - g["split_scores"]).max()
    assert gs.best_params_["alpha"] == pytest.approx(g["best_alpha"])
    be = gs.best_estimator_
    scale = np.abs(g["coef"]).max()
    assert np.abs(be.coef_ - g["coef"]).max() <= 1e-6 * scale
    assert be.intercept_ == pytest.approx(g["icpt"], rel=1e-6, abs=1e-9)
    pair = (R.DUP_COL, D["p"] - 1)
    assert np.array_equal(D["X"][:, pair[0]], D["X"][:, pair[1]])
    for j in pair:
        assert g["coef"][j] != 0.0 and abs(be.coef_[j] - g["coef"][j]) <= 1e-6 * scale, j
    assert g["coef"][pair[0]] != g["coef"][pair[1]]


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan")], ids=["-0.1", "1.5", "nan"])
def test_l1_ratio_outside_the_unit_interval_is_refused(ctx, fx, bad):
    from phenotypeseeker_amd.engine import PskError
    D, call = fx.designs[0], fx.calls[0][0]
    with pytest.raises(PskError) as e:
        ctx.enet_fit(D["X"], D["y"], D["fold"], call["alpha"], call["held"], bad, fx.tol, fx.max_iter)
    assert e.value.code == EINVAL and "l1_ratio" in str(e.value)
    coef, icpt, iters = _fit_all(ctx, fx, D, call)      # the context is usable afterwards
    R.judge(_name(D), coef, icpt, iters, call)


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


def test_cli_end_to_end(tmp_path, monkeypatch):
    """PSK_ENET=1 phenotypeseeker modeling --penalty L1+L2 --l1_ratio 0.3 on a continuous synthetic phenotype (synth.GenomeSet,
    as test_gpu_e2e.py::test_continuous_phenotype_end_to_end) writes the three linreg files; the summary names the ElasticNet,
    the .pkl holds a GridSearchCV over it; `phenotypeseeker prediction` on the same samples writes X @ coef + intercept;
    without the knob the run is refused."""
    from phenotypeseeker_amd.synth import GenomeSet
    gs = GenomeSet(40, 8000, seed=41, gene_len=150)
    wd = tmp_path / "run"
    wd.mkdir()
    os.chdir(wd)
    rows, n_valued = ["ID\tAddresses\tMIC"], 0
    for i in range(gs.n):
        name, fa = gs.sample(i)
        with open(name + ".fasta", "wb") as f:
            f.write(fa)
        v = "NA" if i == 7 else repr(round(gs.continuous_phenotype(i), 4))
        n_valued += v != "NA"
        rows.append("%s\t%s.fasta\t%s" % (name, name, v))
    with open("data.pheno", "w") as f:
        f.write("\n".join(rows) + "\n")
    argv = ["modeling", "data.pheno", "--penalty", "L1+L2", "--l1_ratio", "0.3", "--pvalue", "0.05"]
    monkeypatch.delenv("PSK_ENET", raising=False)
    with pytest.raises(SystemExit) as e:
        _run(wd, argv)
    assert str(e.value) == "Only the L1 and L2 penalties run on the GPU engine, got 'L1+L2'."
    monkeypatch.setenv("PSK_ENET", "1")
    _run(wd, argv)
    names = ["summary_of_linreg_analysis_MIC.txt", "k-mers_and_coefficients_in_linreg_model_MIC.txt", "linreg_model_MIC.pkl"]
    for nm in names:
        assert (wd / nm).exists(), nm
    summary = (wd / names[0]).read_text()
    params = summary.split("Parameters:\n")[1].splitlines()[0]
    assert params == "ElasticNet(l1_ratio=0.3)"
    coef_lines = (wd / names[1]).read_text().splitlines()
    assert coef_lines[0].split("\t")[1] == "coef._in_linreg_model" and len(coef_lines) > 1
    from phenotypeseeker_amd import skpickle
    pkg = skpickle.load_linear_package(str(wd / names[2]))
    assert pkg is not None and pkg["pred_scale"] == "continuous"
    with open(wd / names[2], "rb") as f:
        raw = skpickle._StubUnpickler(f).load()
    assert type(raw["model"]).__name__ == "GridSearchCV" and type(raw["model"].best_estimator_).__name__ == "ElasticNet"
    assert raw["model"].best_estimator_.l1_ratio == 0.3
    block = summary.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: float(ln.split()[2]) for ln in block.splitlines()}
    assert len(trained) == n_valued
    os.chdir(wd)
    with open("samples.txt", "w") as f:
        for line in open("data.pheno").read().splitlines()[1:]:
            if line.strip():
                f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("MIC\t%s\n" % names[2])
    _run(wd, ["prediction", "samples.txt", "phenos.txt"])
    out = open("predictions_MIC.txt").read().splitlines()
    pred = {ln.split("\t")[0]: float(ln.split("\t")[1]) for ln in out[1:]}
    assert set(trained) <= set(pred)
    # X @ coef + intercept: the summary's training predictions are that product on the same rows
    for k, v in trained.items():
        assert pred[k] == pytest.approx(v, rel=1e-9, abs=1e-9), k
    coef = {ln.split("\t")[0]: float(ln.split("\t")[1]) for ln in coef_lines[1:]}
    carriers = {ln.split("\t")[0]: set(ln.rstrip("\n").split("\t")[3].split()) if len(ln.split("\t")) > 3 else set() for ln in coef_lines[1:]}
    icpt = float(np.asarray(pkg["model"].intercept_))
    for k in trained:
        want = icpt + sum(c for km, c in coef.items() if k in carriers[km])
        assert pred[k] == pytest.approx(want, rel=1e-9, abs=1e-9), k
