"""GPU tests of the gradient-boosting path (-m gpu): psk_gb_fit, psk_gb_decision, model.GradientBoosting on the device and
`-bc XGBC` / `-reg XGBR` end to end.  Yardsticks: the NumPy restatement of the contract (tests/gb_restated.py) with ==, on
every output of every sample, and scikit-learn's recorded fits (tests/golden/gb_kat.npz, tools/gen_gb_golden.py) within the
bound the record carries (8 x max(scikit-learn's own spread over random_state, 2^-52 max|F|))."""
import os

import numpy as np
import pytest

import gb_restated as R
from test_gb_host import Fixture

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -4
KEYS = ("node_count", "nodes", "value", "impurity", "staged", "raw")


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def same(got, want, what):
    for key in KEYS:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)


def test_golden_cases_equal_the_restatement_and_meet_scikit_learns_record(ctx, fx):
    """Per design ONE psk_gb_fit call carries the all-sample fit and every fold-masked fit; the depth-1 and depth-4 cases follow."""
    seen = 0
    for d, D in enumerate(fx.designs):
        loss = int(d >= 3)
        main = [c for c in fx.cases if c["design"] == d and (c["stages"], c["depth"]) == (30, 3)]
        assert [c["fit_fold"] for c in main] == [-1, 0, 1, 2]
        fits = ctx.gb_fit(D["X"], D["y"], D["fold"], [-1, 0, 1, 2], loss, 30, fx.rate, 3, [c["init_raw"] for c in main])
        extra = [c for c in fx.cases if c["design"] == d and c["stages"] == 10]
        for c in extra:
            fits += ctx.gb_fit(D["X"], D["y"], D["fold"], [-1], loss, 10, fx.rate, c["depth"], [c["init_raw"]])
        for c, f in zip(main + extra, fits):
            same(f, c["fit"], c["k"])
            err = float(np.abs(f["staged"][:, c["in_bag"]] - c["staged"]).max())
            assert err <= float(c["bound"]), (c["k"], err, float(c["bound"]))
            seen += 1
    assert seen == len(fx.cases)


def design(n, p, seed):
    """A 0/1 design with three causal columns (the strongest one last), a continuous and a 0/1 target and a 3-fold vector."""
    rng = np.random.default_rng(seed)
    X = (rng.random((n, p)) < rng.uniform(.2, .8, p)).astype(np.float32)
    z = 2.0 * X[:, p - 1] - 1.5 * X[:, p // 2] + X[:, 0]
    y = z + 0.3 * rng.normal(0.0, 1.0, n)
    y01 = (rng.random(n) < 1.0 / (1.0 + np.exp(-(2.0 * z - 1.0)))).astype(np.float64)
    return X, (y, y01), (rng.permutation(n) % 3).astype(np.int32)


@pytest.mark.parametrize("n,p,depth,stages", [(63, 5, 3, 8), (64, 5, 3, 8), (70, 5, 3, 8), (130, 65, 3, 6), (200, 1030, 1, 6), (200, 1030, 3, 5),
                                              (4096, 8, 3, 3)])
@pytest.mark.parametrize("loss", [0, 1])
def test_shapes_where_the_kernel_can_go_wrong(ctx, n, p, depth, stages, loss):
    """Word boundary and tail (63, 64, 70); three words and more columns than a wave (130 x 65); the second trip of the
    1,024-thread column loop (200 x 1,030); the full LDS residual array (4,096)."""
    X, ys, fold = design(n, p, 7 * n + p)
    y = ys[loss]
    fit_fold = [-1, 1]
    init = [R.init_raw(y, fold != ff, loss) for ff in fit_fold]
    got = ctx.gb_fit(X, y, fold, fit_fold, loss, stages, 0.1, depth, init)
    want = R.fit(X, y, fold, fit_fold, loss, stages, 0.1, depth, init)
    for j in range(2):
        same(got[j], want[j], (n, p, depth, loss, j))
        assert got[j]["node_count"].max() > 1
    if p > 1024:                     # a column of the second trip is the best one of some root
        assert got[0]["nodes"][:, 0, 0].max() >= 1024


@pytest.mark.parametrize("loss", [0, 1])
def test_a_design_built_to_hit_the_rules(ctx, loss):
    """A constant column, two identical columns (the lower index wins), a column and its complement (one partition: the lower
    index wins), and a fit whose in-bag samples of class 1 all lie in one word of 64 samples.  The 0/1 target under the squared
    error gives nodes whose residuals are bit-equal: leaves by this library's own rule."""
    n, p = 200, 12
    rng = np.random.default_rng(11)
    X = (rng.random((n, p)) < 0.5).astype(np.float32)
    X[:, 2] = 1.0                      # constant
    X[:, 5] = X[:, 1]                  # identical to a column before it
    X[:, 0] = 1.0 - X[:, 4]            # the complement of a column behind it
    fold = (rng.permutation(n) % 3).astype(np.int32)
    y = np.zeros(n)
    y[64:128] = X[64:128, 1]           # class 1 in the second word only ...
    extra = np.nonzero(fold == 0)[0][:10]
    y[extra] = 1.0                     # ... and in samples of fold 0, which fit 1 holds out
    assert (y[fold != 0] == 1).sum() > 3 and set(np.nonzero((y == 1) & (fold != 0))[0] // 64) == {1}
    fit_fold = [-1, 0, 2]
    init = [R.init_raw(y, fold != ff, loss) for ff in fit_fold]
    got = ctx.gb_fit(X, y, fold, fit_fold, loss, 6, 0.1, 3, init)
    want = R.fit(X, y, fold, fit_fold, loss, 6, 0.1, 3, init)
    for j in range(3):
        same(got[j], want[j], (loss, j))
        feats = got[j]["nodes"][:, :, 0]
        assert not np.isin(feats[feats >= 0], [2, 5]).any()          # never the constant column, never the later twin
    assert (got[0]["nodes"][:, :, 0] == 1).any()


def test_fits_are_independent_and_in_the_callers_order(ctx, fx):
    for d in (1, 4):
        D, loss = fx.designs[d], int(d >= 3)
        order = [-1, 0, 1, 2]
        init = [R.init_raw(D["y"], D["fold"] != ff, loss) for ff in order]
        four = ctx.gb_fit(D["X"], D["y"], D["fold"], order, loss, 8, 0.1, 3, init)
        back = ctx.gb_fit(D["X"], D["y"], D["fold"], order[::-1], loss, 8, 0.1, 3, init[::-1])
        for j in range(4):
            same(back[3 - j], four[j], (d, j))
            alone = ctx.gb_fit(D["X"], D["y"], D["fold"], [order[j]], loss, 8, 0.1, 3, [init[j]])[0]
            same(alone, four[j], (d, j, "alone"))
        assert not np.array_equal(four[0]["raw"], four[1]["raw"])
        assert ctx.gb_fit(D["X"], D["y"], D["fold"], [-1], loss, 8, 0.1, 3, init[:1], staged=False)[0]["staged"] is None


def test_refusals_name_the_entry_point_and_leave_the_context_usable(ctx, fx):
    from phenotypeseeker_amd._lib import PskError
    D = fx.designs[3]
    X, y, fold = D["X"], D["y"], D["fold"]
    good = lambda **kw: ctx.gb_fit(**{**dict(X=X, y=y, fold=fold, fit_fold=[-1, 1], loss=1, n_estimators=4, learning_rate=0.1, max_depth=3,
                                             init_raw=[0.1, 0.2], staged=False), **kw})
    want = good()[1]["raw"]

    def refused(code, text, **kw):
        with pytest.raises(PskError) as e:
            good(**kw)
        assert e.value.code == code and "psk_gb_fit" in str(e.value) and text in str(e.value), (kw.keys(), str(e.value))
        assert np.array_equal(good()[1]["raw"], want)

    big = 4097
    refused(ERANGE, "at most 4096 samples", X=np.zeros((big, 1), dtype=np.float32), y=np.arange(big) % 2.0, fold=np.zeros(big, dtype=np.int32),
            fit_fold=[-1], init_raw=[0.0])
    for depth in (0, 11):
        refused(EINVAL, "max_depth", max_depth=depth)
    for stages in (0, 1001):
        refused(EINVAL, "n_estimators", n_estimators=stages)
    for rate in (0.0, -0.1, float("nan"), float("inf")):
        refused(EINVAL, "learning_rate", learning_rate=rate)
    for loss in (-1, 2):
        refused(EINVAL, "loss", loss=loss)
    refused(EINVAL, "labels 0 and 1", y=np.where(np.arange(96) == 5, 2.0, y))
    refused(EINVAL, "no finite target", loss=0, y=np.where(np.arange(96) == 5, np.nan, y))
    one_class_fold = np.where(y == 1, 0, 1).astype(np.int32)           # holding fold 0 out leaves class 0 alone
    refused(EINVAL, "fit 1 are of one class", fold=one_class_fold, fit_fold=[-1, 0])
    assert len(ctx.gb_fit(X, y, one_class_fold, [-1, 0], 0, 2, 0.1, 3, [0.0, 0.0], staged=False)) == 2      # the squared error takes it
    refused(EINVAL, "fit 1 has no in-bag sample", fold=np.zeros(96, dtype=np.int32), fit_fold=[-1, 0])
    X2 = X.copy()
    X2[64, 33] = 2.0                                                    # a count is not a presence bit
    refused(EINVAL, "0/1 design", X=X2)
    # psk_gb_decision: the same design check, and a tree that is not a pre-order tree on these columns
    f = ctx.gb_fit(X, y, fold, [-1], 1, 4, 0.1, 3, [0.1])[0]
    model = lambda nodes: (f["node_count"], nodes, f["value"], 0.1, 0.1, 3)
    raw = ctx.gb_decision(X, *model(f["nodes"]))
    assert np.array_equal(raw, f["raw"])
    with pytest.raises(PskError) as e:
        ctx.gb_decision(X2, *model(f["nodes"]))
    assert e.value.code == EINVAL and "psk_gb_decision" in str(e.value)
    for field, bad in ((0, 40), (1, 0), (2, 15), (2, int(f["node_count"][1]))):
        nodes = f["nodes"].copy()
        nodes[1, 0, field] = bad
        with pytest.raises(PskError) as e:
            ctx.gb_decision(X, *model(nodes))
        assert e.value.code == EINVAL and "psk_gb_decision" in str(e.value) and "stage 1" in str(e.value), (field, bad)
    assert np.array_equal(ctx.gb_decision(X, *model(f["nodes"])), raw)


def test_decision_equals_the_fits_raw_predictions_and_the_restatement(ctx, fx):
    for c in fx.cases:
        if c["fit_fold"] not in (-1, 2):
            continue
        D, f = fx.designs[c["design"]], c["fit"]
        got = ctx.gb_decision(D["X"], f["node_count"], f["nodes"], f["value"], c["init_raw"], fx.rate, c["depth"])
        assert np.array_equal(got, f["raw"]), c["k"]
        assert np.array_equal(got, R.decision(D["X"], f["node_count"], f["nodes"], f["value"], c["init_raw"], fx.rate, c["depth"])), c["k"]
    # rows the model has not seen, more than a word of them, and one row
    c = fx.cases[13]
    f = c["fit"]
    Xn = (np.random.default_rng(3).random((131, 40)) < 0.5).astype(np.float64)
    args = (f["node_count"], f["nodes"], f["value"], c["init_raw"], fx.rate, c["depth"])
    got = ctx.gb_decision(Xn, *args)
    assert np.array_equal(got, R.decision(Xn, *args)) and np.array_equal(ctx.gb_decision(Xn[70:71], *args), got[70:71])


@pytest.mark.parametrize("k", [0, 13])
def test_estimator_on_the_device_equals_the_restatement(ctx, fx, k):
    from phenotypeseeker_amd import model as M
    c = fx.cases[k]
    D, f = fx.designs[c["design"]], c["fit"]
    y = D["y"] if c["loss"] == 0 else D["y"].astype(np.int64)
    m = M.GradientBoosting("log_loss" if c["loss"] else "squared_error", n_estimators=30).fit(D["X"], y, ctx)
    assert m.init_raw_ == c["init_raw"]
    assert np.array_equal(m.node_count_, f["node_count"]) and np.array_equal(m.nodes_, f["nodes"])
    assert np.array_equal(m.value_, f["value"]) and np.array_equal(m.impurity_, f["impurity"])
    assert np.array_equal(m.raw(D["X"], ctx), f["raw"]) and np.array_equal(m.raw(D["X"]), f["raw"])
    assert np.array_equal(m.staged_raw(D["X"]), f["staged"])
    assert np.array_equal(m.feature_importances_, R.feature_importances(f, 40))
    assert np.abs(m.train_score_ - c["train_score"]).max() <= 1e-12
    assert np.array_equal(m.predict(D["X"], ctx), m.predict(D["X"])) and m.score(D["X"], y, ctx) == m.score(D["X"], y)
    if c["loss"]:
        assert np.array_equal(m.predict(D["X"], ctx), c["predict"].astype(np.int64))
        assert np.abs(m.predict_proba(D["X"], ctx) - c["proba"]).max() <= float(c["bound"])
    else:
        assert np.abs(m.predict(D["X"], ctx) - c["predict"]).max() <= float(c["bound"])


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


def _predict_again(wd, pheno, pkl, trained, header):
    """`phenotypeseeker prediction` on the training samples with the written model file: the summary's predictions again."""
    os.chdir(wd)
    with open("samples.txt", "w") as f:
        for line in open("data.pheno").read().splitlines()[1:]:
            if line.strip():
                f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("%s\t%s\n" % (pheno, pkl))
    _run(wd, ["prediction", "samples.txt", "phenos.txt"])
    out = open("predictions_%s.txt" % pheno).read().splitlines()
    assert out[0] == header
    pred = {ln.split("\t")[0]: ln.split("\t")[1] for ln in out[1:]}
    assert {k: pred[k] for k in trained} == trained
    return out


def _files(wd, short, pheno):
    names = ["summary_of_%s_analysis_%s.txt" % (short, pheno), "k-mers_and_coefficients_in_%s_model_%s.txt" % (short, pheno),
             "%s_model_%s.pkl" % (short, pheno)]
    for nm in names:
        assert (wd / nm).exists(), nm
    summary = (wd / names[0]).read_text()
    assert "Grid scores" not in summary and "Best parameters" not in summary
    block = summary.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: ln.split()[2] for ln in block.splitlines()}
    coef = (wd / names[1]).read_text().splitlines()
    assert coef[0] == "K-mer\tcoef._in_%s_model\tNo._of_samples_with_k-mer\tSamples_with_k-mer" % short and len(coef) > 1
    imp = np.array([float(ln.split("\t")[1]) for ln in coef[1:]])
    assert np.all(imp >= 0) and abs(imp.sum() - 1.0) < 1e-9
    return summary, trained, names[2]


def test_bc_xgbc_end_to_end(tmp_path, monkeypatch):
    """PSK_GB=1 phenotypeseeker modeling -bc XGBC writes the three GBC files; `prediction` with the .pkl reproduces the summary's
    training predictions (raw values from psk_gb_decision on the open context)."""
    from helpers import load_dataset
    from test_host_modeling import _write_dataset
    ds = load_dataset("ds_omitB")
    wd = tmp_path / "run"
    wd.mkdir()
    _write_dataset(ds, str(wd))
    monkeypatch.delenv("PSK_GB", raising=False)
    with pytest.raises(SystemExit) as e:
        _run(wd, ["modeling", "data.pheno", "-bc", "XGBC", "--omit_B_correction", "--n_kmers", "100"])
    assert "Only the logistic-regression classifier runs on the GPU engine, got 'XGBC'" in str(e.value)
    monkeypatch.setenv("PSK_GB", "1")
    _run(wd, ["modeling", "data.pheno", "-bc", "XGBC", "--omit_B_correction", "--n_kmers", "100"])
    summary, trained, pkl = _files(wd, "GBC", "Pheno")
    assert summary.startswith("Parameters:\nGradientBoostingClassifier()\n") and "Mean accuracy: " in summary
    assert len(trained) == sum(1 for v in ds["pheno"] if v != "NA") and not (wd / "log_reg_model_Pheno.pkl").exists()
    out = _predict_again(wd, "Pheno", pkl, trained, "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class")
    for ln in out[1:]:
        assert 0.0 <= float(ln.split("\t")[2]) <= 1.0


def test_reg_xgbr_end_to_end(tmp_path, monkeypatch):
    """PSK_GB=1 phenotypeseeker modeling -reg XGBR on a continuous synthetic phenotype (synth.GenomeSet, as test_gpu_e2e.py builds
    it), with -cv1 3 and the final model on everything; `prediction` reproduces the summary's last block to the digit."""
    import joblib
    from phenotypeseeker_amd.synth import GenomeSet
    gs = GenomeSet(40, 8000, seed=41, gene_len=150)
    wd = tmp_path / "run"
    wd.mkdir()
    os.chdir(wd)
    rows = ["ID\tAddresses\tMIC"]
    for i in range(gs.n):
        name, fa = gs.sample(i)
        with open(name + ".fasta", "wb") as f:
            f.write(fa)
        rows.append("%s\t%s.fasta\t%s" % (name, name, "NA" if i == 7 else repr(round(gs.continuous_phenotype(i), 4))))
    with open("data.pheno", "w") as f:
        f.write("\n".join(rows) + "\n")
    monkeypatch.setenv("PSK_GB", "1")
    _run(wd, ["modeling", "data.pheno", "--pvalue", "0.05", "-reg", "XGBR", "-cv1", "3", "-tow"])
    summary, _, pkl = _files(wd, "GBR", "MIC")
    assert summary.count("Parameters:\nGradientBoostingRegressor()\n") == 4 and "##### Train/test split nr.3: #####" in summary
    assert "The final output model training on the whole dataset:" in summary and "Mean squared error: " in summary
    last = summary.split("The final output model training on the whole dataset:")[1]
    block = last.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: ln.split()[2] for ln in block.splitlines()}
    assert len(trained) == gs.n - 1
    _predict_again(wd, "MIC", pkl, trained, "Sample_ID\tpredicted_phenotype")
    pkg = joblib.load(pkl)
    assert type(pkg["model"]).__name__ == "GradientBoostingRegressor" and pkg["pred_scale"] == "continuous"
    assert pkg["model"].n_estimators_ == 100 and len(pkg["model"].estimators_) == 100
