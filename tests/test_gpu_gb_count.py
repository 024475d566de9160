"""GPU tests (-m gpu) of gradient boosting on k-mer counts: psk_gb_fit_counts, psk_gb_decision_counts, model.GradientBoosting
(counts=True) on the device and `-bc XGBC` / `-reg XGBR` with `--real_counts` end to end.  Yardsticks: the NumPy restatement of the
count contract (tests/gb_count_restated.py) with ==, on every output of every sample; psk_gb_fit itself on 0/1 designs, with ==;
and scikit-learn's recorded fits on count designs (tests/golden/gb_count_kat.npz, tools/gen_gb_count_golden.py) within the bound
the record carries (8 x max(scikit-learn's own spread over random_state, 2^-52 max|F|))."""
import csv
import os

import numpy as np
import pytest

import gb_count_restated as C
import gb_restated as R
from helpers import GOLDEN
from test_gb_count_host import fixture, gap_design

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -4
KEYS = ("node_count", "nodes", "threshold", "value", "impurity", "staged", "raw")


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return fixture()


def same(got, want, what, keys=KEYS):
    for key in keys:
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), (what, key)


def test_golden_cases_equal_the_restatement_and_meet_scikit_learns_record(ctx, fx):
    """Per design ONE psk_gb_fit_counts call carries the all-sample fit and every fold-masked fit; the depth-1 and depth-4 cases
    follow.  Kernel == restatement on every output of every sample, hence kernel within the recorded bound of scikit-learn."""
    seen = 0
    for d, D in enumerate(fx.designs):
        loss = int(d >= 3)
        main = [c for c in fx.cases if c["design"] == d and (c["stages"], c["depth"]) == (30, 3)]
        assert [c["fit_fold"] for c in main] == [-1, 0, 1, 2]
        fits = ctx.gb_fit_counts(D["X"], D["y"], D["fold"], [-1, 0, 1, 2], loss, 30, fx.rate, 3, [c["init_raw"] for c in main])
        extra = [c for c in fx.cases if c["design"] == d and c["stages"] == 10]
        for c in extra:
            fits += ctx.gb_fit_counts(D["X"], D["y"], D["fold"], [-1], loss, 10, fx.rate, c["depth"], [c["init_raw"]])
        for c, f in zip(main + extra, fits):
            same(f, c["fit"], c["k"])
            err = float(np.abs(f["staged"][:, c["in_bag"]] - c["staged"]).max())
            print("case %d: %.3g from scikit-learn, bound %.3g" % (c["k"], err, float(c["bound"])))
            assert err <= float(c["bound"]), (c["k"], err, float(c["bound"]))
            seen += 1
    assert seen == len(fx.cases)


@pytest.mark.parametrize("loss", [0, 1])
def test_a_presence_design_is_a_count_design(ctx, loss):
    """Every output of psk_gb_fit_counts on a 0/1 design is psk_gb_fit's, with and without a held-out fold; all thresholds 0.5."""
    g = np.load(os.path.join(GOLDEN, "gb_kat.npz"))
    d = 1 + 3 * loss
    X, y, fold = g["X_%d" % d].astype(np.float64), g["y_%d" % d], g["fold_%d" % d]
    fit_fold = [-1, 1]
    init = [R.init_raw(y, fold != ff, loss) for ff in fit_fold]
    want = ctx.gb_fit(X, y, fold, fit_fold, loss, 20, 0.1, 3, init)
    got = ctx.gb_fit_counts(X, y, fold, fit_fold, loss, 20, 0.1, 3, init)
    for j in range(2):
        same(got[j], want[j], (loss, j), [k for k in KEYS if k != "threshold"])
        split = got[j]["nodes"][:, :, 1] > 0
        assert split.any() and np.all(got[j]["threshold"][split] == 0.5) and np.all(got[j]["threshold"][~split] == -2.0)
        model = (got[j]["node_count"], got[j]["nodes"], got[j]["value"])
        assert np.array_equal(ctx.gb_decision_counts(X, *model, got[j]["threshold"], init[j], 0.1, 3), ctx.gb_decision(X, *model, init[j], 0.1, 3))


def count_design(n, p, seed, values=4, kind=None):
    """Random counts in 0 .. values - 1 with three causal columns (a copy number, a threshold at 2 and a presence), a continuous
    and a 0/1 target and a 3-fold vector.  kind: one of the edge cases of test_shapes_where_the_kernel_can_go_wrong."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, values, (n, p)).astype(np.float64)
    fold = (rng.permutation(n) % 3).astype(np.int32)
    if kind == "wide":                  # one column of 70 distinct values, the largest count among them
        X[:, 1] = rng.permutation(n) % 70
        X[X[:, 1] == 69, 1] = 2.0 ** 24
    if kind == "constant":              # constant over all samples; constant among the in-bag samples of fit 1 only
        X[:, 0] = 3.0
        X[:, 2] = np.where(fold == 1, rng.integers(0, 3, n), 2.0)
    if kind == "flat":
        X[:, :] = np.array([3.0, 0.0, 7.0, 1.0, 2.0])[None, :p]
    z = 0.7 * X[:, p - 1] - 1.5 * (X[:, p // 2] >= 2) + (X[:, 0] > 0) + (0.3 * np.minimum(X[:, 1], 80.0) if kind == "wide" else 0.0)
    y = z + 0.3 * rng.normal(0.0, 1.0, n)
    y01 = (rng.random(n) < 1.0 / (1.0 + np.exp(-(2.0 * (z - z.mean()))))).astype(np.float64)
    return X, (y, y01), fold


@pytest.mark.parametrize("n,p,depth,stages,values,kind", [(63, 5, 3, 8, 4, None), (64, 5, 3, 8, 4, None), (70, 5, 3, 8, 4, None),
                                                          (130, 65, 3, 8, 4, None), (200, 300, 1, 5, 5, None), (200, 300, 3, 5, 5, None),
                                                          (130, 5, 3, 6, 4, "wide"), (130, 5, 3, 6, 4, "constant"), (70, 5, 3, 4, 4, "flat")])
@pytest.mark.parametrize("loss", [0, 1])
def test_shapes_where_the_kernel_can_go_wrong(ctx, n, p, depth, stages, values, kind, loss):
    """Word boundary and tail (63, 64, 70); three words and more planes than a wave (130 x 65); more planes than threads, so that
    the stride loop over the planes wraps (200 x 300 with 5 values a column: about 1,200 planes); a column of 70 distinct values
    up to 2^24; a column that has no plane and one whose planes are all constant in a fit; a design without any plane."""
    X, ys, fold = count_design(n, p, 11 * n + p + depth, values, kind)
    y = ys[loss]
    fit_fold = [-1, 1]
    init = [R.init_raw(y, fold != ff, loss) for ff in fit_fold]
    got = ctx.gb_fit_counts(X, y, fold, fit_fold, loss, stages, 0.1, depth, init)
    want = C.fit(X, y, fold, fit_fold, loss, stages, 0.1, depth, init)
    P = len(C.planes(X)[1])
    for j in range(2):
        same(got[j], want[j], (n, p, depth, kind, loss, j))
        assert np.array_equal(ctx.gb_decision_counts(X, got[j]["node_count"], got[j]["nodes"], got[j]["value"], got[j]["threshold"], init[j],
                                                     0.1, depth), got[j]["raw"])
        if kind == "flat":
            assert P == 0 and np.all(got[j]["node_count"] == 1) and np.all(got[j]["nodes"][:, 0, 0] == -2) and np.all(got[j]["threshold"] == -2.0)
        else:
            assert got[j]["node_count"].max() > 1 and got[j]["threshold"].max() > 0.5
    if p == 300:                     # a plane of the second trip is the best one of some root
        first = np.searchsorted(C.planes(X)[1], got[0]["nodes"][:, 0, 0])
        assert P > 1024 and first.max() >= 1024
    if kind == "wide":
        assert P >= 69 + 3 and X.max() == 2.0 ** 24
    if kind == "constant":
        feats = [got[j]["nodes"][:, :, 0][got[j]["nodes"][:, :, 1] > 0] for j in range(2)]
        assert not (feats[0] == 0).any() and (feats[0] == 2).any() and not np.isin(feats[1], [0, 2]).any()


@pytest.mark.parametrize("loss", [0, 1])
def test_a_design_built_to_hit_the_rules(ctx, loss):
    """A column and its double (one partition at two thresholds: the lower column wins), the copy of a column behind it (the
    lowest threshold of the lowest column), and a 0/1 target, which under the squared error gives nodes whose residuals are
    bit-equal: leaves by this library's own rule."""
    n, p = 200, 8
    rng = np.random.default_rng(23)
    X = rng.integers(0, 4, (n, p)).astype(np.float64)
    X[:, 3] = 2.0 * X[:, 1]            # the double of a column before it
    X[:, 6] = X[:, 2]                  # the copy of a column before it
    fold = (rng.permutation(n) % 3).astype(np.int32)
    y = ((X[:, 1] >= 2) ^ (X[:, 2] >= 1)).astype(np.float64)
    y[rng.random(n) < 0.1] = 1.0
    fit_fold = [-1, 0, 2]
    init = [R.init_raw(y, fold != ff, loss) for ff in fit_fold]
    got = ctx.gb_fit_counts(X, y, fold, fit_fold, loss, 6, 0.1, 3, init)
    want = C.fit(X, y, fold, fit_fold, loss, 6, 0.1, 3, init)
    for j in range(3):
        same(got[j], want[j], (loss, j))
        split = got[j]["nodes"][:, :, 1] > 0
        assert not np.isin(got[j]["nodes"][:, :, 0][split], [3, 6]).any()          # never the double, never the later twin
    assert (got[0]["nodes"][:, :, 0] == 1).any() and (got[0]["threshold"] == 1.5).any()


def test_a_held_out_value_inside_the_gap_goes_left(ctx):
    """Column 0 holds {0, 1, 3}; the in-bag samples of the fit hold {0, 3}; sample 5, held out, holds the 1: threshold 1.5, and the
    sample goes left in `staged` and by psk_gb_decision_counts."""
    X, y, fold = gap_design()
    init = [R.init_raw(y, fold != 1, 0)]
    f = ctx.gb_fit_counts(X, y, fold, [1], 0, 3, 0.1, 2, init)[0]
    same(f, C.fit(X, y, fold, [1], 0, 3, 0.1, 2, init)[0], "gap")
    assert f["nodes"][0, 0, 0] == 0 and f["threshold"][0, 0] == 1.5 and f["nodes"][0, 0, 1] == 1
    assert f["staged"][0][5] == f["staged"][0][1] != f["staged"][0][0]           # with the 0 of sample 1, not the 3 of sample 0
    raw = ctx.gb_decision_counts(X, f["node_count"], f["nodes"], f["value"], f["threshold"], init[0], 0.1, 2)
    assert np.array_equal(raw, f["raw"]) and raw[5] == raw[1]


def test_decision_equals_the_fits_raw_predictions_and_the_host(ctx, fx):
    from phenotypeseeker_amd import model_gb
    for c in fx.cases:
        if c["fit_fold"] not in (-1, 2):
            continue
        D, f = fx.designs[c["design"]], c["fit"]
        args = (f["node_count"], f["nodes"], f["value"], f["threshold"], c["init_raw"], fx.rate, c["depth"])
        got = ctx.gb_decision_counts(D["X"], *args)
        assert np.array_equal(got, f["raw"]), c["k"]
        assert np.array_equal(got, C.decision(D["X"], *args)), c["k"]
    # rows the model has not seen, values absent from training, one row, and more rows than a fit may have
    c = fx.cases[13]
    f = c["fit"]
    host = lambda Z: model_gb.raw_in_order(Z, f["node_count"], f["nodes"], f["value"], c["init_raw"], fx.rate, c["depth"], f["threshold"])
    args = (f["node_count"], f["nodes"], f["value"], f["threshold"], c["init_raw"], fx.rate, c["depth"])
    Xn = np.random.default_rng(3).integers(0, 13, (131, 40)).astype(np.float64)
    got = ctx.gb_decision_counts(Xn, *args)
    assert np.array_equal(got, host(Xn)) and np.array_equal(ctx.gb_decision_counts(Xn[70:71], *args), got[70:71]) and len(set(got)) > 4
    X5, ys, fold = count_design(5000, 5, 77)
    small = ctx.gb_fit_counts(X5[:300], ys[0][:300], fold[:300], [-1], 0, 10, 0.1, 3, [0.0])[0]
    model = (small["node_count"], small["nodes"], small["value"])
    got = ctx.gb_decision_counts(X5 + (np.arange(5000) % 7 == 0)[:, None] * 9.0, *model, small["threshold"], 0.0, 0.1, 3)
    want = model_gb.raw_in_order(X5 + (np.arange(5000) % 7 == 0)[:, None] * 9.0, *model, 0.0, 0.1, 3, small["threshold"])
    assert got.shape == (5000,) and np.array_equal(got, want)


def test_refusals_name_the_entry_point_and_leave_the_context_usable(ctx, fx):
    from phenotypeseeker_amd._lib import PskError
    from phenotypeseeker_amd.engine import _ptr
    D = fx.designs[3]
    X, y, fold = D["X"], D["y"], D["fold"]
    good = lambda **kw: ctx.gb_fit_counts(**{**dict(X=X, y=y, fold=fold, fit_fold=[-1, 1], loss=1, n_estimators=4, learning_rate=0.1, max_depth=3,
                                                    init_raw=[0.1, 0.2], staged=False), **kw})
    want = good()[1]["raw"]

    def refused(code, text, **kw):
        with pytest.raises(PskError) as e:
            good(**kw)
        assert e.value.code == code and "psk_gb_fit_counts" in str(e.value) and text in str(e.value), (kw.keys(), str(e.value))
        assert np.array_equal(good()[1]["raw"], want)

    big = 4097
    refused(ERANGE, "at most 4096 samples", X=np.zeros((big, 1)), y=np.arange(big) % 2.0, fold=np.zeros(big, dtype=np.int32), fit_fold=[-1],
            init_raw=[0.0])
    for depth in (0, 11):
        refused(EINVAL, "max_depth", max_depth=depth)
    one_class_fold = np.where(y == 1, 0, 1).astype(np.int32)           # holding fold 0 out leaves class 0 alone
    refused(EINVAL, "fit 1 are of one class", fold=one_class_fold, fit_fold=[-1, 0])
    # the library's own check of the values names sample and column; the Python layer checks before its cast to float32
    n, p = X.shape
    y64, f32, ff, init = y.astype(np.float64), fold.astype(np.int32), np.array([-1], dtype=np.int32), np.array([0.1])
    cap = 15
    count, nodes = np.zeros(4, dtype=np.int32), np.zeros((4, cap, 4), dtype=np.int32)
    val, imp, thr, raw = np.zeros((4, cap)), np.zeros((4, cap)), np.zeros((4, cap)), np.zeros(n)
    for bad in (1.5, -1.0):
        Xb = np.ascontiguousarray(X, dtype=np.float32)
        Xb[64, 33] = bad
        rc = ctx._lib.psk_gb_fit_counts(ctx._h, _ptr(Xb), _ptr(y64), n, p, _ptr(f32), _ptr(ff), 1, 1, 4, 0.1, 3, _ptr(init), _ptr(count), _ptr(nodes),
                                        _ptr(val), _ptr(imp), _ptr(thr), _ptr(raw), None)
        msg = ctx._lib.psk_last_error(ctx._h).decode()
        assert rc == EINVAL and "psk_gb_fit_counts takes a count design" in msg and "sample 64, column 33 holds %g" % bad in msg, (bad, msg)
        with pytest.raises(ValueError):
            good(X=Xb)
    X2 = X.copy()
    X2[64, 33] = 2.0 ** 24 + 1                                          # float32 would round it to 2^24
    with pytest.raises(ValueError) as e:
        good(X=X2)
    assert "gb_fit_counts takes a count design" in str(e.value)
    X2[64, 33] = 2.0 ** 24
    assert len(good(X=X2)) == 2
    assert np.array_equal(good()[1]["raw"], want)
    # psk_gb_decision_counts: the same value check, a tree that is not a pre-order tree on these columns, a threshold that is not finite
    f = ctx.gb_fit_counts(X, y, fold, [-1], 1, 4, 0.1, 3, [0.1])[0]
    model = lambda nodes, thr: (f["node_count"], nodes, f["value"], thr, 0.1, 0.1, 3)
    raw = ctx.gb_decision_counts(X, *model(f["nodes"], f["threshold"]))
    assert np.array_equal(raw, f["raw"])
    Xb = np.ascontiguousarray(X, dtype=np.float32)
    Xb[64, 33] = 1.5
    rc = ctx._lib.psk_gb_decision_counts(ctx._h, _ptr(Xb), n, p, 4, 3, _ptr(f["node_count"]), _ptr(f["nodes"]), _ptr(f["value"]),
                                         _ptr(f["threshold"]), 0.1, 0.1, _ptr(raw.copy()))
    assert rc == EINVAL and "psk_gb_decision_counts takes a count design" in ctx._lib.psk_last_error(ctx._h).decode()
    with pytest.raises(ValueError):
        ctx.gb_decision_counts(Xb, *model(f["nodes"], f["threshold"]))
    for field, bad in ((0, 40), (1, 0), (2, 15), (2, int(f["node_count"][1]))):
        nodes = f["nodes"].copy()
        nodes[1, 0, field] = bad
        with pytest.raises(PskError) as e:
            ctx.gb_decision_counts(X, *model(nodes, f["threshold"]))
        assert e.value.code == EINVAL and "psk_gb_decision_counts" in str(e.value) and "stage 1" in str(e.value), (field, bad)
    assert f["nodes"][1, 0, 0] >= 0
    for bad in (np.nan, np.inf):
        thr = f["threshold"].copy()
        thr[1, 0] = bad
        with pytest.raises(PskError) as e:
            ctx.gb_decision_counts(X, *model(f["nodes"], thr))
        assert e.value.code == EINVAL and "psk_gb_decision_counts" in str(e.value) and "not finite" in str(e.value)
    assert np.array_equal(ctx.gb_decision_counts(X, *model(f["nodes"], f["threshold"])), raw)
    # the 0/1 entry points still refuse a count
    with pytest.raises(PskError) as e:
        ctx.gb_fit(X, y, fold, [-1], 1, 4, 0.1, 3, [0.1])
    assert e.value.code == EINVAL and "psk_gb_fit takes a 0/1 design" in str(e.value)


@pytest.mark.parametrize("k", [0, 13])
def test_counts_estimator_on_the_device_equals_the_restatement(ctx, fx, k):
    from phenotypeseeker_amd import model as M
    c = fx.cases[k]
    D, f = fx.designs[c["design"]], c["fit"]
    y = D["y"] if c["loss"] == 0 else D["y"].astype(np.int64)
    m = M.GradientBoosting("log_loss" if c["loss"] else "squared_error", n_estimators=30, counts=True).fit(D["X"], y, ctx)
    assert m.init_raw_ == c["init_raw"]
    assert np.array_equal(m.node_count_, f["node_count"]) and np.array_equal(m.nodes_, f["nodes"]) and np.array_equal(m.threshold_, f["threshold"])
    assert np.array_equal(m.value_, f["value"]) and np.array_equal(m.impurity_, f["impurity"])
    assert np.array_equal(m.raw(D["X"], ctx), f["raw"]) and np.array_equal(m.raw(D["X"]), f["raw"])
    assert np.array_equal(m.staged_raw(D["X"]), f["staged"])
    assert np.abs(m.train_score_ - c["train_score"]).max() <= 1e-12
    assert np.array_equal(m.predict(D["X"], ctx), m.predict(D["X"]))
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


@pytest.mark.parametrize("flag,model,short", [("-bc", "XGBC", "GBC"), ("-reg", "XGBR", "GBR")])
def test_real_counts_end_to_end(tmp_path, monkeypatch, flag, model, short):
    """PSK_GB=1 PSK_GB_COUNTS=1 modeling --real_counts on synthetic genomes (synth.GenomeSet, as test_gpu_gb.py builds them) some of
    which carry the gene twice, with a phenotype that follows the copy number: the three files exist, the .pkl loads with joblib
    into scikit-learn's estimator with a split above 0.5, its predictions on the training counts are the summary's, and
    `prediction` runs on the same files through psk_gb_decision_counts."""
    import joblib
    from phenotypeseeker_amd import model_gb
    from phenotypeseeker_amd.synth import GenomeSet
    gs = GenomeSet(40, 8000, seed=41, gene_len=150)
    os.chdir(tmp_path)
    rows = ["ID\tAddresses\tPheno"]
    for i in range(gs.n):
        name, fa = gs.sample(i)
        copies = int(gs.has_gene(i))
        if copies and (i // 2) % 2 == 0:   # the gene again, on a contig of its own: its k-mers occur twice in the sample
            body = fa.split(b"\n", 1)[1].replace(b"\n", b"")
            fa = fa + b">dup\n" + body[4000:4150] + b"\n"
            copies = 2
        with open(name + ".fasta", "wb") as f:
            f.write(fa)
        noise = float(np.random.default_rng([41, i]).normal(0.0, 0.05))
        rows.append("%s\t%s.fasta\t%s" % (name, name, int(copies == 2) if model == "XGBC" else repr(round(0.5 + copies + noise, 4))))
    with open("data.pheno", "w") as f:
        f.write("\n".join(rows) + "\n")
    monkeypatch.setenv("PSK_GB", "1")
    monkeypatch.delenv("PSK_GB_COUNTS", raising=False)
    with pytest.raises(SystemExit) as e:
        _run(tmp_path, ["modeling", "data.pheno", flag, model, "--real_counts", "--omit_B_correction", "--pvalue", "0.01"])
    assert "--real_counts is not supported with %s %s" % (flag, model) in str(e.value)
    monkeypatch.setenv("PSK_GB_COUNTS", "1")
    _run(tmp_path, ["modeling", "data.pheno", flag, model, "--real_counts", "--omit_B_correction", "--pvalue", "0.01"])
    with open("Pheno_MLdf.csv") as f:
        ml = list(csv.reader(f))
    cells = np.array([[int(v) for v in r[1:-2]] for r in ml[1:]])
    assert cells.max() >= 2 and cells.shape[0] == gs.n                  # a selected k-mer occurs twice in some sample
    names = ["summary_of_%s_analysis_Pheno.txt" % short, "k-mers_and_coefficients_in_%s_model_Pheno.txt" % short, "%s_model_Pheno.pkl" % short]
    for nm in names:
        assert os.path.exists(nm), nm
    pkg = joblib.load(names[2])
    sk = pkg["model"]
    assert type(sk).__name__ == ("GradientBoostingClassifier" if model == "XGBC" else "GradientBoostingRegressor")
    assert len(pkg["kmers"]) == cells.shape[1] and sk.n_estimators_ == 100
    thr = np.concatenate([e.tree_.threshold[e.tree_.children_left != -1] for e in sk.estimators_[:, 0]])
    assert thr.max() > 0.5 and np.array_equal(2.0 * thr, np.floor(2.0 * thr))
    summary = open(names[0]).read()
    assert summary.startswith("Parameters:\n%s()\n" % type(sk).__name__)
    block = summary.split("Predicted_phenotype\n")[1].split("\n\n")[0].splitlines()
    pred = sk.predict(cells.astype(np.float64))
    if model == "XGBC":
        assert [int(ln.split()[2]) for ln in block] == list(pred)
    else:
        assert np.abs(np.array([float(ln.split()[2]) for ln in block]) - pred).max() <= 1e-12
    back = model_gb.from_sklearn(sk)
    assert back is not None and back.counts                             # what `prediction` makes of the file: the device path
    with open("samples.txt", "w") as f:
        for line in rows[1:]:
            f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    _run(tmp_path, ["prediction", "samples.txt", "phenos.txt"])
    out = open("predictions_Pheno.txt").read().splitlines()
    assert len(out) == 1 + gs.n
    assert out[0] == ("Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class" if model == "XGBC" else "Sample_ID\tpredicted_phenotype")
    for ln, row in zip(out[1:], rows[1:]):
        cols = ln.split("\t")
        assert cols[0] == row.split()[0] and np.isfinite(float(cols[1]))
