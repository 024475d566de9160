"""GPU tests of the decision-tree path (-m gpu): psk_tree_fit, model.DecisionTree behind GridSearch and `-bc DT` end to end.
Two yardsticks: the NumPy restatement of scikit-learn's builder with the lowest-column tie rule (tests/tree_restated.py) on
EVERY case of tests/golden/tree_kat.npz, and scikit-learn's own recorded trees on the cases where its unseeded tie rule does
not matter (the seed-invariant ones, tools/gen_tree_golden.py), with no restatement in between.  Integers are ==,
impurities within 1e-12 (f64 functions of small integers bounded by 1; the device's log may differ from the C library's
in the last place)."""
import os

import numpy as np
import pytest

import tree_restated as R

pytestmark = pytest.mark.gpu

ATOL = 1e-12


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
def gpu_fits(ctx, fx):
    """Per design ONE launch: the 20 fixture cases on all samples, then fold-masked fits of every fold at three depths under
    both criteria.  {design: [(depth, criterion, fold, fit)]}"""
    out = {}
    for d, D in enumerate(fx.designs):
        jobs = [(c["depth"], c["criterion"], -1) for c in fx.cases if c["design"] == d]
        jobs += [(dp, cr, f) for cr in R.CRITERIA for dp in (2, 5, 10) for f in range(int(D["folds"].max()) + 1)]
        fits = ctx.tree_fit(D["X"], D["y"], D["folds"], [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
        out[d] = [j + (t,) for j, t in zip(jobs, fits)]
    print("psk_tree_fit: %d fits in %d launches" % (sum(len(v) for v in out.values()), len(out)))
    return out


def assert_same_tree(got, want, where):
    assert got["node_count"] == want["node_count"] and got["max_depth"] == want["max_depth"], where
    for k in ("feature", "left", "right", "n_node_samples", "counts"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert float(np.abs(got["impurity"] - want["impurity"]).max()) <= ATOL, where


def test_equals_the_restatement_on_every_case(fx, gpu_fits):
    """All depths, both criteria, the duplicated and complemented designs, fold-masked fits batched with the others; the
    leaf and the class-1 fraction of EVERY sample, held-out ones included."""
    n_all = n_fold = 0
    worst = 0.0
    for d, fits in gpu_fits.items():
        D = fx.designs[d]
        for depth, crit, fold, t in fits:
            where = (d, crit, depth, fold)
            want = R.fit(D["X"], D["y"], D["folds"] != fold, depth, crit)
            assert_same_tree(t, want, where)
            worst = max(worst, float(np.abs(t["impurity"] - want["impurity"]).max()))
            assert np.array_equal(t["leaf"], want["leaf"]), where
            assert np.array_equal(t["frac"], want["frac"]), where        # one correctly rounded division of the same integers
            if fold >= 0:
                te = D["folds"] == fold
                assert np.array_equal(R.apply(t, D["X"][te]), t["leaf"][te]), where
                n_fold += 1
            else:
                n_all += 1
    print("restatement: %d all-sample fits and %d fold-masked fits equal; largest impurity deviation %.3g" % (n_all, n_fold, worst))
    assert n_all == len(fx.cases) and n_fold >= 100


def test_equals_scikit_learn_on_the_seed_invariant_cases(fx, gpu_fits):
    n = 0
    for c in fx.cases:
        if not c["invariant"]:
            continue
        D = fx.designs[c["design"]]
        where = (c["design"], c["criterion"], c["depth"])
        t = [t for depth, crit, fold, t in gpu_fits[c["design"]] if (depth, crit, fold) == (c["depth"], c["criterion"], -1)][0]
        assert_same_tree(t, c["tree"], where)
        assert float(np.abs(R.values(t) - c["value"]).max()) <= ATOL, where
        assert float(np.abs(np.column_stack([1.0 - t["frac"], t["frac"]]) - c["proba"]).max()) <= ATOL, where
        assert float(np.abs(R.importances(t, D["p"]) - c["importances"]).max()) <= ATOL, where
        n += 1
    print("scikit-learn: %d seed-invariant cases equal" % n)
    assert n >= 18


def test_grid_search_reproduces_the_recorded_cv_results(ctx, fx):
    from phenotypeseeker_amd import model as M
    g = fx.gs
    D = fx.designs[g["design"]]
    gs = M.GridSearch(M.DecisionTree(), {"max_depth": g["depths"], "criterion": ["gini", "entropy"]}, cv=g["cv"])
    gs.fit(D["X"], D["y"], ctx)
    r = gs.cv_results_
    assert r["params"] == g["params"]
    for f in range(g["cv"]):
        assert np.array_equal(r["split%d_test_score" % f], g["splits"][:, f]), f
    assert np.array_equal(r["mean_test_score"], g["mean"]) and np.array_equal(r["rank_test_score"], g["rank"])
    assert gs.best_params_ == g["best"]
    c = [c for c in fx.cases if c["design"] == g["design"] and c["criterion"] == g["best"]["criterion"]
         and c["depth"] == g["best"]["max_depth"]][0]
    assert c["invariant"]
    be = gs.best_estimator_
    assert np.array_equal(be.tree_.feature, c["tree"]["feature"]) and np.array_equal(be.tree_.n_node_samples, c["tree"]["n_node_samples"])
    assert float(np.abs(be.predict_proba(D["X"]) - c["proba"]).max()) <= ATOL
    assert float(np.abs(be.feature_importances_ - c["importances"]).max()) <= ATOL
    # the reference's full grid in one launch: 20 candidates x (folds + 1) fits
    full = M.GridSearch(M.DecisionTree(), {"max_depth": list(range(1, 11)), "criterion": ["gini", "entropy"]}, cv=10).fit(D["X"], D["y"], ctx)
    assert len(full.cv_results_["params"]) == 20 and full.cv_results_["params"][0] == {"criterion": "gini", "max_depth": 1}
    assert full.cv_results_["params"][10] == {"criterion": "entropy", "max_depth": 1}
    assert np.array_equal(full.cv_results_["mean_test_score"][[0, 1, 2, 10, 11, 12]] > 0.5, np.ones(6, dtype=bool))


def test_edges(ctx):
    from phenotypeseeker_amd._lib import PskError
    X = np.array([[0, 0], [0, 1], [1, 0], [1, 1]] * 2, dtype=np.float64)
    y = np.array([0, 1, 1, 0] * 2)
    folds = np.array([0, 1, 1, 0, 1, 0, 0, 1])
    t = ctx.tree_fit(X, y, np.zeros(8, dtype=int), [2, 2], ["gini", "entropy"], [-1, -1])
    for k in range(2):                                   # XOR: the zero-improvement first split is taken, column 0 by the tie rule
        assert list(t[k]["feature"]) == [0, 1, -2, -2, 1, -2, -2] and np.all(t[k]["impurity"][[2, 3, 5, 6]] == 0.0)
        assert list(t[k]["leaf"]) == [2, 3, 5, 6] * 2 and list(t[k]["frac"]) == [0.0, 1.0, 1.0, 0.0] * 2
    y1 = (folds == 0).astype(int)                        # every sample outside fold 0 is of class 0
    one = ctx.tree_fit(X, y1, folds, [3], ["gini"], [0])[0]      # trains on the samples outside fold 0: all of class 0
    assert one["node_count"] == 1 and one["feature"][0] == -2 and one["max_depth"] == 0
    assert np.all(one["leaf"] == 0) and np.all(one["frac"] == 0.0) and list(one["counts"][0]) == [4, 0]
    with pytest.raises(PskError) as e:                   # a count is not a presence bit
        ctx.tree_fit(np.array([[0.0, 2.0], [1.0, 0.0]]), [0, 1], [0, 0], [1], ["gini"], [-1])
    assert e.value.code == -1
    big = np.zeros((4097, 3), dtype=np.float32)
    with pytest.raises(PskError) as e:
        ctx.tree_fit(big, np.arange(4097) % 2, np.zeros(4097, dtype=int), [1], ["gini"], [-1])
    assert e.value.code == -4
    with pytest.raises(PskError):                        # depth 11 would not fit the 2,047-node capacity
        ctx.tree_fit(X, y, np.zeros(8, dtype=int), [11], ["gini"], [-1])
    # 65 samples: a second bit word with one live bit, sample 64 trained on in one fit and held out in the other
    rng = np.random.default_rng(3)
    Xs = (rng.random((65, 3)) < 0.5).astype(np.float64)
    ys = ((Xs[:, 0] + Xs[:, 2] + rng.normal(0, 0.5, 65)) > 1).astype(int)
    fs = np.arange(65) % 3
    got = ctx.tree_fit(Xs, ys, fs, [3, 3], ["gini", "entropy"], [-1, 1])
    for k, (cr, ff) in enumerate((("gini", -1), ("entropy", 1))):
        want = R.fit(Xs, ys, fs != ff, 3, cr)
        assert_same_tree(got[k], want, ("65", cr))
        assert np.array_equal(got[k]["leaf"], want["leaf"]) and np.array_equal(got[k]["frac"], want["frac"])
    # 4096 samples, the largest mask: against the restatement
    rng = np.random.default_rng(11)
    Xb = (rng.random((4096, 70)) < 0.4).astype(np.float64)
    yb = ((Xb[:, 0] + Xb[:, 1] + Xb[:, 2] + rng.normal(0, 0.8, 4096)) > 1.2).astype(int)
    fb = np.arange(4096) % 4
    got = ctx.tree_fit(Xb, yb, fb, [6, 6], ["entropy", "gini"], [1, -1])
    for k, (cr, ff) in enumerate((("entropy", 1), ("gini", -1))):
        want = R.fit(Xb, yb, fb != ff, 6, cr)
        assert_same_tree(got[k], want, ("4096", cr))
        assert np.array_equal(got[k]["leaf"], want["leaf"]) and np.array_equal(got[k]["frac"], want["frac"])


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


def test_cli_end_to_end(tmp_path, monkeypatch, capfd):
    """PSK_DT=1 phenotypeseeker modeling -bc DT writes the three DT files; the .pkl goes through `phenotypeseeker prediction`
    on the same samples and reproduces the summary's training predictions."""
    from helpers import load_dataset
    from test_host_modeling import _write_dataset
    monkeypatch.setenv("PSK_DT", "1")
    ds = load_dataset("ds_omitB")
    names = ["summary_of_DT_analysis_Pheno.txt", "k-mers_and_coefficients_in_DT_model_Pheno.txt", "DT_model_Pheno.pkl"]
    wd = tmp_path / "run"
    wd.mkdir()
    _write_dataset(ds, str(wd))
    _run(wd, ["modeling", "data.pheno", "-bc", "DT", "--omit_B_correction", "--n_kmers", "100"])
    for nm in names:
        assert (wd / nm).exists(), nm
    assert not (wd / "log_reg_model_Pheno.pkl").exists() and not list(wd.glob("*.png"))
    assert capfd.readouterr().err.count("plot (DT_model_<phenotype>_plot.png) is not written") == 1
    summary = (wd / names[0]).read_text()
    assert "Parameters:\nDecisionTreeClassifier()\n" in summary
    grid = summary.split("Grid scores (mean accuracy) on development set: \n")[1].split("\n\n")[0].splitlines()
    assert len(grid) == 20 and grid[0].endswith(" for {'criterion': 'gini', 'max_depth': 1} ")
    assert grid[19].endswith(" for {'criterion': 'entropy', 'max_depth': 10} ")
    best = summary.split("Best parameters found on development set: \n")[1].splitlines()[:2]
    assert best[0].startswith("criterion : ") and best[1].startswith("max_depth : ")
    block = summary.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: ln.split()[2] for ln in block.splitlines()}
    assert len(trained) == sum(1 for v in ds["pheno"] if v != "NA")
    coef_lines = (wd / names[1]).read_text().splitlines()
    assert coef_lines[0] == "K-mer\tcoef._in_DT_model\tNo._of_samples_with_k-mer\tSamples_with_k-mer" and len(coef_lines) > 1
    imp = np.array([float(ln.split("\t")[1]) for ln in coef_lines[1:]])
    assert np.all(imp >= 0.0) and abs(imp.sum() - 1.0) < 1e-9            # importances, not coefficients
    os.chdir(wd)
    with open("samples.txt", "w") as f:
        for line in open("data.pheno").read().splitlines()[1:]:
            if line.strip():
                f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    _run(wd, ["prediction", "samples.txt", "phenos.txt"])
    out = open("predictions_Pheno.txt").read().splitlines()
    assert out[0] == "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class"
    pred = {ln.split("\t")[0]: ln.split("\t")[1] for ln in out[1:]}
    assert {k: pred[k] for k in trained} == trained
    for ln in out[1:]:
        assert 0.0 <= float(ln.split("\t")[2]) <= 1.0
