"""GPU tests of the random-forest path (-m gpu): psk_forest_fit, model.RandomForest behind RandomizedSearch and `-bc RF` end
to end.  Two yardsticks: scikit-learn's own recorded forests (tests/golden/forest_kat.npz, tools/gen_forest_golden.py) on
EVERY case with no restatement in between -- the seed fixes every draw, so the recorded trees are THE answer -- and the NumPy
restatement (tests/forest_restated.py) on what scikit-learn's generator cannot be steered to.  Integers are ==; impurities,
sums and importances within 1e-12 of scikit-learn (f64 functions of small integers bounded by 1; the device's log may differ
from the C library's in the last place), == against the restatement where only correctly rounded divisions are involved."""
import os

import numpy as np
import pytest

import forest_restated as R
import tree_restated as TR

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


def launch(ctx, D, jobs, export=None):
    """jobs: (params, weights[T][n], states[T]) per fit -> (sum0, sum1, trees per fit) of ONE psk_forest_fit call."""
    weight, state, tree_fit = [], [], []
    for f, (q, w, s) in enumerate(jobs):
        weight += list(w)
        state += list(s)
        tree_fit += [f] * len(s)
    s0, s1, trees = ctx.forest_fit(D["X"], D["y"], np.array(weight), state, tree_fit, [q["criterion"] for q, _, _ in jobs],
                                   [q["max_depth"] for q, _, _ in jobs], [R.n_max_features(q["max_features"], D["p"]) for q, _, _ in jobs],
                                   [q["min_samples_leaf"] for q, _, _ in jobs], [q["min_samples_split"] for q, _, _ in jobs], export=export)
    out, k = [], 0
    for q, w, s in jobs:
        out.append(trees[k:k + len(s)])
        k += len(s)
    return s0, s1, out


def draws(seed, n_estimators, n, bootstrap, rows=None):
    rows = np.arange(n) if rows is None else rows
    pairs = [R.tree_draws(ts, rows, n, bootstrap) for ts in R.tree_seeds(seed, n_estimators)]
    return [w for w, _ in pairs], [s for _, s in pairs]


@pytest.fixture(scope="module")
def gpu_cases(ctx, fx):
    """Per design ONE launch with every recorded case of the design.  {case index: (sum0, sum1, trees)}"""
    out, launches = {}, 0
    for d, D in enumerate(fx.designs):
        ks = [k for k, c in enumerate(fx.cases) if c["design"] == d]
        if not ks:
            continue
        jobs = []
        for k in ks:
            q = fx.cases[k]["params"]
            jobs.append((q,) + tuple(draws(fx.cases[k]["seed"], q["n_estimators"], D["n"], q["bootstrap"])))
        s0, s1, trees = launch(ctx, D, jobs)
        launches += 1
        for i, k in enumerate(ks):
            out[k] = (s0[i], s1[i], trees[i])
    print("psk_forest_fit: %d forests, %d trees in %d launches" % (len(out), sum(len(v[2]) for v in out.values()), launches))
    return out


def assert_same_tree(got, want, where):
    assert got["node_count"] == want["node_count"] and got["max_depth"] == want["max_depth"], where
    for k in ("feature", "left", "right", "n_node_samples", "counts"):
        assert np.array_equal(got[k], want[k]), (where, k)
    assert float(np.abs(got["impurity"] - want["impurity"]).max()) <= ATOL, where


def test_equals_scikit_learn_on_every_case(fx, gpu_cases):
    """Every tree of every recorded forest node by node, the leaf of EVERY sample (out-of-bag ones included: they are routed
    through the recorded tree), the two sums against predict_proba, and feature_importances_."""
    n = n_trees = 0
    worst = 0.0
    for k, c in enumerate(fx.cases):
        D = fx.designs[c["design"]]
        s0, s1, trees = gpu_cases[k]
        T = c["params"]["n_estimators"]
        assert len(trees) == len(c["trees"]) == T, k
        for t, (got, want) in enumerate(zip(trees, c["trees"])):
            assert_same_tree(got, want, (k, t))
            worst = max(worst, float(np.abs(got["impurity"] - want["impurity"]).max()))
            assert np.array_equal(got["leaf"], TR.apply(want, D["X"])), (k, t)
            n_trees += 1
        assert float(np.abs(np.column_stack([s0 / T, s1 / T]) - c["proba"]).max()) <= ATOL, k
        assert float(np.abs(R.forest_importances(trees, D["p"]) - c["importances"]).max()) <= ATOL, k
        n += 1
    print("scikit-learn: %d forests, %d trees equal; largest impurity deviation %.3g" % (n, n_trees, worst))
    assert n == len(fx.cases) and n_trees == sum(len(c["trees"]) for c in fx.cases)
    assert max(t["max_depth"] for v in gpu_cases.values() for t in v[2]) >= 20


def against_restatement(ctx, X, y, weights, states, q, where):
    D = dict(X=np.asarray(X, dtype=np.float64), y=np.asarray(y), p=np.asarray(X).shape[1])
    s0, s1, (trees,) = launch(ctx, D, [(q, weights, states)])
    w0, w1 = np.zeros(len(y)), np.zeros(len(y))
    for t, (w, s) in enumerate(zip(weights, states)):
        want = R.fit_tree(D["X"], D["y"], w, s, q["criterion"], q["max_depth"], R.n_max_features(q["max_features"], D["p"]),
                          q["min_samples_leaf"], q["min_samples_split"])
        assert_same_tree(trees[t], want, (where, t))
        assert np.array_equal(trees[t]["leaf"], want["leaf"]), (where, t)
        w0 += want["frac0"]
        w1 += want["frac1"]
    assert np.array_equal(s0[0], w0) and np.array_equal(s1[0], w1), where     # the same divisions added in the same order
    return trees


def test_equals_the_restatement_where_scikit_learn_cannot_be_steered(ctx, fx):
    base = dict(criterion="gini", max_depth=None, max_features=None, min_samples_leaf=1, min_samples_split=2)
    D = fx.designs[3]                                           # 65 x 70, mixed
    rng = np.random.default_rng(9)
    # hand-set weights: multiplicities of 40 and 300 (9 bit planes), zeros, and ordinary small ones
    w = rng.integers(0, 4, size=(3, D["n"]))
    w[:, 5], w[:, 64], w[:, 7] = 40, 300, 0
    for crit, mf in (("gini", None), ("entropy", "sqrt")):
        trees = against_restatement(ctx, D["X"], D["y"], list(w), [11, 0, 2147483646], dict(base, criterion=crit, max_features=mf), ("weights", crit))
        assert trees[0]["counts"][0].sum() == w[0].sum() and trees[0]["n_node_samples"][0] == (w[0] > 0).sum()
    against_restatement(ctx, D["X"], D["y"], list(w), [5, 6, 7], dict(base, criterion="entropy", min_samples_leaf=4, min_samples_split=10, max_depth=5), "weights, limits")
    # in-bag samples of one class: a single leaf, every sample in it
    one = np.where(D["y"] == 1, 3, 0)
    t = against_restatement(ctx, D["X"], D["y"], [one], [1], base, "one class")[0]
    assert t["node_count"] == 1 and t["feature"][0] == -2 and t["max_depth"] == 0 and np.all(t["leaf"] == 0) and t["counts"][0, 0] == 0
    # p = 1
    D1 = fx.designs[0]
    against_restatement(ctx, D1["X"], D1["y"], *draws(4, 3, D1["n"], True), dict(base, max_features="sqrt"), "p = 1")
    # every column constant: the root searches, finds nothing and stays an impure leaf
    Xc = np.tile(np.array([0.0, 1.0, 1.0, 0.0, 1.0]), (30, 1))
    yc = np.arange(30) % 2
    t = against_restatement(ctx, Xc, yc, *draws(2, 2, 30, True), base, "constant")[0]
    assert t["node_count"] == 1 and t["impurity"][0] > 0.4
    # more columns than stay in LDS (the per-column arrays in global memory), more than one round of columns per thread
    Dw = fx.designs[2]
    Xw = np.tile(Dw["X"], (1, 46))[:, :1100]
    against_restatement(ctx, Xw, Dw["y"], *draws(8, 2, Dw["n"], True), dict(base, max_features="log2", criterion="entropy"), "p = 1100")
    against_restatement(ctx, Xw[:, :300], Dw["y"], *draws(8, 2, Dw["n"], True), dict(base, max_features="sqrt"), "p = 300")
    # 4096 samples: the largest label array and 64 mask words
    Xb = (rng.random((4096, 20)) < 0.4).astype(np.float64)
    yb = ((Xb[:, 0] + Xb[:, 1] + Xb[:, 2] + rng.normal(0, 0.8, 4096)) > 1.2).astype(int)
    against_restatement(ctx, Xb, yb, *draws(3, 2, 4096, True), dict(base, max_depth=7, min_samples_leaf=4, max_features="sqrt"), "4096")


def test_a_mixed_launch_equals_each_fit_alone(ctx, fx):
    """60 trees of 12 fits with different parameters, folds held out by zero weights, in one launch: the same trees and sums
    as each fit launched alone; node arrays only for the trees that were flagged."""
    D = fx.designs[4]                                           # 130 x 24, mixed
    jobs = []
    for f in range(12):
        q = dict(criterion=R.CRITERIA[f % 2], max_depth=(None, 4, 20)[f % 3], max_features=R.MAX_FEATURES[(f // 2) % 3],
                 min_samples_leaf=(1, 2, 4)[(f // 3) % 3], min_samples_split=(2, 5, 10)[(f // 4) % 3])
        rows = np.nonzero(np.arange(D["n"]) % 4 != f % 4)[0]
        jobs.append((q,) + tuple(draws(20 + f, 5, D["n"], f % 2 == 0, rows)))
    flag = np.arange(60) % 2 == 0
    s0, s1, trees = launch(ctx, D, jobs, export=flag)
    assert sum(len(t) for t in trees) == 60
    for f, job in enumerate(jobs):
        a0, a1, (alone,) = launch(ctx, D, [job])
        assert np.array_equal(s0[f], a0[0]) and np.array_equal(s1[f], a1[0]), f
        for t in range(5):
            if not flag[5 * f + t]:
                assert trees[f][t] is None
                continue
            assert_same_tree(trees[f][t], alone[t], (f, t))
            assert np.array_equal(trees[f][t]["impurity"], alone[t]["impurity"]) and np.array_equal(trees[f][t]["leaf"], alone[t]["leaf"])
            assert trees[f][t]["counts"][0].sum() == np.sum(job[1][t])


def test_the_recorded_search_end_to_end(ctx, fx):
    from phenotypeseeker_amd import model as M
    g = fx.search
    D = fx.designs[g["design"]]
    rs = M.RandomizedSearch(M.RandomForest(random_state=g["seed"]), g["grid"], g["n_iter"], g["cv"], random_state=g["seed"]).fit(D["X"], D["y"], ctx)
    r = rs.cv_results_
    assert r["params"] == g["params"]
    for f in range(g["cv"]):
        assert np.array_equal(r["split%d_test_score" % f], g["splits"][:, f]), f
    assert np.array_equal(r["mean_test_score"], g["mean"]) and np.array_equal(r["rank_test_score"], g["rank"])
    assert rs.best_params_ == g["best"]
    assert float(np.abs(rs.predict_proba(D["X"]) - g["proba"]).max()) <= ATOL
    assert float(np.abs(rs.best_estimator_.feature_importances_ - g["importances"]).max()) <= ATOL
    # the search split into several engine calls gives the same scores
    small = M.RandomForest(random_state=g["seed"])
    small.SCRATCH_BYTES = 16 * D["n"] * 12
    again = M.RandomizedSearch(small, g["grid"], g["n_iter"], g["cv"], random_state=g["seed"]).fit(D["X"], D["y"], ctx)
    assert np.array_equal(again.cv_results_["mean_test_score"], g["mean"]) and again.best_params_ == g["best"]


def test_edges(ctx):
    from phenotypeseeker_amd._lib import PskError
    args = ([0], [0], ["gini"], [None], [1], [1], [2])
    with pytest.raises(PskError) as e:                   # a count is not a presence bit
        ctx.forest_fit(np.array([[0.0, 2.0], [1.0, 0.0]]), [0, 1], np.ones((1, 2), dtype=int), *args)
    assert e.value.code == -1
    with pytest.raises(PskError) as e:
        ctx.forest_fit(np.zeros((4097, 3), dtype=np.float32), np.arange(4097) % 2, np.ones((1, 4097), dtype=int), *args)
    assert e.value.code == -4
    with pytest.raises(PskError) as e:                   # a tree without a sample
        ctx.forest_fit(np.array([[0.0], [1.0]]), [0, 1], np.zeros((1, 2), dtype=int), *args)
    assert e.value.code == -1


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


def test_cli_end_to_end(tmp_path, monkeypatch):
    """PSK_RF=1 phenotypeseeker modeling -bc RF --n_iter 4 writes the three RF files; the .pkl goes through `phenotypeseeker
    prediction` on the same samples, by the stub reader and by joblib, and reproduces the summary's training predictions."""
    from helpers import load_dataset
    from test_host_modeling import _write_dataset
    monkeypatch.setenv("PSK_RF", "1")
    monkeypatch.setenv("PSK_RF_SEED", "7")
    ds = load_dataset("ds_omitB")
    names = ["summary_of_RF_analysis_Pheno.txt", "k-mers_and_coefficients_in_RF_model_Pheno.txt", "RF_model_Pheno.pkl"]
    wd = tmp_path / "run"
    wd.mkdir()
    _write_dataset(ds, str(wd))
    _run(wd, ["modeling", "data.pheno", "-bc", "RF", "--n_iter", "4", "--omit_B_correction", "--n_kmers", "100"])
    for nm in names:
        assert (wd / nm).exists(), nm
    assert not (wd / "log_reg_model_Pheno.pkl").exists()
    summary = (wd / names[0]).read_text()
    assert "Parameters:\nRandomForestClassifier(random_state=7)\n" in summary
    grid = summary.split("Grid scores (mean accuracy) on development set: \n")[1].split("\n\n")[0].splitlines()
    assert len(grid) == 4 and all("'n_estimators': " in ln and "'bootstrap': " in ln for ln in grid)
    best = summary.split("Best parameters found on development set: \n")[1].splitlines()[:7]
    assert sorted(ln.split(" : ")[0] for ln in best) == sorted(R.REFERENCE_GRID)
    block = summary.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: ln.split()[2] for ln in block.splitlines()}
    assert len(trained) == sum(1 for v in ds["pheno"] if v != "NA")
    coef_lines = (wd / names[1]).read_text().splitlines()
    assert coef_lines[0] == "K-mer\tcoef._in_RF_model\tNo._of_samples_with_k-mer\tSamples_with_k-mer" and len(coef_lines) > 1
    imp = np.array([float(ln.split("\t")[1]) for ln in coef_lines[1:]])
    assert np.all(imp >= 0.0) and abs(imp.sum() - 1.0) < 1e-9            # importances, not coefficients
    os.chdir(wd)
    with open("samples.txt", "w") as f:
        for line in open("data.pheno").read().splitlines()[1:]:
            if line.strip():
                f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("PSK_JOBLIB_LOAD", flag)
        _run(wd, ["prediction", "samples.txt", "phenos.txt"])
        out = open("predictions_Pheno.txt").read().splitlines()
        assert out[0] == "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class"
        pred = {ln.split("\t")[0]: ln.split("\t")[1] for ln in out[1:]}
        assert {k: pred[k] for k in trained} == trained
        for ln in out[1:]:
            assert 0.0 <= float(ln.split("\t")[2]) <= 1.0
        outs.append(out)
    assert outs[0] == outs[1]
