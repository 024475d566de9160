"""GPU tests (-m gpu) of the tree estimators on k-mer counts: psk_tree_fit_counts, psk_forest_fit_counts, and `--real_counts`
with -bc DT / -bc RF behind PSK_TREE_COUNTS end to end.  Yardsticks: the NumPy restatement (tests/count_tree_restated.py) on
every case, and scikit-learn's own recorded trees (tests/golden/count_tree_kat.npz, tools/gen_count_tree_golden.py) on the
seed-invariant single trees and on all forest trees.  Everything is asserted ==: the counts are integers, a threshold is the
exactly representable midpoint of two integers, and a reported impurity is the same f64 expression over the same integers,
taken on the host through the C library's log (the kernels' own entropies were one ulp off on 32 of 19,509 nodes)."""
import csv
import os

import numpy as np
import pytest

import count_tree_restated as C
import forest_restated as FR
import tree_restated as TR

pytestmark = pytest.mark.gpu

NODE_KEYS = ("feature", "threshold", "left", "right", "n_node_samples", "counts", "impurity")
FOLDS = 3


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return C.Fixture()


class Impurities:
    """The impurity comparison of a whole test: every other figure is asserted where it is met, the impurities are collected
    and asserted == at the test's end, after their largest deviation has been printed."""

    def __init__(self):
        self.nodes = self.off = 0
        self.worst, self.where = 0.0, None

    def add(self, got, want, where):
        dev = np.abs(got - want)
        self.nodes += len(dev)
        self.off += int((dev != 0).sum())
        if len(dev) and float(dev.max()) > self.worst:
            self.worst, self.where = float(dev.max()), where

    def assert_equal(self, what):
        print("%s: %d of %d node impurities differ, by at most %.3g (%s)" % (what, self.off, self.nodes, self.worst, self.where))
        assert self.off == 0, (what, self.off, self.nodes, self.worst, self.where)


def assert_equal_tree(got, want, where, imp=None):
    """Nodes, thresholds and counts ==; the impurities go to `imp` (left out where a test is not about them)."""
    assert got["node_count"] == want["node_count"] and got["max_depth"] == want["max_depth"], where
    for k in NODE_KEYS:
        if k != "impurity":
            assert np.array_equal(got[k], want[k]), (where, k)
    if imp is not None:
        imp.add(got["impurity"], want["impurity"], where)


def forest_launch(fit, D, jobs):
    """jobs: (params, weights[T][n], states[T]) per forest -> (sum0, sum1, trees per forest) of ONE call of `fit`."""
    weight, state, tree_fit = [], [], []
    for f, (q, w, s) in enumerate(jobs):
        weight += list(w)
        state += list(s)
        tree_fit += [f] * len(s)
    s0, s1, trees = fit(D["X"], D["y"], np.array(weight), state, tree_fit, [q["criterion"] for q, _, _ in jobs],
                        [q["max_depth"] for q, _, _ in jobs], [FR.n_max_features(q["max_features"], D["p"]) for q, _, _ in jobs],
                        [q["min_samples_leaf"] for q, _, _ in jobs], [q["min_samples_split"] for q, _, _ in jobs])
    out, k = [], 0
    for _, _, s in jobs:
        out.append(trees[k:k + len(s)])
        k += len(s)
    return s0, s1, out


def forest_draws(seed, n_estimators, n, bootstrap, rows=None):
    rows = np.arange(n) if rows is None else rows
    pairs = [FR.tree_draws(ts, rows, n, bootstrap) for ts in FR.tree_seeds(seed, n_estimators)]
    return [w for w, _ in pairs], [s for _, s in pairs]


@pytest.fixture(scope="module")
def dt_fits(ctx, fx):
    """Per design ONE launch: its 20 recorded cases on all samples, then fold-masked fits.  {design: [(depth, criterion,
    fold, fit)]}"""
    out = {}
    for d, D in enumerate(fx.designs):
        jobs = [(c["depth"], c["criterion"], -1) for c in fx.dt if c["design"] == d]
        jobs += [(dp, cr, f) for cr in C.CRITERIA for dp in (3, 10) for f in range(FOLDS)]
        fits = ctx.tree_fit_counts(D["X"], D["y"], np.arange(D["n"]) % FOLDS, [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
        out[d] = [j + (t,) for j, t in zip(jobs, fits)]
    return out


@pytest.fixture(scope="module")
def rf_fits(ctx, fx):
    """Per design ONE launch with its recorded forests, then two of them again on the samples outside fold 0.
    {design: [(case index, held-out fold or -1, sum0, sum1, trees)]}"""
    out = {}
    for d, D in enumerate(fx.designs):
        ks = [k for k, c in enumerate(fx.rf) if c["design"] == d]
        if not ks:
            continue
        plan = [(k, -1) for k in ks] + [(k, 0) for k in ks[:2]]
        jobs = []
        for k, fold in plan:
            q = fx.rf[k]["params"]
            rows = None if fold < 0 else np.nonzero(np.arange(D["n"]) % FOLDS != fold)[0]
            jobs.append((q,) + tuple(forest_draws(fx.rf[k]["seed"], q["n_estimators"], D["n"], q["bootstrap"], rows)))
        s0, s1, trees = forest_launch(ctx.forest_fit_counts, D, jobs)
        out[d] = [(k, fold, s0[i], s1[i], trees[i], jobs[i]) for i, (k, fold) in enumerate(plan)]
    return out


def test_a_both_calls_equal_the_restatement_on_every_case(fx, dt_fits, rf_fits):
    """(a) nodes, thresholds, impurities, and for EVERY sample -- held-out and weight-0 ones included -- the leaf and the
    fraction / the two sums."""
    n_dt = n_rf = 0
    imp = Impurities()
    for d, fits in dt_fits.items():
        D = fx.designs[d]
        for depth, crit, fold, t in fits:
            want = C.fit(D["X"], D["y"], np.arange(D["n"]) % FOLDS != fold, depth, crit)
            assert_equal_tree(t, want, ("dt", d, crit, depth, fold), imp)
            assert np.array_equal(t["leaf"], want["leaf"]) and np.array_equal(t["frac"], want["frac"]), (d, crit, depth, fold)
            n_dt += 1
    for d, forests in rf_fits.items():
        D = fx.designs[d]
        for k, fold, s0, s1, trees, (q, weights, states) in forests:
            w0, w1 = np.zeros(D["n"]), np.zeros(D["n"])
            for t, (w, s) in enumerate(zip(weights, states)):
                want = C.fit_tree(D["X"], D["y"], w, s, q["criterion"], q["max_depth"], FR.n_max_features(q["max_features"], D["p"]),
                                  q["min_samples_leaf"], q["min_samples_split"])
                assert_equal_tree(trees[t], want, ("rf", k, fold, t), imp)
                assert np.array_equal(trees[t]["leaf"], want["leaf"]), (k, fold, t)
                w0 += want["frac0"]
                w1 += want["frac1"]
                n_rf += 1
            assert np.array_equal(s0, w0) and np.array_equal(s1, w1), (k, fold)      # the same divisions added in the same order
    print("restatement: %d single trees and %d forest trees equal" % (n_dt, n_rf))
    assert n_dt == len(fx.dt) + 4 * 12 and n_rf == 160 + 40
    imp.assert_equal("restatement")


def test_b_both_calls_equal_scikit_learn(fx, dt_fits, rf_fits):
    """(b) the seed-invariant single trees and all forest trees against scikit-learn's own record."""
    n_dt = n_rf = 0
    imp = Impurities()
    for c in fx.dt:
        if not c["invariant"]:
            continue
        t = [t for depth, crit, fold, t in dt_fits[c["design"]] if (depth, crit, fold) == (c["depth"], c["criterion"], -1)][0]
        assert_equal_tree(t, c["tree"], ("dt", c["design"], c["criterion"], c["depth"]), imp)
        assert np.array_equal(t["leaf"], C.apply(c["tree"], fx.designs[c["design"]]["X"]))
        n_dt += 1
    for d, forests in rf_fits.items():
        D = fx.designs[d]
        for k, fold, s0, s1, trees, _ in forests:
            if fold >= 0:
                continue
            c = fx.rf[k]
            for t, (got, want) in enumerate(zip(trees, c["trees"])):
                assert_equal_tree(got, want, ("rf", k, t), imp)
                assert np.array_equal(got["leaf"], C.apply(want, D["X"])), (k, t)
                n_rf += 1
            T = c["params"]["n_estimators"]
            assert float(np.abs(np.column_stack([s0 / T, s1 / T]) - c["proba"]).max()) <= 1e-15, k    # (one rounding of the mean)
    print("scikit-learn: %d seed-invariant single trees and %d forest trees equal" % (n_dt, n_rf))
    assert n_dt >= 22 and n_rf == 160
    thr = np.concatenate([t["threshold"][t["feature"] >= 0] for v in rf_fits.values() for f in v for t in f[4]])
    assert np.any(thr != np.floor(thr) + 0.5) and np.mean(thr != 0.5) > 0.5      # gaps wider than one count occur
    imp.assert_equal("scikit-learn")


def test_c_a_0_1_design_is_a_count_design(ctx):
    """(c) on the recorded 0/1 designs the count calls return what psk_tree_fit / psk_forest_fit return, thresholds 0.5."""
    tfx, ffx = TR.Fixture(), FR.Fixture()
    n_dt = n_rf = 0
    for d, D in enumerate(tfx.designs):
        jobs = [(c["depth"], c["criterion"], -1) for c in tfx.cases if c["design"] == d] + [(4, "gini", 1), (9, "entropy", 0)]
        args = (D["X"], D["y"], D["folds"], [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
        for old, new in zip(ctx.tree_fit(*args), ctx.tree_fit_counts(*args)):
            assert set(new) == set(old) | {"threshold"}
            for k in old:
                assert np.array_equal(new[k], old[k]), (d, k)
            assert np.array_equal(new["threshold"], np.where(new["feature"] >= 0, 0.5, -2.0))
            n_dt += 1
    for d, D in enumerate(ffx.designs):
        ks = [k for k, c in enumerate(ffx.cases) if c["design"] == d]
        if not ks:
            continue
        jobs = [(ffx.cases[k]["params"],) + tuple(forest_draws(ffx.cases[k]["seed"], ffx.cases[k]["params"]["n_estimators"], D["n"],
                                                               ffx.cases[k]["params"]["bootstrap"])) for k in ks]
        a0, a1, old = forest_launch(ctx.forest_fit, D, jobs)
        b0, b1, new = forest_launch(ctx.forest_fit_counts, D, jobs)
        assert np.array_equal(a0, b0) and np.array_equal(a1, b1), d
        for fo, fn in zip(old, new):
            for o, t in zip(fo, fn):
                for k in o:
                    assert np.array_equal(t[k], o[k]), (d, k)
                assert np.array_equal(t["threshold"], np.where(t["feature"] >= 0, 0.5, -2.0))
                n_rf += 1
    assert n_dt == len(tfx.cases) + 2 * len(tfx.designs) and n_rf == sum(len(c["trees"]) for c in ffx.cases)


def test_d_a_held_out_value_inside_the_gap_is_routed_by_the_threshold(ctx):
    """(d) n = 65, p = 3: the training samples of the root hold {0, 3} in column 1; 1 and 2 occur in held-out samples only.
    scikit-learn's threshold is 1.5, so a held-out 1 goes left and a held-out 2 right -- whichever of the three global gaps
    won the search."""
    n = 65
    X = np.zeros((n, 3))
    X[:, 0] = np.arange(n) % 2                              # uninformative
    X[:, 1] = np.where(np.arange(n) % 3 == 0, 3.0, 0.0)
    X[:, 2] = 5.0                                           # constant
    y = (X[:, 1] == 3).astype(int)
    fold = np.zeros(n, dtype=int)
    fold[[7, 20, 33, 64]] = 1
    X[[7, 20, 33, 64], 1] = [1.0, 2.0, 1.0, 2.0]
    for crit in C.CRITERIA:
        t = ctx.tree_fit_counts(X, y, fold, [2], [crit], [1])[0]
        assert t["feature"][0] == 1 and t["threshold"][0] == 1.5, crit
        left, right = t["left"][0], t["right"][0]
        assert list(t["leaf"][[7, 20, 33, 64]]) == [left, right, left, right], crit
        assert np.array_equal(t["leaf"], C.apply(t, X))
        want = C.fit(X, y, fold != 1, 2, crit)
        assert_equal_tree(t, want, ("gap", crit))
        assert np.array_equal(t["leaf"], want["leaf"]) and np.array_equal(t["frac"], want["frac"])
        w = (fold != 1).astype(int)
        s0, s1, (f,) = ctx.forest_fit_counts(X, y, w[None, :], [12345], [0], [crit], [None], [3], [1], [2])
        assert f["feature"][0] == 1 and f["threshold"][0] == 1.5, crit
        assert list(f["leaf"][[7, 20, 33, 64]]) == [f["left"][0], f["right"][0], f["left"][0], f["right"][0]], crit
        want = C.fit_tree(X, y, w, 12345, crit, None, 3, 1, 2)
        assert_equal_tree(f, want, ("gap forest", crit))
        assert np.array_equal(f["leaf"], want["leaf"]) and np.array_equal(s1[0], want["frac1"])


def test_e_edges(ctx):
    from phenotypeseeker_amd._lib import PskError
    from phenotypeseeker_amd.engine import _ptr
    forest_args = ([0], [0], ["gini"], [None], [1], [1], [2])
    # 2^24, the largest count: the threshold between 0 and 2^24 is 2^23
    X = np.array([[0.0, 1.0], [float(1 << 24), 1.0], [0.0, 1.0], [float(1 << 24), 1.0]])
    t = ctx.tree_fit_counts(X, [0, 1, 0, 1], [0, 0, 0, 0], [1], ["gini"], [-1])[0]
    assert list(t["feature"]) == [0, -2, -2] and list(t["threshold"]) == [float(1 << 23), -2.0, -2.0] and list(t["leaf"]) == [1, 2, 1, 2]
    f = ctx.forest_fit_counts(X, [0, 1, 0, 1], np.ones((1, 4), dtype=int), [7], [0], ["gini"], [None], [2], [1], [2])[2][0]
    assert list(f["feature"]) == [0, -2, -2] and f["threshold"][0] == float(1 << 23)
    # the library's own check (the engine's ValueError is tested on the host): -1, 0.5 and NaN are PSK_EINVAL and name the call
    y, z, depth, crit, all_samples = (np.array(v, dtype=np.int32) for v in ([0, 1], [0, 0], [1], [0], [-1]))
    buf = np.zeros(8 * ctx.TREE_NODE_CAP)                  # room for every output of one fit
    for bad in (-1.0, 0.5, np.nan):
        Xb = np.ascontiguousarray([[0.0, 1.0], [bad, 2.0]], dtype=np.float32)
        rc = ctx._lib.psk_tree_fit_counts(ctx._h, _ptr(Xb), _ptr(y), 2, 2, _ptr(z), _ptr(depth), _ptr(crit), _ptr(all_samples), 1, _ptr(buf),
                                          _ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf))
        assert rc == -1 and "psk_tree_fit_counts takes a count design" in ctx._lib.psk_last_error(ctx._h).decode(), bad
        with pytest.raises(ValueError):
            ctx.tree_fit_counts(Xb, y, z, [1], ["gini"], [-1])
        with pytest.raises(ValueError):
            ctx.forest_fit_counts(Xb, y, np.ones((1, 2), dtype=int), *forest_args)
    big = np.zeros((4097, 3), dtype=np.float32)
    with pytest.raises(PskError) as e:
        ctx.tree_fit_counts(big, np.arange(4097) % 2, np.zeros(4097, dtype=int), [1], ["gini"], [-1])
    assert e.value.code == -4 and "psk_tree_fit_counts keeps" in str(e.value)
    with pytest.raises(PskError) as e:
        ctx.forest_fit_counts(big, np.arange(4097) % 2, np.ones((1, 4097), dtype=int), *forest_args)
    assert e.value.code == -4 and "psk_forest_fit_counts keeps" in str(e.value)
    # an all-constant design has no plane at all: a single leaf
    Xc = np.tile([3.0, 0.0, 7.0], (10, 1))
    t = ctx.tree_fit_counts(Xc, np.arange(10) % 2, np.zeros(10, dtype=int), [4], ["entropy"], [-1])[0]
    assert t["node_count"] == 1 and list(t["feature"]) == [-2] and list(t["threshold"]) == [-2.0] and np.all(t["leaf"] == 0)
    assert np.all(t["frac"] == 0.5)
    s0, s1, (f,) = ctx.forest_fit_counts(Xc, np.arange(10) % 2, np.ones((1, 10), dtype=int), [3], [0], ["gini"], [None], [3], [1], [2])
    assert f["node_count"] == 1 and list(f["threshold"]) == [-2.0] and np.all(s0 == 0.5) and np.all(s1 == 0.5)
    # the 0/1 entry points still refuse a count
    with pytest.raises(PskError) as e:
        ctx.tree_fit(np.array([[0.0, 2.0], [1.0, 0.0]]), [0, 1], [0, 0], [1], ["gini"], [-1])
    assert e.value.code == -1 and "psk_tree_fit takes a 0/1 design" in str(e.value)
    with pytest.raises(PskError) as e:
        ctx.forest_fit(np.array([[0.0, 2.0], [1.0, 0.0]]), [0, 1], np.ones((1, 2), dtype=int), *forest_args)
    assert e.value.code == -1 and "psk_forest_fit takes a 0/1 design" in str(e.value)


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


@pytest.mark.parametrize("bc,extra", [("DT", []), ("RF", ["--n_iter", "4"])])
def test_f_cli_end_to_end(tmp_path, monkeypatch, bc, extra):
    """(f) PSK_DT=1 / PSK_RF=1 with PSK_TREE_COUNTS=1: modeling -bc DT|RF --real_counts on samples some of which carry a
    stretch twice; the three files exist, the .pkl unpickles with thresholds, prediction writes a line per sample."""
    import joblib
    from phenotypeseeker_amd.synth import GenomeSet
    monkeypatch.setenv("PSK_" + bc, "1")
    monkeypatch.setenv("PSK_TREE_COUNTS", "1")
    gs = GenomeSet(24, 6000, seed=91, gene_len=120)
    os.chdir(tmp_path)
    rows = ["ID\tAddresses\tPheno"]
    for i in range(gs.n):
        name, fa = gs.sample(i)
        if i % 3 == 0:   # duplicate a stretch so that some k-mers occur twice in the sample
            body = fa.split(b"\n", 1)[1].replace(b"\n", b"")
            fa = fa + b">dup\n" + body[2980:3100] + b"\n"
        with open(name + ".fasta", "wb") as f:
            f.write(fa)
        rows.append("%s\t%s.fasta\t%d" % (name, name, gs.phenotype(i)))
    with open("data.pheno", "w") as f:
        f.write("\n".join(rows) + "\n")
    _run(tmp_path, ["modeling", "data.pheno", "-bc", bc, "--real_counts", "--omit_B_correction", "--pvalue", "0.5", "--n_kmers", "200"] + extra)
    with open("Pheno_MLdf.csv") as f:
        ml = list(csv.reader(f))
    cells = np.array([[int(v) for v in r[1:-2]] for r in ml[1:]])
    assert cells.max() >= 2 and cells.shape[0] == gs.n            # a selected k-mer occurs twice in some sample
    names = ["summary_of_%s_analysis_Pheno.txt" % bc, "k-mers_and_coefficients_in_%s_model_Pheno.txt" % bc, "%s_model_Pheno.pkl" % bc]
    for nm in names:
        assert os.path.exists(nm), nm
    pkg = joblib.load(names[2])
    be = pkg["model"].best_estimator_
    trees = [e.tree_ for e in be.estimators_] if bc == "RF" else [be.tree_]
    assert len(pkg["kmers"]) == cells.shape[1] and all(t.n_features == cells.shape[1] for t in trees)
    assert np.array_equal(pkg["model"].predict(cells.astype(np.float64)),
                          [int(ln.split()[2]) for ln in open(names[0]).read().split("Predicted_phenotype\n")[1].split("\n\n")[0].splitlines()])
    with open("samples.txt", "w") as f:
        for line in rows[1:]:
            f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    _run(tmp_path, ["prediction", "samples.txt", "phenos.txt"])
    out = open("predictions_Pheno.txt").read().splitlines()
    assert out[0] == "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class" and len(out) == 1 + gs.n
    for ln, row in zip(out[1:], rows[1:]):
        cols = ln.split("\t")
        assert len(cols) == 3 and cols[0] == row.split()[0] and cols[1] in ("0", "1") and 0.0 <= float(cols[2]) <= 1.0
