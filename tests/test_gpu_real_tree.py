"""GPU tests (-m gpu) of the tree estimators on real-valued designs: psk_tree_fit_real, psk_forest_fit_real, and `--pca` with
-bc DT / -bc RF behind PSK_TREE_PCA end to end.  Yardsticks: the NumPy restatement (tests/real_tree_restated.py) on every
case, scikit-learn's own recorded trees (tests/golden/real_tree_kat.npz, tools/gen_real_tree_golden.py) on the seed-invariant
single trees, the seeded deep trees and all forest trees, and the existing tree calls on 0/1 and count designs.  Everything
is asserted ==: the counts are integers, a threshold is one f64 expression of two float32 values, and a reported impurity is
the same f64 expression over the same integers, taken on the host through the C library's log.  A forest's predict_proba is
held to 1e-15 for the one rounding of the mean."""
import os

import numpy as np
import pytest

import count_tree_restated as C
import forest_restated as FR
import real_tree_restated as R
import tree_restated as TR
from test_gpu_count_tree import FOLDS, Impurities, assert_equal_tree, forest_draws, forest_launch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


FOLD_JOBS = [(dp, cr, f) for cr in R.CRITERIA for dp in (3, 10) for f in range(FOLDS)]


@pytest.fixture(scope="module")
def dt_fits(ctx, fx):
    """Per design ONE launch: its recorded cases on all samples, then fold-masked fits.  {design: [(depth, criterion, fold, fit)]}"""
    out = {}
    for d, D in enumerate(fx.designs):
        jobs = [(c["depth"], c["criterion"], -1) for c in fx.dt if c["design"] == d] + FOLD_JOBS
        fits = ctx.tree_fit_real(D["X"], D["y"], np.arange(D["n"]) % FOLDS, [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
        out[d] = [j + (t,) for j, t in zip(jobs, fits)]
    return out


DEEP = dict(bootstrap=False, max_depth=None, max_features=None, min_samples_leaf=1, min_samples_split=2, n_estimators=1)


@pytest.fixture(scope="module")
def rf_fits(ctx, fx):
    """Per design ONE launch: its recorded forests, two of them again on the samples outside fold 0, and its seeded deep trees,
    each a forest of one all-ones tree with max_features = p whose tree seed is scikit-learn's random_state.
    {design: [(kind, case index, held-out fold or -1, sum0, sum1, trees, job)]}"""
    out = {}
    for d, D in enumerate(fx.designs):
        ks = [k for k, c in enumerate(fx.rf) if c["design"] == d]
        plan = [("rf", k, -1) for k in ks] + [("rf", k, 0) for k in ks[:2]] + [("deep", k, -1) for k, c in enumerate(fx.deep) if c["design"] == d]
        jobs = []
        for kind, k, fold in plan:
            if kind == "deep":
                w, s = FR.tree_draws(fx.deep[k]["seed"], np.arange(D["n"]), D["n"], False)
                jobs.append((dict(DEEP, criterion=fx.deep[k]["criterion"]), [w], [s]))
                continue
            q = fx.rf[k]["params"]
            rows = None if fold < 0 else np.nonzero(np.arange(D["n"]) % FOLDS != fold)[0]
            jobs.append((q,) + tuple(forest_draws(fx.rf[k]["seed"], q["n_estimators"], D["n"], q["bootstrap"], rows)))
        s0, s1, trees = forest_launch(ctx.forest_fit_real, D, jobs)
        out[d] = [(kind, k, fold, s0[i], s1[i], trees[i], jobs[i]) for i, (kind, k, fold) in enumerate(plan)]
    return out


def test_a_both_calls_equal_the_restatement_on_every_case(fx, dt_fits, rf_fits):
    """(a) nodes, thresholds, impurities, and for EVERY sample -- held-out and weight-0 ones included -- the leaf and the
    fraction / the two sums."""
    n_dt = n_rf = 0
    imp = Impurities()
    for d, fits in dt_fits.items():
        D = fx.designs[d]
        for depth, crit, fold, t in fits:
            want = R.fit(D["X"], D["y"], np.arange(D["n"]) % FOLDS != fold, depth, crit)
            assert_equal_tree(t, want, ("dt", d, crit, depth, fold), imp)
            assert np.array_equal(t["leaf"], want["leaf"]) and np.array_equal(t["frac"], want["frac"]), (d, crit, depth, fold)
            n_dt += 1
    for d, forests in rf_fits.items():
        D = fx.designs[d]
        for kind, k, fold, s0, s1, trees, (q, weights, states) in forests:
            w0, w1 = np.zeros(D["n"]), np.zeros(D["n"])
            for t, (w, s) in enumerate(zip(weights, states)):
                want = R.fit_tree(D["X"], D["y"], w, s, q["criterion"], q["max_depth"], FR.n_max_features(q["max_features"], D["p"]),
                                  q["min_samples_leaf"], q["min_samples_split"])
                assert_equal_tree(trees[t], want, (kind, k, fold, t), imp)
                assert np.array_equal(trees[t]["leaf"], want["leaf"]), (kind, k, fold, t)
                w0 += want["frac0"]
                w1 += want["frac1"]
                n_rf += 1
            assert np.array_equal(s0, w0) and np.array_equal(s1, w1), (kind, k, fold)      # the same divisions added in the same order
    print("restatement: %d single trees and %d forest trees equal" % (n_dt, n_rf))
    assert n_dt == len(fx.dt) + len(FOLD_JOBS) * len(fx.designs)
    assert n_rf >= sum(len(c["trees"]) for c in fx.rf) + len(fx.deep) + 40
    imp.assert_equal("restatement")


def test_b_both_calls_equal_scikit_learn(fx, dt_fits, rf_fits):
    """(b) the seed-invariant single trees, all forest trees, and the seeded deep trees against scikit-learn's own record."""
    n_dt = n_dt3 = n_rf = n_deep = adjacent = 0
    imp = Impurities()
    for c in fx.dt:
        if not c["invariant"]:
            continue
        t = [t for depth, crit, fold, t in dt_fits[c["design"]] if (depth, crit, fold) == (c["depth"], c["criterion"], -1)][0]
        assert_equal_tree(t, c["tree"], ("dt", c["design"], c["criterion"], c["depth"]), imp)
        assert np.array_equal(t["leaf"], R.apply(c["tree"], fx.designs[c["design"]]["X"]))
        n_dt += 1
        n_dt3 += int((t["feature"] >= 0).sum()) >= 3
    for d, forests in rf_fits.items():
        D = fx.designs[d]
        for kind, k, fold, s0, s1, trees, _ in forests:
            if fold >= 0:
                continue
            if kind == "deep":
                assert_equal_tree(trees[0], fx.deep[k]["tree"], ("deep", k), imp)
                assert np.array_equal(trees[0]["leaf"], R.apply(fx.deep[k]["tree"], D["X"])), k
                n_deep += 1
                continue
            c = fx.rf[k]
            for t, (got, want) in enumerate(zip(trees, c["trees"])):
                assert_equal_tree(got, want, ("rf", k, t), imp)
                assert np.array_equal(got["leaf"], R.apply(want, D["X"])), (k, t)
                n_rf += 1
                for j, thr in zip(got["feature"], got["threshold"]):
                    if j >= 0:
                        col = D["X32"][:, j]
                        adjacent += bool(np.nextafter(col[col <= thr].max(), np.float32(np.inf)) == col[col > thr].min())
            T = c["params"]["n_estimators"]
            assert float(np.abs(np.column_stack([s0 / T, s1 / T]) - c["proba"]).max()) <= 1e-15, k    # (one rounding of the mean)
    print("scikit-learn: %d seed-invariant single trees (%d with three splits), %d forest trees, %d seeded deep trees equal; "
          "%d thresholds between adjacent float32 values" % (n_dt, n_dt3, n_rf, n_deep, adjacent))
    # the generator's own conditions: the test cannot pass by comparing nothing
    assert n_dt == fx.n_invariant >= 10 and n_dt3 == fx.n_invariant_3_splits >= 4
    assert n_rf == sum(len(c["trees"]) for c in fx.rf) >= 120 and len(fx.rf) >= 12
    assert n_deep == len(fx.deep) == 4 * len(fx.designs) and adjacent >= 1
    imp.assert_equal("scikit-learn")


def test_c_a_0_1_design_and_a_count_design_are_real_designs(ctx):
    """(c) on the recorded 0/1 designs the real calls return what psk_tree_fit / psk_forest_fit return, thresholds 0.5; on the
    recorded count designs what the count calls return, in every output."""
    tfx, ffx, cfx = TR.Fixture(), FR.Fixture(), C.Fixture()
    n_dt = n_rf = n_cdt = n_crf = 0
    for d, D in enumerate(tfx.designs):
        jobs = [(c["depth"], c["criterion"], -1) for c in tfx.cases if c["design"] == d] + [(4, "gini", 1), (9, "entropy", 0)]
        args = (D["X"], D["y"], D["folds"], [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
        for old, new in zip(ctx.tree_fit(*args), ctx.tree_fit_real(*args)):
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
        b0, b1, new = forest_launch(ctx.forest_fit_real, D, jobs)
        assert np.array_equal(a0, b0) and np.array_equal(a1, b1), d
        for fo, fn in zip(old, new):
            for o, t in zip(fo, fn):
                for k in o:
                    assert np.array_equal(t[k], o[k]), (d, k)
                assert np.array_equal(t["threshold"], np.where(t["feature"] >= 0, 0.5, -2.0))
                n_rf += 1
    assert n_dt == len(tfx.cases) + 2 * len(tfx.designs) and n_rf == sum(len(c["trees"]) for c in ffx.cases)
    for d, D in enumerate(cfx.designs):
        jobs = [(c["depth"], c["criterion"], -1) for c in cfx.dt if c["design"] == d] + [(4, "gini", 1), (9, "entropy", 0)]
        args = (D["X"], D["y"], np.arange(D["n"]) % FOLDS, [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
        for old, new in zip(ctx.tree_fit_counts(*args), ctx.tree_fit_real(*args)):
            assert set(new) == set(old)
            for k in old:
                assert np.array_equal(new[k], old[k]), (d, k)
            n_cdt += 1
        ks = [k for k, c in enumerate(cfx.rf) if c["design"] == d]
        if not ks:
            continue
        jobs = [(cfx.rf[k]["params"],) + tuple(forest_draws(cfx.rf[k]["seed"], cfx.rf[k]["params"]["n_estimators"], D["n"],
                                                            cfx.rf[k]["params"]["bootstrap"])) for k in ks]
        a0, a1, old = forest_launch(ctx.forest_fit_counts, D, jobs)
        b0, b1, new = forest_launch(ctx.forest_fit_real, D, jobs)
        assert np.array_equal(a0, b0) and np.array_equal(a1, b1), d
        for fo, fn in zip(old, new):
            for o, t in zip(fo, fn):
                assert set(t) == set(o)
                for k in o:
                    assert np.array_equal(t[k], o[k]), (d, k)
                n_crf += 1
    assert n_cdt == len(cfx.dt) + 2 * len(cfx.designs) and n_crf == sum(len(c["trees"]) for c in cfx.rf)


def test_d_probes_zeros_gaps_and_a_design_past_the_plane_cap(ctx, fx):
    """(d) the four probes split where scikit-learn split; -0.0 / +0.0 make no gap; a held-out value strictly inside a gap is
    routed by the threshold; a 1,024 x 1,100 Gaussian design, refused by psk_tree_fit_counts on its rank-coded copy, is fitted."""
    from phenotypeseeker_amd._lib import PskError
    for k, pr in enumerate(fx.probes):
        x, n = pr["x"].reshape(-1, 1), len(pr["x"])
        for crit in R.CRITERIA:
            t = ctx.tree_fit_real(x, pr["y"], np.zeros(n, dtype=int), [3], [crit], [-1])[0]
            assert t["node_count"] == 3 and t["threshold"][0] == pr["threshold"], (k, crit)
            assert np.array_equal(t["leaf"], R.apply(t, x)) and len(set(t["leaf"].tolist())) == 2
            f = ctx.forest_fit_real(x, pr["y"], np.ones((1, n), dtype=int), [5], [0], [crit], [None], [1], [1], [2])[2][0]
            assert f["node_count"] == 3 and f["threshold"][0] == pr["threshold"], (k, crit)
    # -0.0 and +0.0 are one value: column 0 is constant, column 1 separates the classes
    n = 70
    y = np.arange(n) % 2
    X = np.zeros((n, 2), dtype=np.float32)
    X[:, 0] = np.where(y == 1, np.float32(-0.0), np.float32(0.0))
    X[:, 1] = np.where(y == 1, np.float32(-0.0), np.float32(-1.5))
    assert set(np.signbit(X[:, 0]).tolist()) == {True, False}
    t = ctx.tree_fit_real(X, y, np.zeros(n, dtype=int), [3], ["gini"], [-1])[0]
    assert list(t["feature"]) == [1, -2, -2] and t["threshold"][0] == -0.75
    t = ctx.tree_fit_real(X[:, :1], y, np.zeros(n, dtype=int), [3], ["entropy"], [-1])[0]
    assert t["node_count"] == 1 and np.all(t["frac"] == 0.5)
    s0, s1, (f,) = ctx.forest_fit_real(X[:, :1], y, np.ones((1, n), dtype=int), [9], [0], ["gini"], [None], [1], [1], [2])
    assert f["node_count"] == 1 and np.all(s1 == 0.5)
    # n = 65, p = 3: the training samples of the root hold {-0.25, 0.5} in column 1; held-out samples lie strictly inside the gap
    n = 65
    X = np.zeros((n, 3))
    X[:, 0] = (np.arange(n) % 2) * 0.3                        # uninformative
    X[:, 1] = np.where(np.arange(n) % 3 == 0, 0.5, -0.25)
    X[:, 2] = 5.25                                            # constant
    y = (X[:, 1] == 0.5).astype(int)
    fold = np.zeros(n, dtype=int)
    held = [7, 20, 33, 64]
    fold[held] = 1
    X[held, 1] = [0.1, 0.2, 0.125, 0.126]                     # the threshold is 0.125: <= goes left
    for crit in R.CRITERIA:
        t = ctx.tree_fit_real(X, y, fold, [2], [crit], [1])[0]
        assert t["feature"][0] == 1 and t["threshold"][0] == 0.125, crit
        left, right = t["left"][0], t["right"][0]
        assert list(t["leaf"][held]) == [left, right, left, right], crit
        want = R.fit(X, y, fold != 1, 2, crit)
        assert_equal_tree(t, want, ("gap", crit))
        assert np.array_equal(t["leaf"], want["leaf"]) and np.array_equal(t["frac"], want["frac"])
        w = (fold != 1).astype(int)
        s0, s1, (f,) = ctx.forest_fit_real(X, y, w[None, :], [12345], [0], [crit], [None], [3], [1], [2])
        assert f["feature"][0] == 1 and f["threshold"][0] == 0.125, crit
        assert list(f["leaf"][held]) == [f["left"][0], f["right"][0], f["left"][0], f["right"][0]], crit
        want = R.fit_tree(X, y, w, 12345, crit, None, 3, 1, 2)
        assert_equal_tree(f, want, ("gap forest", crit))
        assert np.array_equal(f["leaf"], want["leaf"]) and np.array_equal(s1[0], want["frac1"])
    # 1,024 x 1,100: about 1.1 million gaps, more than PSK_TREE_PLANE_CAP threshold planes
    rng = np.random.default_rng(23)
    n, p = 1024, 1100
    X = rng.normal(0.0, 1.0, (n, p)).astype(np.float32)
    y = (X[:, 700] + 0.8 * X[:, 3] + rng.normal(0.0, 0.5, n) > 0).astype(int)
    ranks = np.argsort(np.argsort(X, axis=0, kind="stable"), axis=0).astype(np.float64)
    with pytest.raises(PskError) as e:
        ctx.tree_fit_counts(ranks, y, np.zeros(n, dtype=int), [3], ["gini"], [-1])
    assert e.value.code == -4 and "threshold planes" in str(e.value)
    fits = ctx.tree_fit_real(X, y, np.zeros(n, dtype=int), [3, 3], ["gini", "entropy"], [-1, -1])
    imp = Impurities()
    for crit, t in zip(R.CRITERIA, fits):
        want = R.fit(X, y, np.ones(n, dtype=bool), 3, crit)
        assert_equal_tree(t, want, ("wide", crit), imp)
        assert np.array_equal(t["leaf"], want["leaf"]) and np.array_equal(t["frac"], want["frac"]) and t["node_count"] >= 7
    imp.assert_equal("wide design")


def test_e_edges(ctx):
    from phenotypeseeker_amd._lib import PskError
    from phenotypeseeker_amd.engine import _ptr
    forest_args = ([0], [0], ["gini"], [None], [1], [1], [2])
    # the library's own check (the engine's ValueError is tested on the host): NaN and the infinities are PSK_EINVAL and name the call
    y, z, depth, crit, all_samples = (np.array(v, dtype=np.int32) for v in ([0, 1], [0, 0], [1], [0], [-1]))
    buf = np.zeros(8 * ctx.TREE_NODE_CAP)                  # room for every output of one fit
    wt, state, tfit, flag, one, two = (np.array(v, dtype=t) for v, t in (([1, 1], np.uint16), ([7], np.uint32), ([0], np.int32),
                                                                        ([1], np.int32), ([1], np.int32), ([2], np.int32)))
    for bad in (np.nan, np.inf, -np.inf):
        Xb = np.ascontiguousarray([[0.0, 1.0], [bad, 2.0]], dtype=np.float32)
        rc = ctx._lib.psk_tree_fit_real(ctx._h, _ptr(Xb), _ptr(y), 2, 2, _ptr(z), _ptr(depth), _ptr(crit), _ptr(all_samples), 1, _ptr(buf),
                                        _ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf))
        assert rc == -1 and "psk_tree_fit_real takes a finite float32 design" in ctx._lib.psk_last_error(ctx._h).decode(), bad
        rc = ctx._lib.psk_forest_fit_real(ctx._h, _ptr(Xb), _ptr(y), 2, 2, 1, _ptr(wt), _ptr(state), _ptr(tfit), _ptr(flag), 1, _ptr(crit),
                                          _ptr(z[:1]), _ptr(two), _ptr(one), _ptr(two), _ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf), 3,
                                          _ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf), _ptr(buf))
        assert rc == -1 and "psk_forest_fit_real takes a finite float32 design" in ctx._lib.psk_last_error(ctx._h).decode(), bad
        with pytest.raises(ValueError):
            ctx.tree_fit_real(Xb, y, z, [1], ["gini"], [-1])
        with pytest.raises(ValueError):
            ctx.forest_fit_real(Xb, y, np.ones((1, 2), dtype=int), *forest_args)
    big = np.zeros((4097, 3), dtype=np.float32)
    with pytest.raises(PskError) as e:
        ctx.tree_fit_real(big, np.arange(4097) % 2, np.zeros(4097, dtype=int), [1], ["gini"], [-1])
    assert e.value.code == -4 and "psk_tree_fit_real keeps" in str(e.value)
    with pytest.raises(PskError) as e:
        ctx.forest_fit_real(big, np.arange(4097) % 2, np.ones((1, 4097), dtype=int), *forest_args)
    assert e.value.code == -4 and "psk_forest_fit_real keeps" in str(e.value)
    # an all-constant design is a single leaf
    Xc = np.tile([3.5, -0.25, 7.0], (10, 1))
    t = ctx.tree_fit_real(Xc, np.arange(10) % 2, np.zeros(10, dtype=int), [4], ["entropy"], [-1])[0]
    assert t["node_count"] == 1 and list(t["feature"]) == [-2] and list(t["threshold"]) == [-2.0] and np.all(t["leaf"] == 0)
    assert np.all(t["frac"] == 0.5)
    s0, s1, (f,) = ctx.forest_fit_real(Xc, np.arange(10) % 2, np.ones((1, 10), dtype=int), [3], [0], ["gini"], [None], [3], [1], [2])
    assert f["node_count"] == 1 and list(f["threshold"]) == [-2.0] and np.all(s0 == 0.5) and np.all(s1 == 0.5)
    # p = 1, past one 256-thread trip of samples
    rng = np.random.default_rng(4)
    x = rng.normal(0.0, 1.0, (300, 1)).astype(np.float32)
    y1 = (x[:, 0] + rng.normal(0.0, 0.7, 300) > 0).astype(int)
    t = ctx.tree_fit_real(x, y1, np.arange(300) % 3, [5], ["gini"], [2])[0]
    want = R.fit(x, y1, np.arange(300) % 3 != 2, 5, "gini")
    assert_equal_tree(t, want, "p = 1")
    assert np.array_equal(t["leaf"], want["leaf"]) and t["node_count"] > 3
    w, s = FR.tree_draws(11, np.arange(300), 300, True)
    f = ctx.forest_fit_real(x, y1, w[None, :], [s], [0], ["entropy"], [None], [1], [2], [5])[2][0]
    want = R.fit_tree(x, y1, w, s, "entropy", None, 1, 2, 5)
    assert_equal_tree(f, want, "p = 1 forest")
    assert np.array_equal(f["leaf"], want["leaf"])
    # a fit whose training samples are of one class is a single leaf
    fold = (y1 == 1).astype(int)                              # holding fold 1 out leaves class 0 only
    t = ctx.tree_fit_real(x, y1, fold, [5], ["gini"], [1])[0]
    assert t["node_count"] == 1 and np.all(t["frac"] == 0.0) and list(t["counts"][0]) == [int((y1 == 0).sum()), 0]
    s0, s1, (f,) = ctx.forest_fit_real(x, y1, (y1 == 0).astype(int)[None, :], [3], [0], ["gini"], [None], [1], [1], [2])
    assert f["node_count"] == 1 and np.all(s0 == 1.0) and np.all(s1 == 0.0)


def test_g_either_side_of_the_segment_threshold(ctx):
    """A column's ranks are cut into segments, a thread each, where 2 p is at most the workgroup's threads (1,024 for the single
    tree, 256 for the forest): p = 512 | 513 and p = 128 | 129 lie on either side, and all four equal the restatement."""
    rng = np.random.default_rng(31)
    n = 150
    X = rng.normal(0.0, 1.0, (n, 513)).astype(np.float32)
    X[:, 7] = np.rint(X[:, 7] * 4.0) / 4.0                      # ties that straddle segment borders
    y = (X[:, 100] + 0.7 * X[:, 7] + rng.normal(0.0, 0.6, n) > 0).astype(int)
    fold = np.arange(n) % FOLDS
    imp = Impurities()
    for p in (512, 513):
        fits = ctx.tree_fit_real(X[:, :p], y, fold, [10, 10, 4], ["gini", "entropy", "entropy"], [-1, 0, 1])
        for (depth, crit, ff), t in zip(((10, "gini", -1), (10, "entropy", 0), (4, "entropy", 1)), fits):
            want = R.fit(X[:, :p], y, fold != ff, depth, crit)
            assert_equal_tree(t, want, ("tree", p, crit, ff), imp)
            assert np.array_equal(t["leaf"], want["leaf"]) and np.array_equal(t["frac"], want["frac"]) and t["node_count"] > 7
    for p in (128, 129):
        for seed, (crit, mf, msl, boot) in enumerate((("gini", p, 1, True), ("entropy", 11, 2, False))):
            w, st = FR.tree_draws(seed + 3, np.nonzero(fold != 0)[0], n, boot)
            s0, s1, (t,) = ctx.forest_fit_real(X[:, :p], y, w[None, :], [st], [0], [crit], [None], [mf], [msl], [2])
            want = R.fit_tree(X[:, :p], y, w, st, crit, None, mf, msl, 2)
            assert_equal_tree(t, want, ("forest", p, crit), imp)
            assert np.array_equal(t["leaf"], want["leaf"]) and np.array_equal(s0[0], want["frac0"]) and np.array_equal(s1[0], want["frac1"])
            assert t["node_count"] > 7
    imp.assert_equal("segment threshold")


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


def _write_genomes(tmp_path):
    from phenotypeseeker_amd.synth import GenomeSet
    gs = GenomeSet(24, 6000, seed=91, gene_len=120)
    os.chdir(tmp_path)
    rows = ["ID\tAddresses\tPheno"]
    for i in range(gs.n):
        name, fa = gs.sample(i)
        with open(name + ".fasta", "wb") as f:
            f.write(fa)
        rows.append("%s\t%s.fasta\t%d" % (name, name, gs.phenotype(i)))
    with open("data.pheno", "w") as f:
        f.write("\n".join(rows) + "\n")
    return gs, rows


@pytest.mark.parametrize("bc,extra", [("DT", []), ("RF", ["--n_iter", "4"])])
def test_f_cli_end_to_end(tmp_path, monkeypatch, bc, extra):
    """(f) PSK_PCA=1, PSK_DT=1 / PSK_RF=1 and PSK_TREE_PCA=1: modeling --pca -bc DT|RF writes the three files; the .pkl loads
    with joblib, its trees split the kept components at thresholds other than 0.5 and reproduce the summary's predictions
    from the float32 scores; prediction writes a line per sample, by the stub reader and by joblib."""
    import csv

    import joblib
    from phenotypeseeker_amd import model_pca
    for knob in ("PSK_" + bc, "PSK_PCA", "PSK_TREE_PCA"):
        monkeypatch.setenv(knob, "1")
    gs, rows = _write_genomes(tmp_path)
    argv = ["modeling", "data.pheno", "-bc", bc, "--pca", "--omit_B_correction", "--pvalue", "0.5", "--n_kmers", "200"] + extra
    _run(tmp_path, argv)
    names = ["summary_of_%s_analysis_Pheno.txt" % bc, "PCs_and_coefficients_in_%s_model_Pheno.txt" % bc, "%s_model_Pheno.pkl" % bc]
    for nm in names:
        assert os.path.exists(nm), nm
    assert not os.path.exists("k-mers_and_coefficients_in_%s_model_Pheno.txt" % bc)
    pkg = joblib.load(names[2])
    assert set(pkg) == {"model", "kmers", "pca", "pred_scale", "scaler", "pca_model", "PCs_to_keep"} and pkg["pca"] is True
    keep = np.asarray(pkg["PCs_to_keep"], dtype=bool)
    be = pkg["model"].best_estimator_
    trees = [e.tree_ for e in be.estimators_] if bc == "RF" else [be.tree_]
    assert all(t.n_features == int(keep.sum()) for t in trees)
    thr = np.concatenate([t.threshold[t.feature >= 0] for t in trees])
    assert len(thr) and np.all(thr != 0.5)
    lines = open(names[1]).read().splitlines()
    assert lines[0] == "PC\tcoef._in_%s_model\texplained_variance\texplained_variance_ratio\tt-test_statistic\tt-test_pvalue" % bc
    assert [ln.split("\t")[0] for ln in lines[1:]] == ["PC_%d" % (c + 1) for c in np.nonzero(keep)[0]]
    assert [ln.split("\t")[1] for ln in lines[1:]] == [str(np.float64(v)) for v in be.feature_importances_]
    with open("Pheno_MLdf.csv") as f:
        ml = list(csv.reader(f))
    cells = np.array([[int(v) for v in r[1:-2]] for r in ml[1:]], dtype=np.float64)
    scores = model_pca.project(pkg["scaler"], pkg["pca_model"], cells, keep).astype(np.float32)
    assert np.array_equal(pkg["model"].predict(scores),
                          [int(ln.split()[2]) for ln in open(names[0]).read().split("Predicted_phenotype\n")[1].split("\n\n")[0].splitlines()])
    with open("samples.txt", "w") as f:
        for line in rows[1:]:
            f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("PSK_JOBLIB_LOAD", flag)
        _run(tmp_path, ["prediction", "samples.txt", "phenos.txt"])
        out = open("predictions_Pheno.txt").read().splitlines()
        assert out[0] == "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class" and len(out) == 1 + gs.n
        for ln, row in zip(out[1:], rows[1:]):
            cols = ln.split("\t")
            assert len(cols) == 3 and cols[0] == row.split()[0] and cols[1] in ("0", "1") and 0.0 <= float(cols[2]) <= 1.0
        outs.append(out)
    assert outs[0] == outs[1]
    monkeypatch.delenv("PSK_TREE_PCA")                          # without the knob: today's refusal
    with pytest.raises(SystemExit) as e:
        _run(tmp_path, argv)
    assert "--pca is not supported with -bc %s." % bc in str(e.value)
