"""CPU tests of what tests/test_gpu_l1_float.py rests on (tests/l1_float_cases.py): the placement table against the constants
of csrc/solver_l1_plan.h and solver_common.h, the arbiter's certificate of every logistic fit from the zero hint, the stop
rule at the certified optimum, and the NumPy elastic-net descent with its KKT certificate.  A case that fails here has no
place in the GPU tests."""
import time

import numpy as np
import pytest

import l1_float_cases as L

np.seterr(over="ignore")        # exp() of a large margin overflows to inf on purpose: 1 / (1 + inf) = 0


def test_every_case_lands_in_the_placement_its_table_row_names():
    """placement() and the Lasso's use_lds rule, computed from the values the headers spell out, put every case where CASES
    says; all four placements and both use_lds values occur; the edge shapes are the last / first of their placements.  A
    change of PSK_L1_LDS_MAX, psk_l1_feature_bytes or SV_LDS_N fails here instead of silently uncovering a placement."""
    H = L.header_constants()
    assert H["host_rules"], "psk_logreg_l1_fit / lasso_float_fit no longer spell the rules that l1_float_cases restates"
    assert H["lds_max"] == L.L1_LDS_MAX == 155648 and H["SV_LDS_N"] == L.SV_LDS_N
    assert all(H["feature_bytes"](p) == 40 * (p + 1) for p in (0, 1, 40, 3892))
    seen = set()
    for name, c in L.CASES.items():
        got = L.placement(c["n"], c["p"], H["lds_max"], H["feature_bytes"])
        assert L.route_is_float(name) == (c["place"] is not None), name
        if c["place"] is not None:
            assert got == c["place"] == L.placement(c["n"], c["p"]), (name, got)
            if name in L.TABLE:
                seen.add(got)
    assert seen == {(1, 1), (0, 1), (1, 0), (0, 0)}
    a, b = L.CASES["A-edge"], L.CASES["B-edge"]
    assert (a["n"], a["p"] + 1) == (b["n"], b["p"]) and a["n"] + a["p"] + 1 == 3891
    assert np.array_equal(L.case_data("A-edge")[0], L.case_data("B-edge")[0][:, :a["p"]])
    # one sample fewer and the sample arrays of C and D are back in LDS
    for name in ("C", "D"):
        c = L.CASES[name]
        assert L.placement(c["n"] - 1, c["p"])[1] == 1 and c["place"][1] == 0, name
    assert L.CASES["C-bin"]["n"] == L.BITS_MAX_N + 1 and L.CASES["C-bin-4096"]["n"] == L.BITS_MAX_N
    assert np.array_equal(L.case_data("C-bin")[0][:4096], L.case_data("C-bin-4096")[0])
    assert {(c["n"], L.lasso_use_lds(c["n"], H["SV_LDS_N"])) for c in L.LASSO_CASES.values()} == {(8192, 1), (8193, 0)}
    assert all(L.lasso_use_lds(c["n"], H["SV_LDS_N"]) == c["use_lds"] for c in L.LASSO_CASES.values())
    assert 8192 * 8 == 64 * 1024        # n = 8192: dynamic LDS is exactly the 64 KiB that need no attribute


def test_the_designs_are_what_the_cases_say():
    for name, c in L.CASES.items():
        X, y, fold, fp, ff = L.case_data(name)
        assert X.dtype == np.float32 and np.all(np.isfinite(X)) and X.min() == 0.0
        assert bool(np.any((X != 0) & (X != 1))) == c["counts"], name
        if c["counts"]:
            assert X.max() == 200.0 and (X == 200.0).sum() >= 4
        if c["p"] > 9 and "widen" not in c:
            assert np.all(X[:, L.CONST_COL] == 1) and not X[:, L.ZERO_COL].any() and np.array_equal(X[:, L.DUP_COL], X[:, -1])
        for h in set(ff.tolist()):
            tr = fold != h
            assert 0 < y[tr].sum() < tr.sum(), (name, h)                        # both classes in every training set
            assert not c["counts"] or np.any((X[tr] != 0) & (X[tr] != 1))       # non-binary without the held-out rows too
    assert len(L.case_data("E")[3]) == 120 and len(L.case_data("D")[3]) == 2 and len(L.case_data("A")[3]) == 30


@pytest.mark.parametrize("name", [n for n in L.CASES])
def test_the_arbiter_certifies_every_fit_from_the_zero_hint(name):
    """kkt < 1e-10 from w_hint = 0, b_hint = 0; a support of 3..80 patterns (the intercept, with which the constant column is
    folded, counting as one; a tail shape offers at most p + 1); no rank deficiency.  Then liblinear's stop rule accepts the
    certified optimum and rejects w = 0."""
    X, y, fold, fp, ff = L.case_data(name)
    t0 = time.perf_counter()
    arbs = L.certified(name)
    secs = time.perf_counter() - t0
    ypm = 2.0 * y - 1.0
    sizes = []
    for j, a in enumerate(arbs):
        tr = fold != ff[j]
        Xt = X[tr].astype(np.float64)
        assert a["kkt"] < L.KKT_MAX, (name, j, a["kkt"])
        assert not a["rank_deficient"], (name, j)       # the arbiter never holds the constant column AND the intercept
        g = L.const_group(Xt, a)
        assert g is None or a["w_groups"][g] == 0.0 or a["b"] == 0.0, (name, j)
        k = L.support_size(Xt, a)
        sizes.append(k)
        assert min(L.SUPPORT_MIN, X.shape[1] + 1) <= k <= L.SUPPORT_MAX, (name, j, float(fp[j]), int(ff[j]), k)
        w = L.expand(a, X.shape[1])
        assert np.allclose(Xt @ w + a["b"], a["linpred"], rtol=1e-12, atol=1e-12)
        opt = (w[None, :], np.array([a["b"]]), [0])
        L.stop_rule_holds(X, ypm, fold, fp[j:j + 1], ff[j:j + 1], *opt, [0], tol=1e-12, slack=1.0)
        with pytest.raises(AssertionError):
            L.stop_rule_holds(X, ypm, fold, fp[j:j + 1], ff[j:j + 1], 0 * opt[0], 0 * opt[1], [0], [0], tol=1e-4)
        assert L.objectives(X, ypm, fold, fp[j:j + 1], ff[j:j + 1], *opt[:2])[0] == pytest.approx(a["objective"], rel=1e-13)
    print("%s: %d fits, support %d..%d patterns, largest kkt %.1e, %.2f s" % (name, len(arbs), min(sizes), max(sizes),
                                                                              max(a["kkt"] for a in arbs), secs))
    if name == "D":
        assert secs < 20.0      # one Newton solve per coordinate added: the cap on the support is what keeps this short


@pytest.mark.parametrize("name", ["A", "C"])
def test_held_out_rows_do_not_reach_the_arbiter(name):
    """Overwriting a fold's rows with counts up to 1e6 and flipping its labels leaves the training rows, and so the arbiter's
    answer for that fold's fits, unchanged."""
    from oracle import oracle_model as OM
    X, y, fold, fp, ff = L.case_data(name)
    held = 1
    X2, y2 = L.garbage(X, y, fold, held)
    tr = fold != held
    assert X2[~tr].max() == 1e6 and np.all(np.isfinite(X2)) and np.array_equal(y2[~tr], 1 - y[~tr])
    assert np.array_equal(X2[tr], X[tr]) and np.array_equal(y2[tr], y[tr]) and not np.array_equal(X2[~tr], X[~tr])
    j = int(np.nonzero(ff == held)[0][0])
    a = OM.logreg_l1_arbiter(X2[tr], y2[tr], float(fp[j]), np.zeros(X.shape[1]), 0.0, max_rounds=L.ARBITER_ROUNDS)
    b = L.certified(name)[j]
    assert np.array_equal(a["w_groups"], b["w_groups"]) and a["b"] == b["b"] and a["objective"] == b["objective"]


@pytest.mark.parametrize("name", list(L.LASSO_CASES))
@pytest.mark.parametrize("l1_ratio", [1.0, 0.5])
def test_the_numpy_descent_is_certified_and_agrees_with_the_oracle(name, l1_ratio):
    """enet_descent ends with the KKT conditions of enet_certificate on every fit; for l1_ratio = 1 the oracle's own Lasso
    (orc_lasso_fit, a second opinion) ends within 1e-9 of it; some fit of the case leaves a coefficient at zero or the test of
    the support says nothing."""
    from oracle import oracle_model as OM
    X, y, fold, fa, ff = L.lasso_data(name)
    refs = L.lasso_certified(name, l1_ratio)        # (asserts the certificate of each)
    worst = [0.0, 0.0, 0.0]
    for (w, b), alpha, h in zip(refs, fa, ff):
        tr = fold != h
        worst = [max(u, v) for u, v in zip(worst, L.enet_certificate(X[tr], y[tr], w, float(alpha), l1_ratio))]
        if l1_ratio == 1.0:
            w2, b2 = OM.lasso_fit(X[tr], y[tr], float(alpha))
            assert np.abs(w2 - w).max() <= 1e-9 * max(np.abs(w).max(), 1.0) and b2 == pytest.approx(b, rel=1e-9, abs=1e-9)
    print("%s l1_ratio=%g: |g|/l1 off the support %.12f, defect on it %.2e, gap / y'y %.2e" % ((name, l1_ratio) + tuple(worst)))
    sizes = [(w != 0).sum() for w, _ in refs]
    assert min(sizes) < X.shape[1] and max(sizes) > 0
    # a wrong answer is refused: a coefficient moved by 1e-6 of the largest breaks the certificate
    w = refs[0][0].copy()
    w[np.argmax(np.abs(w))] *= 1 + 1e-6
    with pytest.raises(AssertionError):
        L.enet_certificate(X[fold != ff[0]], y[fold != ff[0]], w, float(fa[0]), l1_ratio)


def test_garbage_for_a_continuous_target():
    X, y, fold, fa, ff = L.lasso_data("8193x6 counts")
    X2, y2 = L.garbage(X, y, fold, 1)
    tr = fold != 1
    assert np.array_equal(X2[tr], X[tr]) and np.array_equal(y2[tr], y[tr]) and np.all(np.abs(y2[~tr]) > 1e5) and np.all(np.isfinite(y2))
