"""CPU tests: the oracle (oracle/) against the fixtures captured from the reference itself
(tests/golden/, generator oracle/gen_golden.py).  This is what pins the oracle."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, load_dataset, read_results_tsv, tokenizer_cases


def test_tokenizer_cases_byte_identical_to_glistmaker(oracle):
    cases = tokenizer_cases()
    assert len(cases) > 100
    for data, k, ref in cases:
        w, f, nt = oracle.count_kmers(data, k)
        if ref is None:
            assert len(w) == 0
        else:
            assert oracle.list_bytes(k, w, f) == ref, (data[:60], k)


@pytest.mark.parametrize("tag", ["ds_omitB", "ds_bonf", "ds_k21"])
def test_dataset_lists_union_mapping(oracle, tag):
    ds = load_dataset(tag)
    k = ds["meta"]["k"]
    lists = {}
    for name in ds["names"]:
        w, f, nt = oracle.count_kmers(ds["files"][name], k)
        img = oracle.list_bytes(k, w, f)
        m = ds["meta"]["lists"][name]
        assert (len(w), nt) == (m["n_unique"], m["n_total"])
        assert hashlib.sha256(img).hexdigest() == m["sha256"], name
        lists[name] = (w, f)
    first = ds["names"][0]
    with open(os.path.join(ds["dir"], "%s_0_%d.list" % (first, k)), "rb") as fh:
        assert fh.read() == oracle.list_bytes(k, *lists[first])
    # glistcompare -u : key set and summed frequencies
    uw, uf = oracle.union_freqs([lists[n] for n in ds["names"]])
    assert np.array_equal(uw, np.load(os.path.join(ds["dir"], "union_words.npy")))
    assert np.array_equal(uf, np.load(os.path.join(ds["dir"], "union_freqs.npy")))
    assert hashlib.sha256(oracle.list_bytes(k, uw, uf)).hexdigest() == ds["meta"]["union_sha256"]
    assert np.array_equal(uw, oracle.union([lists[n][0] for n in ds["names"]]))
    # glistquery -l : text mapping of one sample onto the union
    ms = ds["meta"]["mapped_sample"]
    counts = oracle.map_counts(lists[ms][0], lists[ms][1], uw)
    txt = "".join("%s\t%d\n" % (oracle.word_to_kmer(w, k), c) for w, c in zip(uw, counts))
    assert hashlib.sha256(txt.encode()).hexdigest() == ds["meta"]["mapped_sha256"]


def _oracle_rows(oracle, ds, omit_B, pvalue=0.05):
    k = ds["meta"]["k"]
    names = ds["names"]
    wl = [oracle.count_kmers(ds["files"][n], k)[0] for n in names]
    uw = oracle.union(wl)
    bits = oracle.presence_bits(wl, uw)
    n = len(names)
    res = oracle.chi2_scan(bits, ds["pheno"], np.ones(n), n, 2, n - 2, pvalue, omit_B, len(uw))
    rows = {}
    for r in np.nonzero(res["keep"])[0]:
        pres = [(int(bits[r, i >> 6]) >> (i & 63)) & 1 for i in range(n)]
        with_names = [names[i] for i in range(n) if pres[i] and ds["pheno"][i] != "NA"]
        rows[oracle.word_to_kmer(uw[r], k)] = (repr(oracle.round2(res["stat"][r])), oracle.pstring(res["p"][r]),
                                                str(int(res["n_with"][r])), " ".join(["|"] + with_names), pres)
    return rows


@pytest.mark.parametrize("tag,omit_B", [("ds_omitB", True), ("ds_bonf", False), ("ds_k21", False)])
def test_chi2_results_tsv_matches_reference(oracle, tag, omit_B):
    ds = load_dataset(tag)
    rows = _oracle_rows(oracle, ds, omit_B)
    header, ref = read_results_tsv(os.path.join(ds["dir"], "chi2_results_Pheno.tsv"))
    assert header == ["k-mer", "chi2", "p-value", "num_samples_w_kmer", "samples_with_kmer"]
    assert len(ref) > 50
    assert {r[0] for r in ref} == set(rows)
    for kmer, stat, p, nw, nm in ref:
        assert rows[kmer][:4] == (stat, p, nw, nm), kmer
    # ordering contract (a9): p-value strings ascending lexicographically
    order = oracle.select_order([r[0] for r in ref], [r[2] for r in ref])
    assert [ref[i][2] for i in order] == [r[2] for r in ref]
    # the MLdf.csv presence columns
    import csv
    with open(os.path.join(ds["dir"], "Pheno_MLdf.csv")) as f:
        rd = list(csv.reader(f))
    cols = rd[0][1:-2]
    non_na = [i for i, p in enumerate(ds["pheno"]) if p != "NA"]
    assert [r[0] for r in rd[1:]] == [ds["names"][i] for i in non_na]
    for j, kmer in enumerate(cols):
        assert [int(r[1 + j]) for r in rd[1:]] == [rows[kmer][4][i] for i in non_na]
    assert [int(float(r[-1])) for r in rd[1:]] == [ds["pheno"][i] for i in non_na]


def test_chi2_kats_from_reference_function(oracle):
    with open(os.path.join(GOLDEN, "chi2_kat.json")) as f:
        cases = json.load(f)["cases"]
    kept = 0
    for c in cases:
        assert c["result"] != "ValueError"
        r = oracle.chi2_row(c["presence"], c["pheno"], c["weights"], c["min"], c["max"])
        if r is not None and not oracle.chi2_keep(r[1], c["pvalue_cutoff"], c["omit_B"], c["n_kmers"]):
            r = None
        if c["result"] is None:
            assert r is None, c
            continue
        kept += 1
        assert r is not None, c
        ref = c["result"]
        assert oracle.round2(r[0]) == ref[1]
        assert oracle.pstring(r[1]) == ref[2]
        assert r[2] == ref[3]
    assert kept > 100


def test_welch_kats(oracle):
    with open(os.path.join(GOLDEN, "welch_kat.json")) as f:
        d = json.load(f)
    for c in d["t_sf"]:
        assert oracle.t_two_sided_p(c["t"], c["df"]) == pytest.approx(c["p"], rel=1e-10, abs=1e-300)
    for c in d["cases"]:
        r = oracle.ttest_row(c["presence"], c["values"], c["weights"], 1, len(c["values"]))
        assert r is not None
        t, p, mx, my, nw = r
        assert t == pytest.approx(c["t"], rel=1e-9)
        assert p == pytest.approx(c["p"], rel=1e-8, abs=1e-300)
        assert mx == pytest.approx(c["mean_x"], rel=1e-12)
        assert my == pytest.approx(c["mean_y"], rel=1e-12)
        assert nw == sum(c["presence"])


def test_welch_means_are_np_average(oracle):
    """The means the reference prints are round(np.average(x, weights=x_weights), 2) (modeling.py:735-736): numpy's
    pairwise sums within 8,192-element buffers.  The oracle's, bit for bit, at group sizes on both sides of 8, 128 and 8,192
    (the GPU's equal the oracle's: tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(11)
    for n in (6, 9, 17, 130, 131, 300, 1025, 8200, 17000):
        for wt in (False, True):
            vals = np.round(rng.normal(3.0, 1.5, n), 4)
            valid = rng.random(n) > 0.05
            pres = rng.random(n) < 0.5
            valid[:4] = True
            pres[:4] = [True, True, False, False]   # two samples in each group at least: the row passes the filter
            w = rng.integers(1, 5, n).astype(np.float64) if wt else np.ones(n)
            r = oracle.ttest_row(pres, [float(v) if ok else "NA" for v, ok in zip(vals, valid)], w, 1, n)
            x, y = pres & valid, ~pres & valid
            assert (r[2], r[3]) == (np.average(vals[x], weights=w[x]), np.average(vals[y], weights=w[y])), (n, wt)


def test_gmer_counter_outputs(oracle):
    import base64
    import gzip
    with open(os.path.join(GOLDEN, "gmer_counter.json")) as f:
        d = json.load(f)
    k = d["k"]
    words = [oracle.canonical_word(oracle.kmer_to_word(km), k) for km in d["kmers"]]
    for c in d["cases"]:
        fa = gzip.decompress(base64.b64decode(c["fasta_gz_b64"]))
        counts = oracle.count_dict(fa, k, words)
        lines = c["output"].splitlines()
        assert lines[0].startswith("#") and lines[1].startswith("#")
        body = [l.split("\t") for l in lines[2:]]
        assert [b[0] for b in body] == d["kmers"]
        assert [int(b[2]) for b in body] == counts.tolist()


def test_model_oracle_against_converged_sklearn():
    from oracle import oracle_model as OM
    z = np.load(os.path.join(GOLDEN, "model_kat.npz"))
    for tag in ("1", "2"):
        X, y = z["X" + tag], z["y" + tag]
        cv = int(min(np.bincount(y).min(), 10))
        assert np.array_equal(OM.stratified_kfold(y, cv), z["skf_folds" + tag])
        # C=1000 on the 18-sample, near-separable design 1 is ill-conditioned for plain CDN
        # (0.15 % above liblinear's optimum after 2000 sweeps) -- not used as a pin
        for ci in ((3, 4, 6, 9, 12) if tag == "1" else (0, 4, 6, 9, 12)):
            C = float(z["Cs"][ci])
            w, b = OM.logreg_l1_fit(X, y, C, tol=1e-7, max_sweeps=1500)
            obj = OM.logreg_l1_objective(X, y, w, b, C)
            ref_obj = float(z["logreg_obj" + tag][ci])
            assert obj <= ref_obj * (1 + 1e-6) + 1e-9
            assert obj == pytest.approx(ref_obj, rel=2e-5)
    X2, yc2 = z["X2"], z["yc2"]
    assert np.array_equal(OM.kfold(len(yc2), 10), z["kf_folds2"])
    for ai in (0, 3, 5, 6, 8):
        w, b = OM.lasso_fit(X2, yc2, float(z["alphas"][ai]))
        assert np.allclose(w, z["lasso_coef2"][ai], rtol=1e-7, atol=1e-9)
        assert b == pytest.approx(float(z["lasso_icpt2"][ai]), rel=1e-8)
    gs = OM.grid_search(X2, yc2, [float(a) for a in z["alphas"]], "lasso", 10)
    assert np.allclose(gs["mean_test_score"], z["lasso_gs_mean_score2"], rtol=1e-6, atol=1e-8)
    assert float(z["alphas"][gs["best_index"]]) == float(z["lasso_gs_best_alpha2"])


def test_l2_model_oracle_against_sklearn():
    """`--penalty L2` (set_model, modeling.py:1001-1002, :1015-1019): both objectives are strictly convex, so
    the coefficients themselves are pinned."""
    from oracle import oracle_model as OM
    z = np.load(os.path.join(GOLDEN, "model_kat.npz"))
    g = np.load(os.path.join(GOLDEN, "model_l2_kat.npz"))
    for tag, X, y in (("1", z["X1"], g["yc1"]), ("2", z["X2"], z["yc2"])):
        for ai in (0, 4, 6, 9, 12):
            w, b = OM.ridge_fit(X, y, float(z["alphas"][ai]))
            assert np.allclose(w, g["ridge_coef" + tag][ai], rtol=1e-7, atol=1e-9)
            assert b == pytest.approx(float(g["ridge_icpt" + tag][ai]), rel=1e-8, abs=1e-10)
    gs = OM.grid_search(z["X2"], z["yc2"], [float(a) for a in z["alphas"]], "ridge", 10)
    assert np.allclose(gs["mean_test_score"], g["ridge_gs_mean_score2"], rtol=1e-8, atol=1e-10)
    assert float(z["alphas"][gs["best_index"]]) == float(g["ridge_gs_best_alpha2"])
    for tag in ("1", "2"):
        X, y = z["X" + tag], z["y" + tag]
        for ci in (0, 3, 6, 9, 12):
            C = float(z["Cs"][ci])
            w, b = OM.logreg_l2_fit(X, y, C)
            assert np.allclose(w, g["l2_free_coef" + tag][ci], rtol=1e-6, atol=1e-8), (tag, C)
            assert b == pytest.approx(float(g["l2_free_icpt" + tag][ci]), rel=1e-6, abs=1e-8)
            w, b = OM.logreg_l2_fit(X, y, C, penalise_intercept=True)
            assert np.allclose(w, g["l2_liblinear_coef" + tag][ci], rtol=2e-5, atol=2e-6), (tag, C)
            assert b == pytest.approx(float(g["l2_liblinear_icpt" + tag][ci]), rel=2e-5, abs=2e-6)
    X, y = z["X2"], z["y2"]
    cv = int(min(np.bincount(y).min(), 10))
    gs = OM.grid_search(X, y, [float(c) for c in z["Cs"]], "logreg_l2", cv)
    assert np.allclose(gs["mean_test_score"], g["l2_gs_mean_score2"], atol=1e-12)
    assert float(z["Cs"][gs["best_index"]]) == pytest.approx(float(g["l2_gs_best_C2"]))


def test_l1_logreg_arbiter_pins_the_liblinear_fixture():
    """a10: the exact optimum (active-set Newton, KKT < 1e-12) the GPU solver is held to at 1e-6, against the
    converged scikit-learn / liblinear solutions of model_kat.npz: the same support, coefficient sums per distinct
    column pattern and linear predictor within 3e-6 relative -- liblinear's own stopping rule at tol = 1e-10 leaves it
    1.2e-6 from the optimum at C = 1000 on design 1 (it is the fixture, not the arbiter, that limits this bound: the
    arbiter's KKT residual is < 1e-12 and the HIP solver at tol = 1e-12 agrees with it to 1e-8) --, and the same point
    from a cold start (no hint)."""
    from oracle import oracle_model as OM
    z = np.load(os.path.join(GOLDEN, "model_kat.npz"))
    for tag in ("1", "2"):
        X, y = z["X" + tag], z["y" + tag]
        for ci, C in enumerate(z["Cs"]):
            rw, rb = z["logreg_coef" + tag][ci], float(z["logreg_icpt" + tag][ci])
            a = OM.logreg_l1_arbiter(X, y, float(C), rw, rb)
            assert a["kkt"] < 1e-12 and not a["rank_deficient"], (tag, ci, a["kkt"])
            sums = np.zeros(len(a["w_groups"]))
            np.add.at(sums, a["group"], rw)
            assert np.array_equal(sums != 0, a["w_groups"] != 0)
            # (per coefficient the fixture is up to 9e-6 off on its small entries: its error is absolute, ~1e-6 of the largest)
            assert np.allclose(sums, a["w_groups"], rtol=3e-6, atol=1e-6 * np.abs(a["w_groups"]).max()), (tag, ci)
            assert np.allclose(X @ rw + rb, a["linpred"], rtol=3e-6, atol=1e-12)
            assert a["objective"] <= float(z["logreg_obj" + tag][ci]) * (1 + 1e-15)
            cold = OM.logreg_l1_arbiter(X, y, float(C), np.zeros_like(rw), 0.0)
            assert cold["kkt"] < 1e-12 and np.allclose(cold["w_groups"], a["w_groups"], rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("tag", ["g", "h", "i"])
def test_large_model_fixture_holds_certified_optima(tag):
    """model_large_kat.npz: liblinear's converged fits of the designs that take the Gram-global / four-wave
    solver forms, and beside each the arbiter's point.  Re-checked here from the stored numbers alone, with ONE gradient
    evaluation per fit: the arbiter's point satisfies the KKT conditions of liblinear's objective (modeling.py:1011-1014) to
    1e-10 max(1, C) -- the certificate of optimality of a convex problem, whoever computed the point --, its objective is
    the one stored, and liblinear's own point lies at or above it, within what its tolerance leaves (1e-6 relative up to
    C = 10 where it ran at tol = 1e-8 -- measured 6e-8 --; 1e-3 at C = 100, tol = 1e-6 -- measured 4e-4: liblinear's stopping rule is loose there, which is why
    the GPU tests compare with the certified point and not with liblinear's)."""
    from helpers import large_design
    z = np.load(os.path.join(GOLDEN, "model_large_kat.npz"))
    X, y, fold = large_design(z, tag)
    X = X.astype(np.float64)
    ypm_all = 2.0 * y - 1.0
    assert len(z["fit_C_" + tag]) == 15
    for j, (C, hf) in enumerate(zip(z["fit_C_" + tag], z["fit_held_" + tag])):
        tr = fold != hf
        A = np.hstack([X[tr], np.ones((tr.sum(), 1))])
        ypm = ypm_all[tr]
        th = np.append(z["arb_coef_" + tag][j], z["arb_icpt_" + tag][j])
        zlin = A @ th
        g = -C * (A.T @ (ypm / (1.0 + np.exp(ypm * zlin))))
        grp = z["arb_group_" + tag][j]
        # columns that coincide on the training rows share one gradient entry and one coefficient sum (stored on the first)
        ng = grp.max() + 1
        gth, gg = np.zeros(ng + 1), np.zeros(ng + 1)
        np.add.at(gth, grp, th[:-1])
        gg[grp] = g[:-1]
        gth[ng], gg[ng] = th[-1], g[-1]
        on = gth != 0
        kkt = max(np.abs(gg[on] + np.sign(gth[on])).max() if on.any() else 0.0,
                  np.maximum(np.abs(gg[~on]) - 1.0, 0.0).max() if (~on).any() else 0.0)
        assert kkt < 1e-10 * max(1.0, C), (tag, j, C, hf, kkt)
        obj = np.abs(th).sum() + C * np.logaddexp(0.0, -ypm * zlin).sum()
        assert obj == pytest.approx(float(z["arb_obj_" + tag][j]), rel=1e-13)
        lw, lb = z["lib_coef_" + tag][j], float(z["lib_icpt_" + tag][j])
        lobj = np.abs(lw).sum() + abs(lb) + C * np.logaddexp(0.0, -ypm * (X[tr] @ lw + lb)).sum()
        assert lobj == pytest.approx(float(z["lib_obj_" + tag][j]), rel=1e-13)
        assert obj * (1 - 1e-14) <= lobj <= obj * (1 + (1e-6 if C <= 10 else 1e-3)), (tag, j, C, lobj / obj - 1)
    # the grid search as the reference configures it: three liblinear seeds, the same folds
    sc = z["gs_split_scores_" + tag]
    assert sc.shape[0] == 3 and sc.shape[1] == 13 and np.all((sc >= 0) & (sc <= 1))
