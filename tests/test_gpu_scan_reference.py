"""The chi2 and Welch scans against the reference's own arithmetic instead of the C oracle: the returns of the reference
function captured in tests/golden/ (chi2_kat.json, welch_kat.json), scipy itself, and a float64 restatement of
conduct_chi_squared_test (modeling.py:759-798) in its operation order (helpers.chi2_restated).  GPU == oracle cannot catch
an error the two share; these tests can.

Every chi2 form: the default route (the exception-coded kernel wherever the matrix has an encoded copy), the dense kernel
(PSK_SCAN_DENSE=1) in MODE 0 and MODE 2, and the weighted kernels over the f32 table, the f64 table (PSK_LUT_F64=1) and
no table (PSK_NO_LUT=1).  Every row shape: 8-byte rows, 2, 4, 8 and 16 words, and more than 1,024 samples (the phenotype
masks are uploaded instead of riding in the kernel arguments)."""
import json
import math
import os

import numpy as np
import pytest
import scipy.stats

from helpers import GOLDEN, chi2_every_table, chi2_reference_keep, pack_presence, round2, scan_knobs

pytestmark = pytest.mark.gpu

# on a matrix with an encoded copy the default route is chi2_scan_kernel_cx; PSK_SCAN_DENSE=1 reaches the dense kernel,
# whose two unit-weight forms PSK_CHI2_MODE picks
UNWEIGHTED_FORMS = ({}, {"PSK_SCAN_DENSE": "1"}, {"PSK_SCAN_DENSE": "1", "PSK_CHI2_MODE": "0"},
                    {"PSK_SCAN_DENSE": "1", "PSK_CHI2_MODE": "2"})
WEIGHTED_FORMS = ({}, {"PSK_LUT_F64": "1"}, {"PSK_NO_LUT": "1"})
# sample counts: n <= 64 (8-byte rows), 65-128, 129-256, 257-512, 513-1024, > 1024
SHAPES = ((6, 64), (65, 128), (129, 256), (257, 512), (513, 1024), (1025, 1100))


def _encodable(n):
    """the sample counts whose matrices the encoder takes (given few enough overflow rows)"""
    return 65 <= n <= 256


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


def _scan(ctx, env, ph8, w, mn, mx, cut, omit, nk):
    with scan_knobs(env):
        return ctx.get_results(ctx.chi2_scan(ph8, w, mn, mx, cut, omit, nk))


def _placement(rng, k, n, interleave):
    """where a case's k samples go among n; the other n - k samples are NA: spread over the row, or the first k"""
    return np.sort(rng.choice(n, k, replace=False)) if interleave else np.arange(k)


def _padded_row(rng, pres_case, pos, n, kind):
    """the case's presence at pos; the NA samples' bits all 0, all 1 or random"""
    row = np.zeros(n, bool) if kind == 0 else np.ones(n, bool) if kind == 1 else rng.random(n) < 0.5
    row[pos] = pres_case
    return row


# ---- A1: the reference function's 311 returns, on the device ----------------------------------------------------------
def test_chi2_kats_every_form_and_shape(ctx):
    """Each case of chi2_kat.json padded with NA samples to a sample count of each shape, as the one non-empty row of a
    matrix of all-absent rows (which every case's min >= 1 rejects) -- at row 0, at row 5 (the second slot of a 16-byte
    pair) or at the last row.  Unit-weight cases in every form (and the weighted forms with all-ones weights), the others
    in the weighted forms.  Kept exactly when the reference returned a row; then round(chi2, 2), "%.2E" % p and n_with are
    the reference's."""
    cases = _golden("chi2_kat.json")["cases"]
    assert len(cases) == 311
    m = 17
    rng = np.random.default_rng(2024)
    n_scans = n_cx = 0
    for i, c in enumerate(cases):
        k = len(c["pheno"])
        unit = all(w == 1 for w in c["weights"])
        for s, (lo, hi) in enumerate(SHAPES):
            if k > hi:
                continue
            n = int(rng.integers(max(lo, k), hi + 1))
            pos = _placement(rng, k, n, (i + s) % 2 == 0)
            kind = (i + 2 * s) % 3
            row = (0, 5, m - 1)[(i + s) % 3]
            pres = np.zeros((m, n), bool)
            pres[row] = _padded_row(rng, np.asarray(c["presence"]) != 0, pos, n, kind)
            ph8 = np.full(n, -1, np.int8)
            ph8[pos] = [-1 if p == "NA" else int(p) for p in c["pheno"]]
            w = np.ones(n) if unit else rng.uniform(0.1, 5.0, n)   # the NA samples' weights must not matter
            w[pos] = c["weights"]
            ctx.set_presence(pack_presence(pres), n)
            encoded = ctx.compact_info()[0]
            assert encoded == _encodable(n), (i, n)
            n_cx += encoded
            forms = [(env, None) for env in UNWEIGHTED_FORMS] if unit else []
            forms += [(env, w) for env in WEIGHTED_FORMS]
            for env, wts in forms:
                res = _scan(ctx, env, ph8, wts, c["min"], c["max"], c["pvalue_cutoff"], c["omit_B"], c["n_kmers"])
                n_scans += 1
                what = (i, n, kind, row, env, wts is not None)
                if c["result"] is None:
                    assert len(res["row"]) == 0, what
                    continue
                assert res["row"].tolist() == [row], what
                assert [round2(res["stat"][0]), "%.2E" % res["p"][0], int(res["n_with"][0])] == c["result"][1:4], what
    assert n_cx > 300 and n_scans > 8000


# ---- A2: the Welch fixtures (scipy's ttest_ind), on the device ----------------------------------------------------------
def _welch_check(res, row, c, n_with, what):
    assert res["row"].tolist() == [row], what
    assert int(res["n_with"][0]) == n_with, what
    t, p, mx, my = (float(res[f][0]) for f in ("stat", "p", "mean_x", "mean_y"))
    assert t == pytest.approx(c["t"], rel=1e-9), what
    assert p == pytest.approx(c["p"], rel=1e-8, abs=1e-300), what
    assert mx == pytest.approx(c["mean_x"], rel=1e-12) and my == pytest.approx(c["mean_y"], rel=1e-12), what
    assert [round2(t), "%.2E" % p, round2(mx), round2(my)] == [round2(c["t"]), "%.2E" % c["p"], round2(c["mean_x"]),
                                                               round2(c["mean_y"])], what


def test_welch_kats_every_shape(ctx):
    """Each case of welch_kat.json padded with NA samples to each shape, through ttest_scan (min 1, max = the case's
    samples, a cut every p is under).  Integer weights through the weighted kernels, and again with unit weights and each
    sample repeated w times: both give the fixture's t, p and means (the frequency-weight identity the fixture was made
    with), at the tolerances of test_oracle_golden.py::test_welch_kats and string-identical where the reference prints."""
    cases = _golden("welch_kat.json")["cases"]
    assert len(cases) == 196
    m = 17
    rng = np.random.default_rng(2025)
    n_scans = 0
    for i, c in enumerate(cases):
        vals0 = np.asarray(c["values"], np.float64)
        pres0 = np.asarray(c["presence"]) != 0
        w0 = np.asarray(c["weights"], np.float64)
        unit = bool(np.all(w0 == 1))
        runs = [(vals0, pres0, None if unit else w0, int(pres0.sum()))]
        if not unit:
            rep = w0.astype(int)
            runs.append((np.repeat(vals0, rep), np.repeat(pres0, rep), None, int(rep[pres0].sum())))
        for r, (vals, pres_case, w, n_with) in enumerate(runs):
            k = len(vals)
            for s, (lo, hi) in enumerate(SHAPES):
                if k > hi:
                    continue
                n = int(rng.integers(max(lo, k), hi + 1))
                pos = _placement(rng, k, n, (i + s + r) % 2 == 0)
                row = (0, 5, m - 1)[(i + s + r) % 3]
                pres = np.zeros((m, n), bool)
                pres[row] = _padded_row(rng, pres_case, pos, n, (i + 2 * s) % 3)
                v = rng.normal(0.0, 1e3, n)            # the NA samples' values and weights must not matter
                v[pos] = vals
                valid = np.zeros(n, np.uint8)
                valid[pos] = 1
                wn = None if w is None else rng.uniform(0.1, 5.0, n)
                if wn is not None:
                    wn[pos] = w
                ctx.set_presence(pack_presence(pres), n)
                with scan_knobs(WEIGHTED_FORMS[(i + s) % 3]):
                    res = ctx.get_results(ctx.ttest_scan(v, valid, wn, 1, k, 1.5, 1))
                n_scans += 1
                _welch_check(res, row, c, n_with, (i, r, n, row))
    assert n_scans > 1500


# ---- B: every 2 x 2 table a scan can see ---------------------------------------------------------------------------------
TABLE_CONFIGS = [(44, 0, 20), (64, 3, 30), (100, 7, 50), (256, 0, 128), (300, 10, 140), (1100, 30, 520)]


def _table_matrix(n, n_na, n1, seed):
    """One row for every table (a, c) of a phenotype with n1 cases, n - n_na - n1 controls and n_na NA samples: the present
    samples of each class sit on a run of a random order of the class, the NA samples' bits are random.  Returns (bits,
    a per row, c per row, int8 phenotype)."""
    rng = np.random.default_rng(seed)
    n0 = n - n_na - n1
    order = rng.permutation(n)
    na, cls1, cls0 = order[:n_na], order[n_na:n_na + n1], order[n_na + n1:]
    ph8 = np.full(n, -1, np.int8)
    ph8[cls1] = 1
    ph8[cls0] = 0
    idx = np.arange((n1 + 1) * (n0 + 1))
    a, c = idx // (n0 + 1), idx % (n0 + 1)
    rows = []
    for lo in range(0, len(idx), 16384):
        aa, cc = a[lo:lo + 16384], c[lo:lo + 16384]
        pres = np.zeros((len(aa), n), bool)
        pres[:, cls1] = (np.arange(n1)[None, :] - rng.integers(0, n1, len(aa))[:, None]) % n1 < aa[:, None]
        pres[:, cls0] = (np.arange(n0)[None, :] - rng.integers(0, n0, len(cc))[:, None]) % n0 < cc[:, None]
        pres[:, na] = rng.random((len(aa), n_na)) < 0.5
        rows.append(pack_presence(pres))
    return np.concatenate(rows), a, c, ph8


def _pad_for_encoder(bits, a, c, n):
    """all-absent rows (e = 0) appended until the encoder takes the matrix: at most 1/8 of the rows overflow, and slots plus
    side matrix take at most 0.6 of the dense bytes"""
    pc = np.bitwise_count(bits).sum(axis=1)
    n_ov = int((np.minimum(pc, n - pc) > 7).sum())
    wpr = bits.shape[1]
    need = max(8 * n_ov, int(math.ceil(n_ov * (wpr * 8 + 4) / (0.6 * wpr * 8 - 8))) + 1, len(bits))
    extra = need - len(bits)
    z = np.zeros(extra, dtype=a.dtype)
    return np.concatenate([bits, np.zeros((extra, wpr), np.uint64)]), np.concatenate([a, z]), np.concatenate([c, z])


def _table_sweeps(n_valid, m):
    """(min, max, cutoff, omit_B, n_kmers): the usual cut with and without omit_B, a cut >= 1 that keeps every table the
    frequency filter passes (with n_wo = 1 and 2 at the max edge), a cut where the Bonferroni division decides, min = max
    = a + c, and min = max at n_wo = 1 (nothing passes) and at n_wo = 2"""
    nw = n_valid // 3
    return [(2, n_valid - 2, 0.05, False, m), (2, n_valid - 2, 0.05, True, m), (1, n_valid, 1.5, True, 1),
            (1, n_valid, 0.5, False, 50), (nw, nw, 1.5, True, 1), (n_valid - 1, n_valid - 1, 1.5, True, 1),
            (n_valid - 2, n_valid - 2, 1.5, True, 1)]


@pytest.mark.parametrize("n,n_na,n1", TABLE_CONFIGS)
def test_every_table_against_scipy(ctx, n, n_na, n1):
    """Every reachable (a, c) at this phenotype, in every form and through a sweep of cuts and filters: survivors = the
    reference's keep set; stat = the float64 restatement bit for bit (unit weights as None and as ones); p within 1e-13 of
    scipy.stats.chi2.sf(stat, 2) (the device's exp(-stat / 2) is not chi2.sf to the last bit: DESIGN.md section 4); the
    printed round(stat, 2) and "%.2E" % p identical.  Cuts set at a table's p (strict <: not kept) and at the next double
    above it (kept), on tables whose device p equals scipy's."""
    n_valid = n - n_na
    n0 = n_valid - n1
    bits, a, c, ph8 = _table_matrix(n, n_na, n1, seed=n * 7 + n_na)
    stat_t, p_t = chi2_every_table(n1, n0)
    # scipy's chisquare itself on some of these tables: the restatement and chi2.sf(stat, 2) are what it returns, bit for bit
    rng = np.random.default_rng(n)
    for ai, ci in zip(rng.integers(0, n1 + 1, 50).tolist(), rng.integers(0, n0 + 1, 50).tolist()):
        A, B, C, D = ai, n1 - ai, ci, n0 - ci
        if A + C == 0 or B + D == 0:
            continue
        e = [(n1 * (A + C)) / float(n_valid), (n1 * (B + D)) / float(n_valid), (n0 * (A + C)) / float(n_valid),
             (n0 * (B + D)) / float(n_valid)]
        r = scipy.stats.chisquare([A, B, C, D], e, 1)
        assert (float(r[0]), float(r[1])) == (stat_t[ai, ci], p_t[ai, ci]), (ai, ci)
    if _encodable(n):
        bits, a, c = _pad_for_encoder(bits, a, c, n)
    m = len(bits)
    ctx.set_presence(bits, n)
    assert ctx.compact_info()[0] == _encodable(n)
    stat_r, p_r, n_w = stat_t[a, c], p_t[a, c], a + c
    n_wo = n_valid - n_w
    forms = [(env, None) for env in UNWEIGHTED_FORMS] + [(env, np.ones(n)) for env in WEIGHTED_FORMS]
    for env, w in forms:
        exact = None   # [(row, p)]: tables whose p in this form is scipy's, one in the usual range and one far out in the tail
        for sw in _table_sweeps(n_valid, m):
            res = _scan(ctx, env, ph8, w, *sw)
            rows = res["row"].astype(np.int64)
            keep = np.nonzero(chi2_reference_keep(n_w, n_wo, p_r, *sw))[0]
            what = (env, w is not None, sw)
            assert np.array_equal(rows, keep), what + (len(rows), len(keep))
            assert np.array_equal(res["n_with"], n_w[rows]), what
            assert np.array_equal(res["stat"], stat_r[rows]), what
            dp = res["p"] != p_r[rows]
            rel = np.abs(res["p"][dp] - p_r[rows][dp]) / p_r[rows][dp]
            assert np.all(rel <= 1e-13), what + ("device p != chi2.sf(stat, 2) on %d of %d tables, at most %.3g relative"
                                                 % (dp.sum(), len(rows), rel.max()),)
            # stat is the restatement's, so round(stat, 2) is; "%.2E" % p can only differ where p does
            assert ["%.2E" % x for x in res["p"][dp]] == ["%.2E" % x for x in p_r[rows][dp]], what
            if sw[2] >= 1 and exact is None:
                same = rows[~dp]
                ps = p_r[same]
                exact = [(int(r), float(p_r[r])) for r in (same[np.argmin(np.abs(np.log(ps / 1e-3)))], same[np.argmin(ps)])]
        assert exact is not None, (env, w is not None)
        for r, pc in exact:
            for cut in (pc, float(np.nextafter(pc, np.inf))):
                res = _scan(ctx, env, ph8, w, 1, n_valid, cut, False, 1)
                keep = np.nonzero(chi2_reference_keep(n_w, n_wo, p_r, 1, n_valid, cut, False, 1))[0]
                assert np.array_equal(res["row"].astype(np.int64), keep), (env, w is not None, cut)
                assert (r in set(keep.tolist())) == (cut > pc), (env, w is not None, r, cut)


# ---- C: Welch against scipy at scale -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [12, 64, 65, 256, 1024, 1100, 2048])
def test_welch_against_scipy(ctx, n):
    """Random and planted rows; unit weights against scipy.stats.ttest_ind(x, y, equal_var=False), integer weights against
    the same on the replicated samples.  t within 1e-12, p within 1e-9 while df <= 1e4 and p >= 1e-300, the printed
    round(t, 2), "%.2E" % p and round(mean, 2) identical, and the kept rows scipy's at cuts away from every row's p."""
    rng = np.random.default_rng(4000 + n)
    m = 160
    vals = np.round(rng.normal(3.0, 1.5, n), 4)
    valid = rng.random(n) > 0.06
    valid[:4] = True
    n_valid = int(valid.sum())
    pres = rng.random((m, n)) < rng.uniform(0.05, 0.95, m)[:, None]
    for r in range(0, m, 2):   # planted: present where the value is high, through noise of every strength
        pres[r] = vals + rng.normal(0, rng.uniform(0.05, 3.0), n) > 3.0 + rng.uniform(-1, 1)
    ctx.set_presence(pack_presence(pres), n)
    for w in (None, rng.integers(1, 5, n).astype(np.float64)):
        res = ctx.get_results(ctx.ttest_scan(vals, valid.astype(np.uint8), w, 2, n_valid - 2, 1.5, 1))
        rep = np.ones(n, int) if w is None else w.astype(int)
        ref = {}
        for r in range(m):
            in_x, in_y = pres[r] & valid, ~pres[r] & valid
            if in_x.sum() < 2 or in_y.sum() < 2:
                continue
            x, y = np.repeat(vals[in_x], rep[in_x]), np.repeat(vals[in_y], rep[in_y])
            tt = scipy.stats.ttest_ind(x, y, equal_var=False)
            if np.isfinite(tt.pvalue):
                # the means as the reference prints them: np.average over the group's samples with their weights
                mx, my = (np.average(vals[g], weights=rep[g].astype(np.float64)) for g in (in_x, in_y))
                ref[r] = (float(tt.statistic), float(tt.pvalue), float(tt.df), mx, my, int(in_x.sum()))
        assert res["row"].tolist() == sorted(ref), (n, w is not None)
        printed, printed_ref = [], []
        for j, r in enumerate(res["row"].tolist()):
            t, p, df, mx, my, nw = ref[r]
            what = (n, w is not None, r)
            assert int(res["n_with"][j]) == nw, what
            # (absolute 1e-12 only where t is near 0: there the difference of the means cancels in scipy and here alike)
            assert res["stat"][j] == pytest.approx(t, rel=1e-12, abs=1e-12), what
            # the means are np.average's: numpy's pairwise sums, bit for bit (values of four decimals put a mean exactly on
            # a two-decimal tie now and then, where an ulp decides the printed digit)
            assert (res["mean_x"][j], res["mean_y"][j]) == (mx, my), what
            if df <= 1e4 and p >= 1e-300:
                assert res["p"][j] == pytest.approx(p, rel=1e-9, abs=0), what + (res["p"][j], p, df)
                printed.append("%.2E" % res["p"][j])
                printed_ref.append("%.2E" % p)
            printed += [round2(res["stat"][j]), round2(res["mean_x"][j]), round2(res["mean_y"][j])]
            printed_ref += [round2(t), round2(mx), round2(my)]
        assert printed == printed_ref, (n, w is not None)
        # cuts between two rows' p-values: the kept rows are the ones scipy's p keeps
        ps = np.sort([v[1] for v in ref.values()])
        n_cuts = 0
        for q in (0.2, 0.5, 0.8):
            j = int(q * (len(ps) - 1))
            if not (ps[j] > 0 and ps[j + 1] > ps[j] * (1 + 1e-6)):
                continue
            cut = math.sqrt(ps[j] * ps[j + 1])
            got = ctx.get_results(ctx.ttest_scan(vals, valid.astype(np.uint8), w, 2, n_valid - 2, cut, 1))
            assert got["row"].tolist() == sorted(r for r, v in ref.items() if v[1] < cut), (n, w is not None, cut)
            n_cuts += 1
        assert n_cuts >= 2
