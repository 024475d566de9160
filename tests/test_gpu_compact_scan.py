"""The unweighted chi2 scan over the exception-coded copy of the matrix (presence_compact.hip, chi2_scan_kernel_cx)
against the dense kernel (PSK_SCAN_DENSE=1, in a child process): the same survivors, bit for bit (row, stat, p,
n_with); and against the C oracle: the same rows and n_with, stat and p as test_gpu_parity.py compares them.
Also: which matrices are encoded and which are declined; and, against the dense kernel and the reference restatement
(helpers.chi2_restated, scipy's chi2.sf): the kernel at 2.1 M rows under a capped grid (several grid-stride passes per
wave, the slot / side-matrix split of cx_grid, 0 ... 500 side-matrix rows), at 1 ... 257 rows, and after intersect_db."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import chi2_every_table, chi2_reference_keep, pack_presence, scan_knobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("row", "stat", "p", "n_with")


def _bits_from_presence(pres, wpr):
    m, n = pres.shape
    bits = np.zeros((m, wpr), dtype=np.uint64)
    for i in range(n):
        bits[:, i >> 6] |= pres[:, i].astype(np.uint64) << np.uint64(i & 63)
    return bits


def _core_or_rare(n, m, seed):
    """A matrix shaped like a k-mer union: rows within 0..7 samples of all-absent or all-present (the exact edges e = 0
    and 7, all-present and all-absent among them), about 3 % of rows with 8 or more exceptions (e = 8 exactly included),
    and some rows associated with the phenotype of _phenotypes."""
    rng = np.random.default_rng(seed)
    pres = np.zeros((m, n), dtype=bool)
    e = rng.integers(0, 8, m)
    e[:50] = 0
    e[50:100] = 7
    ovf = rng.random(m) < 0.03
    e[ovf] = rng.integers(8, n // 2 + 1, ovf.sum())
    e[100:150] = 8
    flip = rng.random(m) < 0.4          # the exceptions are the absent samples
    flip[:25] = True                    # all-present rows
    flip[25:50] = False                 # all-absent rows
    for r in range(m):
        if e[r]:
            pres[r, rng.choice(n, e[r], replace=False)] = True
    pres[flip] = ~pres[flip]
    assoc = rng.random(m) < 0.015       # present in most even samples, few odd ones (the phenotype of case 0)
    even = (np.arange(n) % 2) == 0
    pres[assoc] = np.where(even, rng.random((assoc.sum(), n)) < 0.9, rng.random((assoc.sum(), n)) < 0.1)
    from phenotypeseeker_amd.engine import words_per_row
    return _bits_from_presence(pres, words_per_row(n))


def _phenotypes(n, seed):
    rng = np.random.default_rng(seed)
    out = [(np.arange(n) % 2 == 0).astype(np.int8)]                           # no NA
    out.append(np.where(rng.random(n) < 0.08, -1, rng.integers(0, 2, n)).astype(np.int8))   # NA samples
    out.append(np.zeros(n, np.int8))                                          # n1 = 0: every table is NaN (chi2_kat.json)
    return out


def _scan_cases(n, m):
    """(min, max, cutoff, omit_B, n_kmers_global): the usual filter, omit_B, a cutoff >= 1 (every row that passes the
    frequency filter survives), a tiny one, and min / max at their edges"""
    return [(2, n - 2, 0.05, False, m), (2, n - 2, 0.05, True, m), (1, n, 1.5, True, 10), (2, n - 2, 1e-30, True, m),
            (0, n, 0.05, True, m), (n // 2, n // 2, 0.5, True, m), (3, 5, 0.2, True, 100)]


def _run_cases(ctx, n, m, pheno_seed):
    """Every scan case over the current matrix -> {name: array}"""
    out = {}
    for pi, ph in enumerate(_phenotypes(n, pheno_seed)):
        for ci, (mn, mx, cut, omit, nk) in enumerate(_scan_cases(n, m)):
            c = ctx.chi2_scan(ph, None, mn, mx, cut, omit, nk)
            res = ctx.get_results(c)
            for f in FIELDS:
                out["%d_%d_%s" % (pi, ci, f)] = res[f]
    return out


def _matrices():
    """(tag, n, kind, seed): hand-made matrices at 65 ... 256 samples, and synthetic genome sets"""
    return [("hand65", 65, "hand", 1), ("hand128", 128, "hand", 2), ("hand200", 200, "hand", 3), ("hand256", 256, "hand", 4),
            ("genomes200", 200, "genomes", 5), ("genomes256", 256, "genomes", 6)]


def _load(ctx, n, kind, seed):
    if kind == "hand":
        bits = _core_or_rare(n, 20_000, seed)
        ctx.set_presence(bits, n)
        return bits
    from phenotypeseeker_amd.synth import GenomeSet
    gs = GenomeSet(n, 60_000, seed=seed, gene_len=600)
    ctx.begin(13, n)
    for lo in range(0, n, 64):
        ctx.count_kmers_batch(lo, [gs.sample(i)[1] for i in range(lo, min(lo + 64, n))], 8)
    m = ctx.build_presence()
    return ctx.get_rows(np.arange(m, dtype=np.uint64)).reshape(m, -1)


def _dense_results(tmp_path):
    """The same scans in a fresh process whose scans all take the dense kernel"""
    out = str(tmp_path / "dense.npz")
    env = dict(os.environ, PSK_SCAN_DENSE="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=ROOT, env=env, check=True, timeout=900)
    return np.load(out)


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


def test_compact_scan_equals_dense_kernel_and_oracle(ctx, oracle, tmp_path):
    dense = _dense_results(tmp_path)
    for tag, n, kind, seed in _matrices():
        bits = _load(ctx, n, kind, seed)
        m = bits.shape[0]
        enc, n_ov = ctx.compact_info()
        assert enc and 0 < n_ov <= m // 8, (tag, enc, n_ov, m)
        got = _run_cases(ctx, n, m, seed)
        for key, val in got.items():
            assert np.array_equal(val, dense["%s_%s" % (tag, key)]), (tag, key)
        for pi, ph in enumerate(_phenotypes(n, seed)):
            ph_list = [("NA" if v < 0 else int(v)) for v in ph]
            for ci, (mn, mx, cut, omit, nk) in enumerate(_scan_cases(n, m)):
                ref = oracle.chi2_scan(bits, ph_list, np.ones(n), n, mn, mx, cut, omit, nk)
                keep = np.nonzero(ref["keep"])[0]
                assert np.array_equal(got["%d_%d_row" % (pi, ci)], keep.astype(np.uint64)), (tag, pi, ci)
                assert np.array_equal(got["%d_%d_n_with" % (pi, ci)], ref["n_with"][keep]), (tag, pi, ci)
                # (the oracle's exp is the host's: within an ulp of the device's, as in test_gpu_parity.py)
                assert np.allclose(got["%d_%d_stat" % (pi, ci)], ref["stat"][keep], rtol=1e-12, atol=0), (tag, pi, ci)
                assert np.allclose(got["%d_%d_p" % (pi, ci)], ref["p"][keep], rtol=1e-12, atol=0), (tag, pi, ci)
        # a cutoff >= 1 keeps every row that passes the frequency filter, slot rows and overflow rows alike
        assert len(got["0_2_row"]) > n_ov


def test_two_scans_in_flight_and_rescan_on_the_compact_path(ctx):
    n = 256
    bits = _core_or_rare(n, 50_001, 7)     # an odd row count: the last 16-byte load holds one slot
    ctx.set_presence(bits, n)
    assert ctx.compact_info()[0]
    phs = _phenotypes(n, 7)[:2]
    want = []
    for ph in phs:
        c = ctx.chi2_scan(ph, None, 2, n - 2, 0.05, True, 50_001)
        want.append((c, ctx.get_results(c)))
    assert want[0][0] > 0
    ctx.chi2_scan_begin(phs[0], None, 2, n - 2, 0.05, True, 50_001)
    ctx.chi2_scan_begin(phs[1], None, 2, n - 2, 0.05, True, 50_001)
    for i in range(2):
        c = ctx.scan_end()
        got = ctx.get_results(c)
        assert c == want[i][0] and all(np.array_equal(got[f], want[i][1][f]) for f in FIELDS)
    assert ctx.rescan_timed(3) > 0
    got = ctx.get_results(ctx.scan_end())
    assert all(np.array_equal(got[f], want[1][1][f]) for f in FIELDS)
    # a weighted scan of the same matrix takes the dense kernels
    w = np.random.default_rng(1).uniform(0.5, 2.0, n)
    assert ctx.chi2_scan(phs[0], w, 2, n - 2, 0.05, True, 50_001) >= 0


def test_which_matrices_are_encoded(ctx):
    # up to 64 samples a dense row is 8 bytes: never encoded
    ctx.set_presence(_core_or_rare(64, 5000, 8), 64)
    assert ctx.compact_info() == (False, 0)
    # the device-generated matrix of bench.py's beyond-cache leg (its seed, fewer rows): 19 % random-density rows, declined
    ctx.synth_presence(2_000_000, 256, seed=(80 << 48) | 11)
    assert ctx.compact_info() == (False, 0)
    # ... and at 200 and 128 samples
    for n in (200, 128):
        ctx.synth_presence(500_000, n, seed=(80 << 48) | 11)
        assert ctx.compact_info() == (False, 0)
    # a matrix whose rows are mostly random: declined
    rng = np.random.default_rng(3)
    ctx.set_presence(_bits_from_presence(rng.random((4000, 150)) < 0.3, 4), 150)
    assert ctx.compact_info() == (False, 0)
    # intersect_db re-encodes what is left: the survivors are the dense kernel's and the reference's on the kept rows
    bits = _core_or_rare(256, 20_000, 9)
    ctx.set_presence(bits, 256)
    assert ctx.compact_info()[0]
    assert ctx.intersect_db(np.arange(0, 20_000, 3, dtype=np.uint64)) == len(bits[::3])
    enc, n_ov = ctx.compact_info()
    assert enc and n_ov > 0
    for ph in _phenotypes(256, 9)[:2]:
        _compact_dense_and_reference(ctx, bits[::3], ph, _sweeps(ph, len(bits[::3])), "intersect")
    # an intersection that keeps no row: no copy, an empty scan
    assert ctx.intersect_db(np.array([1 << 40], dtype=np.uint64)) == 0
    assert ctx.compact_info() == (False, 0)
    assert ctx.chi2_scan(_phenotypes(256, 9)[0], None, 1, 256, 1.5, True, 10) == 0
    # a declined matrix (half its rows random) that the intersection turns into an encoded one (its core-or-rare rows)
    core = _core_or_rare(256, 6000, 10)
    mixed = np.empty((12_000, 4), np.uint64)
    mixed[0::2] = core
    mixed[1::2] = _bits_from_presence(rng.random((6000, 256)) < 0.3, 4)
    ctx.set_presence(mixed, 256)
    assert ctx.compact_info() == (False, 0)
    assert ctx.intersect_db(np.arange(0, 12_000, 2, dtype=np.uint64)) == 6000
    assert ctx.compact_info()[0]
    for ph in _phenotypes(256, 10)[:2]:
        _compact_dense_and_reference(ctx, core, ph, _sweeps(ph, 6000), "declined then encoded")


# ---- the exception-coded kernel against the dense kernel and the reference restatement, at scale and at the edges ----------
def _scan(ctx, env, ph8, mn, mx, cut, omit, nk):
    with scan_knobs(env):
        return ctx.get_results(ctx.chi2_scan(ph8, None, mn, mx, cut, omit, nk))


def _sweeps(ph8, m):
    """the usual cut with omit_B, and a cut >= 1: every row the frequency filter passes survives"""
    n_valid = int((ph8 >= 0).sum())
    return [(2, n_valid - 2, 0.05, True, m), (1, n_valid, 1.5, True, 1)]


def _compact_dense_and_reference(ctx, bits, ph8, sweeps, what):
    """Each sweep on the encoded copy (asserted) and on the dense kernel: the same survivors bit for bit, and the
    reference's -- keep set, the restated statistic bit for bit, p within 1e-13 of chi2.sf.  Returns the survivor counts."""
    assert ctx.compact_info()[0], what
    n1, n0 = int((ph8 == 1).sum()), int((ph8 == 0).sum())
    m1, m0 = (pack_presence((ph8 == v)[None, :])[0] for v in (1, 0))
    a = np.bitwise_count(bits & m1).sum(axis=1).astype(np.int64)
    c = np.bitwise_count(bits & m0).sum(axis=1).astype(np.int64)
    stat_t, p_t = chi2_every_table(n1, n0)
    counts = []
    for sw in sweeps:
        got = _scan(ctx, {}, ph8, *sw)
        dense = _scan(ctx, {"PSK_SCAN_DENSE": "1"}, ph8, *sw)
        for f in FIELDS:
            assert np.array_equal(got[f], dense[f]), (what, sw, f)
        keep = np.nonzero(chi2_reference_keep(a + c, n1 + n0 - a - c, p_t[a, c], *sw))[0]
        rows = got["row"].astype(np.int64)
        assert np.array_equal(rows, keep), (what, sw, len(rows), len(keep))
        assert np.array_equal(got["n_with"], (a + c)[rows]), (what, sw)
        assert np.array_equal(got["stat"], stat_t[a[rows], c[rows]]), (what, sw)
        p_ref = p_t[a[rows], c[rows]]
        assert np.all(np.abs(got["p"] - p_ref) <= 1e-13 * p_ref), (what, sw)
        counts.append(len(rows))
    return counts


def _slot_rows(rng, m, n):
    """m rows of 1 ... 7 exceptions (an index drawn twice counts once), present or absent samples alike"""
    from phenotypeseeker_amd.engine import words_per_row
    e = rng.integers(1, 8, m)
    idx = rng.integers(0, n, (m, 7))
    bits = np.zeros((m, words_per_row(n)), np.uint64)
    for j in range(7):
        on = j < e
        for wd in range(bits.shape[1]):
            sel = on & (idx[:, j] >> 6 == wd)
            bits[sel, wd] |= np.uint64(1) << (idx[sel, j] & 63).astype(np.uint64)
    flip = rng.random(m) < 0.5
    bits[flip] ^= pack_presence(np.ones((1, n), bool))[0]
    return bits


def _ov_rows(rng, k, ph8):
    """k rows of many exceptions (the side matrix), associated with the phenotype: present in most cases, few controls"""
    return pack_presence(np.where(ph8 == 1, rng.random((k, len(ph8))) < 0.8, rng.random((k, len(ph8))) < 0.2))


@pytest.fixture(scope="module")
def big_matrix():
    """2.1 M slot rows at 256 samples, 500 side-matrix rows, a phenotype with NA samples"""
    rng = np.random.default_rng(21)
    n = 256
    ph8 = np.where(rng.random(n) < 0.04, -1, np.arange(n) % 2 == 0).astype(np.int8)
    return n, _slot_rows(rng, 2_100_000, n), _ov_rows(rng, 500, ph8), ph8


@pytest.mark.parametrize("grid_mult", [1, 2])
def test_compact_scan_grid_stride_passes_and_split(big_matrix, grid_mult):
    """A context whose scan grid is capped at 1 or 2 workgroups per CU (PSK_GRID_MULT, read by psk_init): each wave makes
    several passes of its grid-stride loop, and cx_grid splits the capped grid between slots and side matrix in proportion
    to their bytes -- with 1, 64, 65 side-matrix rows the side matrix gets the one workgroup of the n_ov && bo == 0
    branch; with none, no workgroup.  A cut >= 1 keeps nearly every row: no result segment may overflow (PSK_ERANGE)."""
    from phenotypeseeker_amd.engine import PskContext
    n, base, ov, ph8 = big_matrix
    saved = os.environ.get("PSK_GRID_MULT")
    os.environ["PSK_GRID_MULT"] = str(grid_mult)
    try:
        ctx = PskContext(0)
    finally:
        os.environ.pop("PSK_GRID_MULT", None)
        if saved is not None:
            os.environ["PSK_GRID_MULT"] = saved
    try:
        for k in ((0, 1, 64, 65, 500) if grid_mult == 1 else (500,)):
            rng = np.random.default_rng(k)
            m = len(base) + k
            at = np.zeros(m, bool)
            at[rng.choice(m, k, replace=False)] = True
            bits = np.empty((m, base.shape[1]), np.uint64)
            bits[~at] = base
            bits[at] = ov[:k]
            ctx.set_presence(bits, n)
            assert ctx.compact_info() == (True, k)
            counts = _compact_dense_and_reference(ctx, bits, ph8, _sweeps(ph8, m), ("grid_mult", grid_mult, k))
            assert counts[1] > 0.75 * m
    finally:
        ctx.close()


@pytest.mark.parametrize("m", [1, 2, 3, 255, 256, 257])
def test_compact_scan_small_row_counts(ctx, m):
    """Row counts around one slot pair and one wave step, on the encoded path (no side matrix)"""
    for n in (100, 200):
        rng = np.random.default_rng(m * 1000 + n)
        ph8 = np.where(rng.random(n) < 0.05, -1, rng.random(n) < 0.5).astype(np.int8)
        bits = _slot_rows(rng, m, n)
        ctx.set_presence(bits, n)
        assert ctx.compact_info() == (True, 0)
        _compact_dense_and_reference(ctx, bits, ph8, _sweeps(ph8, m) + [(0, n, 0.9, False, 1)], ("rows", m, n))


if __name__ == "__main__":      # the dense side of test_compact_scan_equals_dense_kernel_and_oracle (PSK_SCAN_DENSE=1)
    sys.path.insert(0, ROOT)
    from phenotypeseeker_amd.engine import PskContext
    res = {}
    with PskContext(0) as c:
        for tag, n, kind, seed in _matrices():
            bits = _load(c, n, kind, seed)
            for key, val in _run_cases(c, n, bits.shape[0], seed).items():
                res["%s_%s" % (tag, key)] = val
    np.savez(sys.argv[1], **res)
