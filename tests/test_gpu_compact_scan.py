"""The unweighted chi2 scan over the exception-coded copy of the matrix (presence_compact.hip, chi2_scan_kernel_cx)
against the dense kernel (PSK_SCAN_DENSE=1, in a child process): the same survivors, bit for bit (row, stat, p,
n_with); and against the C oracle: the same rows and n_with, stat and p as test_gpu_parity.py compares them.
Also: which matrices are encoded and which are declined."""
import os
import subprocess
import sys

import numpy as np
import pytest

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
    # intersect_db re-encodes what is left
    bits = _core_or_rare(256, 20_000, 9)
    ctx.set_presence(bits, 256)
    assert ctx.compact_info()[0]
    ctx.intersect_db(np.arange(0, 20_000, 3, dtype=np.uint64))
    enc, n_ov = ctx.compact_info()
    assert enc and n_ov > 0
    ph = _phenotypes(256, 9)[0]
    c = ctx.chi2_scan(ph, None, 2, 254, 1.5, True, 10)
    assert c > 0


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
