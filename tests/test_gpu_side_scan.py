"""The side-matrix chi2 kernel (chi2_scan_kernel_cx_side: every scan of an exception-coded matrix whose plan skips the
slots) against the dense kernel (PSK_SCAN_DENSE=1), the mixed kernel (PSK_CX_SIDE_KERNEL=0) -- row, stat, p, n_with
bit for bit -- and the restated statistic of helpers.py.  The context is made with PSK_GRID_MULT=1: the grid is 256
workgroups = 1,024 waves, so from 2^16 (two chunks per row) or 2^17 (one chunk) overflow rows on a wave sweeps more than one
batch, whatever the kernel's unroll.

The matrices: overflow rows are random packed words (about half the samples present: far more than 7 exceptions) and
planted rows near the case mask; the rest are slot rows of one exception.  The encoder keeps a copy only when at most an
eighth of the rows overflow and the copy is at most 0.6 of the dense bytes (presence_compact.hip), so a matrix of n_ov
overflow rows has 8 n_ov rows at four words per row and 12.5 n_ov at two -- 200 rows (below SC_NSEG) where that allows it.
The scans use omit_B with cut-off 0.01 (thr 9.21: about 1 % of the random rows survive).  With the flagship's frequency filter
(2, n_valid - 2) that skips the slots for an alternating phenotype; with n1 = 3 a slot row of the three cases reaches any
threshold, so the other two phenotypes take the filter (8, n_valid - 8), which no row of at most 7 exceptions passes."""
import os

import numpy as np
import pytest

from helpers import chi2_reference_keep, chi2_restated, pack_presence

pytestmark = pytest.mark.gpu

FIELDS = ("row", "stat", "p", "n_with")
CUT = 0.01


class knobs:
    """the given PSK_* variables for the block (the library reads them per scan), restored after it"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in ("PSK_SCAN_DENSE", "PSK_CX_SIDE_KERNEL", "PSK_CHI2_MODE")}
        for k in self.saved:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _new_ctx():
    from phenotypeseeker_amd.engine import PskContext
    saved = os.environ.get("PSK_GRID_MULT")
    os.environ["PSK_GRID_MULT"] = "1"
    try:
        return PskContext(0)
    finally:
        os.environ.pop("PSK_GRID_MULT", None)
        if saved is not None:
            os.environ["PSK_GRID_MULT"] = saved


@pytest.fixture(scope="module")
def ctx():
    c = _new_ctx()
    yield c
    c.close()


def _phenotypes(n):
    rng = np.random.default_rng(1000 + n)
    alt = (np.arange(n) % 2 == 0).astype(np.int8)
    na = np.where(rng.random(n) < 0.08, -1, alt).astype(np.int8)
    few = np.zeros(n, np.int8)
    few[[1, n // 2, n - 2]] = 1
    out = []
    for tag, ph in (("alternating", alt), ("na", na), ("n1=3", few)):
        nv = int((ph >= 0).sum())
        out.append((tag, ph, (2, nv - 2) if tag == "alternating" else (8, nv - 8)))
    return out


def _valid_mask(n, wpr):
    return pack_presence(np.ones((1, n), bool))[0][:wpr]


def _matrix(n, n_ov, ph8, seed, planted=300, all_planted=False, m_min=200):
    """(bits [m][wpr], positions of the overflow rows).  Packed words drawn directly."""
    from phenotypeseeker_amd.engine import words_per_row
    rng = np.random.default_rng(seed)
    wpr = words_per_row(n)
    m = max(m_min, int(np.ceil((8 if wpr == 4 else 12.5) * n_ov)))
    bits = np.zeros((m, wpr), np.uint64)
    one = rng.integers(0, n, m)                                   # slot rows: one exception, present or absent
    bits[np.arange(m), one >> 6] = np.uint64(1) << (one & 63).astype(np.uint64)
    flip = rng.random(m) < 0.5
    bits[flip] ^= _valid_mask(n, wpr)
    at = np.sort(rng.choice(m, n_ov, replace=False))
    ov = rng.integers(0, 1 << 63, (n_ov, wpr), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (n_ov, wpr), dtype=np.uint64)
    ov &= _valid_mask(n, wpr)
    k = n_ov if all_planted else min(planted, n_ov // 2)
    if k:
        near = np.tile(pack_presence((ph8 == 1)[None, :])[0][:wpr], (k, 1))
        for _ in range(10 if all_planted else 12):               # flips of single samples (one drawn twice flips back)
            s = rng.integers(0, n, k)
            near[np.arange(k), s >> 6] ^= np.uint64(1) << (s & 63).astype(np.uint64)
        ov[rng.choice(n_ov, k, replace=False)] = near
    bits[at] = ov
    return bits, at


def _scan(ctx, env, ph8, mn, mx, nk, expect_skipped=None):
    with knobs(env):
        res = ctx.get_results(ctx.chi2_scan(ph8, None, mn, mx, CUT, True, nk))
        plan = ctx.last_scan_plan()
    if expect_skipped is not None:
        assert plan == (True, 0, True), (env, plan)
    return res


def _same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f, len(a[f]), len(b[f]))


def _restated(bits, at, ph8, got, mn, mx, what, sample=300):
    """a few hundred overflow rows, survivors first: n_with, the statistic bit for bit, and who is kept"""
    import scipy.stats
    n1, n0 = int((ph8 == 1).sum()), int((ph8 == 0).sum())
    m1, m0 = (pack_presence((ph8 == v)[None, :])[0][:bits.shape[1]] for v in (1, 0))
    rows = np.unique(np.concatenate([got["row"][:sample].astype(np.int64), at[:sample]]))
    a = np.bitwise_count(bits[rows] & m1).sum(axis=1).astype(np.int64)
    c = np.bitwise_count(bits[rows] & m0).sum(axis=1).astype(np.int64)
    stat = chi2_restated(a, n1 - a, c, n0 - c)
    keep = chi2_reference_keep(a + c, n1 + n0 - a - c, scipy.stats.chi2.sf(stat, 2), mn, mx, CUT, True, len(bits))
    rows_got = got["row"].astype(np.int64)          # ascending (psk_get_results)
    found = np.isin(rows, rows_got)
    assert np.array_equal(found, keep), (what, int(found.sum()), int(keep.sum()))
    pos = np.searchsorted(rows_got, rows[found])
    assert np.array_equal(got["stat"][pos], stat[found]), what
    assert np.array_equal(got["n_with"][pos], (a + c)[found]), what


CASES = [(0, 256), (1, 130), (33, 65), ((1 << 16) - 1, 256), ((1 << 16) + 1, 130), ((1 << 17) + 33, 128), (3 * (1 << 17) + 33, 65)]


@pytest.mark.parametrize("n_ov,n", CASES)
def test_side_kernel_equals_dense_mixed_and_restated(ctx, n_ov, n):
    phs = _phenotypes(n)
    bits, at = _matrix(n, n_ov, phs[0][1], seed=n_ov * 7 + n)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, n_ov)
    m = len(bits)
    for tag, ph8, (mn, mx) in phs:
        what = (n_ov, n, tag)
        got = _scan(ctx, {}, ph8, mn, mx, m, expect_skipped=True)
        mixed = _scan(ctx, {"PSK_CX_SIDE_KERNEL": "0"}, ph8, mn, mx, m, expect_skipped=True)
        dense = _scan(ctx, {"PSK_SCAN_DENSE": "1"}, ph8, mn, mx, m)
        _same(got, dense, what)
        _same(got, mixed, what)
        if n_ov >= 1 << 16 and tag != "n1=3":
            assert 0.002 * n_ov < len(got["row"]) < 0.03 * n_ov, (what, len(got["row"]))     # about 1 % of the random rows
        if n_ov:
            assert np.all(np.isin(got["row"].astype(np.int64), at)), what
            _restated(bits, at, ph8, got, mn, mx, what)
        else:
            assert len(got["row"]) == 0


def test_every_overflow_row_survives(ctx):
    """Rows that are the case mask with ten flips: every one of the 2^17 + 33 overflow rows comes back -- a workgroup
    appends every row it visits, so rows_per_block must bound the whole sweep (psk_scan_end: PSK_ERANGE otherwise)."""
    n, n_ov = 256, (1 << 17) + 33
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    bits, at = _matrix(n, n_ov, ph8, seed=5, all_planted=True)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, n_ov)
    got = _scan(ctx, {}, ph8, mn, mx, len(bits), expect_skipped=True)
    assert np.array_equal(got["row"].astype(np.int64), at)
    _same(got, _scan(ctx, {"PSK_SCAN_DENSE": "1"}, ph8, mn, mx, len(bits)), "all survive")


@pytest.fixture(scope="module")
def alternation():
    """one matrix, and the scans A (skipped), B (decoded: omit_B at 0.05 with the usual filter), A' (skipped: other class
    sizes, another threshold), each on a fresh context"""
    n, n_ov = 256, (1 << 16) + 1
    phs = _phenotypes(n)
    bits, at = _matrix(n, n_ov, phs[0][1], seed=77)
    m = len(bits)
    scans = {"A": (phs[0][1], None, phs[0][2][0], phs[0][2][1], CUT, True, m),
             "B": (phs[1][1], None, 2, int((phs[1][1] >= 0).sum()) - 2, 0.05, True, m),
             "A'": (phs[1][1], None, phs[1][2][0], phs[1][2][1], 0.002, True, m)}
    want = {}
    for key, args in scans.items():
        c = _new_ctx()
        try:
            c.set_presence(bits, n)
            want[key] = (c.get_results(c.chi2_scan(*args)), c.last_scan_plan()[2])
        finally:
            c.close()
    assert [want[k][1] for k in ("A", "B", "A'")] == [True, False, True]
    return n, bits, scans, want


def test_alternating_plans_on_one_context(ctx, alternation):
    """A, B, A, A', B on one context -- one call, two in flight, and a repeated scan: the kept plan never serves a scan
    it was not made for"""
    n, bits, scans, want = alternation
    ctx.set_presence(bits, n)
    _same(ctx.get_results(ctx.chi2_scan(*scans["A"])), want["A"][0], "A, one call")
    ctx.chi2_scan_begin(*scans["B"])
    ctx.chi2_scan_begin(*scans["A"])
    _same(ctx.get_results(ctx.scan_end()), want["B"][0], "B, two in flight")
    _same(ctx.get_results(ctx.scan_end()), want["A"][0], "A, two in flight")
    assert ctx.last_scan_plan()[2]
    ctx.chi2_scan(*scans["A'"])
    ctx.rescan_timed(2)
    _same(ctx.get_results(ctx.scan_end()), want["A'"][0], "A', repeated")
    assert ctx.last_scan_plan()[2]
    _same(ctx.get_results(ctx.chi2_scan(*scans["B"])), want["B"][0], "B, one call")
    assert not ctx.last_scan_plan()[2]


def test_new_matrix_on_the_same_context(ctx, alternation):
    """set_presence with another number of overflow rows: the results are the new matrix's"""
    n, bits, scans, want = alternation
    ctx.set_presence(bits, n)
    _same(ctx.get_results(ctx.chi2_scan(*scans["A"])), want["A"][0], "first matrix")
    ph8, _, mn, mx, cut, omit, _ = scans["A"]
    bits2, at2 = _matrix(n, 40_000, ph8, seed=78)
    ctx.set_presence(bits2, n)
    assert ctx.compact_info() == (True, 40_000)
    got = _scan(ctx, {}, ph8, mn, mx, len(bits2), expect_skipped=True)
    _same(got, _scan(ctx, {"PSK_SCAN_DENSE": "1"}, ph8, mn, mx, len(bits2)), "second matrix")
    assert len(got["row"]) > 0 and np.all(np.isin(got["row"].astype(np.int64), at2))
