"""The popcount-filtered side-matrix chi2 kernel (chi2_scan_kernel_cx_side_pc: a side-kernel scan whose popcount plan,
psk_cx_pc_plan, rules out some overflow rows) against the unfiltered side kernel (PSK_CX_PC_FILTER=0) and the dense
kernel (PSK_SCAN_DENSE=1): row, stat, p, n_with bit for bit.  psk_last_scan_filter must say `filtered` exactly when the
plan is a side-kernel plan, the knob is on and fewer rows are feasible than the side matrix has, and rows_feasible must
be numpy's count of the overflow rows whose popcount bit is set.

The context is made with PSK_GRID_MULT=1 (256 workgroups = 1,024 waves); the sizes come from psk_cx_pc_shape: one batch
per wave + 1 makes wave 0 sweep twice, two batches per wave + 33 makes it prefetch across batches.

The matrices: slot rows of one exception, as in test_gpu_side_scan.py; the overflow rows are, by turns along the row
ids, a low band (8 to 20 samples present or absent), random half-present rows and rows near the case mask.  Two cuts,
both with omit_B: 0.01 (threshold 9.21) and 1e-9 (threshold 41.4, which a row of at most 20 present or absent samples of
two equal classes cannot reach: 256 s / (256 - s) = 21.7 at s = 20)."""
import ctypes
import math
import os

import numpy as np
import pytest

from helpers import pack_presence
from test_gpu_side_scan import _new_ctx, _phenotypes, _same, _valid_mask

pytestmark = pytest.mark.gpu

CUT, CUT_B = 0.01, 1e-9
KNOBS = ("PSK_SCAN_DENSE", "PSK_CX_SIDE_KERNEL", "PSK_CX_PC_FILTER", "PSK_CHI2_MODE")


class knobs:
    """the given PSK_* variables for the block (the library reads them per scan), restored after it"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in KNOBS}
        for k in self.saved:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx():
    c = _new_ctx()
    yield c
    c.close()


def _pc_shape(n_ov, cap=256):
    from phenotypeseeker_amd import _lib
    blocks, rpb, batch = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32()
    assert _lib.load().psk_cx_pc_shape(n_ov, cap, ctypes.byref(blocks), ctypes.byref(rpb), ctypes.byref(batch)) == 0
    return blocks.value, rpb.value, batch.value


def _one_batch_per_wave():
    blocks, _, batch = _pc_shape(0)
    return blocks * 4 * batch


def _rows_of_k(rng, n, k, among=None):
    """[len(k)][wpr] rows with exactly k[i] distinct samples set, drawn from `among` (default: all n)"""
    from phenotypeseeker_amd.engine import words_per_row
    among = np.arange(n) if among is None else np.asarray(among)
    q = len(among)
    steps = np.array([s for s in range(1, q) if math.gcd(s, q) == 1])
    start, step = rng.integers(0, q, len(k)), steps[rng.integers(0, len(steps), len(k))]
    out = np.zeros((len(k), words_per_row(n)), np.uint64)
    rows = np.arange(len(k))
    for j in range(int(k.max(initial=0))):              # start + j * step mod q: distinct for j < q, step coprime to q
        s = among[(start + j * step) % q]
        on = j < k
        out[rows[on], s[on] >> 6] |= np.uint64(1) << (s[on] & 63).astype(np.uint64)
    return out


def _overflow_rows(rng, n, n_ov, ph8, kinds=(0, 1, 2)):
    """kind 0: low band, 1: random half-present, 2: the case mask with 12 single-sample flips; by turns along the rows"""
    from phenotypeseeker_amd.engine import words_per_row
    wpr = words_per_row(n)
    valid = _valid_mask(n, wpr)
    kind = np.asarray(kinds)[np.arange(n_ov) % len(kinds)]
    ov = np.zeros((n_ov, wpr), np.uint64)
    i0 = np.nonzero(kind == 0)[0]
    low = _rows_of_k(rng, n, rng.integers(8, 21, len(i0)))
    low[rng.random(len(i0)) < 0.5] ^= valid
    ov[i0] = low
    i1 = np.nonzero(kind == 1)[0]
    ov[i1] = (rng.integers(0, 1 << 63, (len(i1), wpr), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (len(i1), wpr), dtype=np.uint64)) & valid
    i2 = np.nonzero(kind == 2)[0]
    near = np.tile(pack_presence((ph8 == 1)[None, :])[0][:wpr], (len(i2), 1))
    for _ in range(12):                                   # (one sample drawn twice flips back)
        s = rng.integers(0, n, len(i2))
        near[np.arange(len(i2)), s >> 6] ^= np.uint64(1) << (s & 63).astype(np.uint64)
    ov[i2] = near
    return ov


def _matrix(n, ov, seed, m_min=200):
    """(bits [m][wpr], positions of the overflow rows `ov`): the rest are slot rows of one exception"""
    rng = np.random.default_rng(seed)
    n_ov, wpr = ov.shape
    m = max(m_min, int(np.ceil((8 if wpr == 4 else 12.5) * n_ov)))
    bits = np.zeros((m, wpr), np.uint64)
    one = rng.integers(0, n, m)
    bits[np.arange(m), one >> 6] = np.uint64(1) << (one & 63).astype(np.uint64)
    bits[rng.random(m) < 0.5] ^= _valid_mask(n, wpr)
    at = np.sort(rng.choice(m, n_ov, replace=False))
    bits[at] = ov
    return bits, at


def _popcounts(ov):
    return np.bitwise_count(ov).sum(axis=1).astype(np.int64)


def _feasible(ph8, n, mn, mx, cut):
    from phenotypeseeker_amd.engine import cx_pc_plan
    return cx_pc_plan(int((ph8 == 1).sum()), int((ph8 == 0).sum()), n, mn, mx, -2.0 * math.log(cut))


def _scan(ctx, env, ph8, mn, mx, cut, nk):
    with knobs(env):
        res = ctx.get_results(ctx.chi2_scan(ph8, None, mn, mx, cut, True, nk))
        return res, ctx.last_scan_plan(), ctx.last_scan_filter()


def _check_three_ways(ctx, ov, n, ph8, mn, mx, cut, nk, what):
    """default, unfiltered and dense agree bit for bit; the filter report is the rule's.  Returns the default's results"""
    n_ov = len(ov)
    feas = _feasible(ph8, n, mn, mx, cut)
    want_feasible = int(np.isin(_popcounts(ov), sorted(feas)).sum())
    got, plan, filt = _scan(ctx, {}, ph8, mn, mx, cut, nk)
    assert plan == (True, 0, True), (what, plan)                      # a side-kernel plan: no slot class is feasible
    assert filt == (want_feasible < n_ov, want_feasible, n_ov), (what, filt, want_feasible)
    plain, plan, filt = _scan(ctx, {"PSK_CX_PC_FILTER": "0"}, ph8, mn, mx, cut, nk)
    assert plan == (True, 0, True) and filt == (False, n_ov, n_ov), (what, plan, filt)
    dense, plan, filt = _scan(ctx, {"PSK_SCAN_DENSE": "1"}, ph8, mn, mx, cut, nk)
    assert not plan[0] and filt == (False, 0, 0), (what, plan, filt)
    _same(got, dense, what + ("dense",))
    _same(got, plain, what + ("unfiltered",))
    return got, want_feasible


def _cases():
    b1 = _one_batch_per_wave()
    sizes = [0, 1, 33, b1 + 1, 2 * b1 + 33]
    return [(s, 256) for s in sizes] + [(s, 65 if s < 64 else 128) for s in sizes]


@pytest.mark.parametrize("n_ov,n", _cases())
def test_filtered_kernel_equals_unfiltered_and_dense(ctx, n_ov, n):
    phs = _phenotypes(n)
    ov = _overflow_rows(np.random.default_rng(n_ov * 5 + n), n, n_ov, phs[0][1])
    bits, at = _matrix(n, ov, seed=n_ov * 7 + n)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, n_ov)
    seen_filtered = 0
    for tag, ph8, (mn, mx) in phs:
        for cut in (CUT, CUT_B):
            got, n_feas = _check_three_ways(ctx, ov, n, ph8, mn, mx, cut, len(bits), (n_ov, n, tag, cut))
            seen_filtered += n_feas < n_ov
            assert np.all(np.isin(got["row"].astype(np.int64), at))
            if tag == "alternating" and cut == CUT and n_ov > 1000:
                assert 0.001 * n_ov < len(got["row"]) < 0.4 * n_ov      # some of the random rows, the planted ones at most
    if n_ov >= 33:
        assert seen_filtered > 0      # the low band is ruled out by the small cut: the filtered kernel ran


def test_every_row_infeasible(ctx):
    """low-band rows only, the small cut: no popcount of the matrix is feasible, nothing is read and nothing survives"""
    n, n_ov = 256, 1000
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    ov = _overflow_rows(np.random.default_rng(3), n, n_ov, ph8, kinds=(0,))
    bits, at = _matrix(n, ov, seed=4)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, n_ov)
    got, n_feas = _check_three_ways(ctx, ov, n, ph8, mn, mx, CUT_B, len(bits), ("all infeasible",))
    assert n_feas == 0 and len(got["row"]) == 0
    assert ctx.last_scan_plan()[0] is False      # (the last of the three scans was the dense one)


def test_every_row_feasible_runs_unfiltered(ctx):
    """random half-present rows, cut 0.01: every popcount of the matrix is feasible and the plan keeps the unfiltered kernel"""
    n, n_ov = 256, 5000
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    ov = _overflow_rows(np.random.default_rng(5), n, n_ov, ph8, kinds=(1,))
    bits, at = _matrix(n, ov, seed=6)
    ctx.set_presence(bits, n)
    got, n_feas = _check_three_ways(ctx, ov, n, ph8, mn, mx, CUT, len(bits), ("all feasible",))
    assert n_feas == n_ov and len(got["row"]) > 0
    with knobs({}):
        ctx.chi2_scan(ph8, None, mn, mx, CUT, True, len(bits))
        assert ctx.last_scan_filter() == (False, n_ov, n_ov)


def test_rows_at_the_lowest_feasible_popcount_and_one_below(ctx):
    """Pure case rows (a = pc, c = 0) of the lowest feasible popcount L and of L - 1, by turns: every one of the first
    kind survives -- 256 L / (256 - L) is the statistic, 41.89 at L = 36 against the keep rule's 41.45 -- and none of
    the second, which the filter does not read"""
    n, n_ov = 256, 4001
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    feas = _feasible(ph8, n, mn, mx, CUT_B)
    low = min(pc for pc in feas if pc >= 8)
    assert low == 36 and low - 1 not in feas
    k = np.where(np.arange(n_ov) % 2 == 0, low, low - 1)
    ov = _rows_of_k(np.random.default_rng(7), n, k, among=np.nonzero(ph8 == 1)[0])
    assert np.array_equal(_popcounts(ov), k)
    bits, at = _matrix(n, ov, seed=8)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, n_ov)
    got, n_feas = _check_three_ways(ctx, ov, n, ph8, mn, mx, CUT_B, len(bits), ("lowest feasible",))
    assert n_feas == int((k == low).sum())
    assert np.array_equal(got["row"].astype(np.int64), at[k == low])
    assert np.all(got["n_with"] == low)


def test_every_live_row_survives(ctx):
    """One batch per wave + 1 rows, all of them the case mask with ten flips but for a low-band tail that turns the
    filter on: workgroup 0 appends every row of its waves' batches, so rows_per_block must bound the whole sweep
    (psk_scan_end: PSK_ERANGE otherwise; seen once with rows_per_block halved in cx_pc_shape)"""
    n = 128
    n_ov = _one_batch_per_wave() + 1
    blocks, rpb, batch = _pc_shape(n_ov)
    assert rpb == 2 * 4 * batch and blocks == 256
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    rng = np.random.default_rng(9)
    ov = _overflow_rows(rng, n, n_ov, ph8, kinds=(2,))
    tail = 64
    ov[n_ov - 1 - tail:n_ov - 1] = _overflow_rows(rng, n, tail, ph8, kinds=(0,))      # (the last row stays live: wave 0's second batch)
    bits, at = _matrix(n, ov, seed=10)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, n_ov)
    feas = _feasible(ph8, n, mn, mx, CUT)
    live = np.isin(_popcounts(ov), sorted(feas))
    assert live[:n_ov - 1 - tail].all() and live[-1] and not live.all()
    with knobs({}):
        got = ctx.get_results(ctx.chi2_scan(ph8, None, mn, mx, CUT, True, len(bits)))
        assert ctx.last_scan_filter() == (True, int(live.sum()), n_ov)
    keep = np.ones(n_ov, bool)
    keep[n_ov - 1 - tail:n_ov - 1] = False
    assert np.array_equal(got["row"].astype(np.int64), at[keep])      # every near-mask row, none of the tail
    with knobs({"PSK_SCAN_DENSE": "1"}):
        _same(got, ctx.get_results(ctx.chi2_scan(ph8, None, mn, mx, CUT, True, len(bits))), "all live survive")


def test_two_filtered_scans_in_flight_then_a_repeat(ctx):
    """two scans with different bitmaps in flight on one context, then the second repeated: each gets its own bitmap"""
    n, n_ov = 256, 40_000
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    ov = _overflow_rows(np.random.default_rng(11), n, n_ov, ph8)
    bits, at = _matrix(n, ov, seed=12)
    m = len(bits)
    ctx.set_presence(bits, n)
    want, filt = {}, {}
    for cut in (CUT, CUT_B):
        with knobs({"PSK_SCAN_DENSE": "1"}):
            want[cut] = ctx.get_results(ctx.chi2_scan(ph8, None, mn, mx, cut, True, m))
        filt[cut] = (True, int(np.isin(_popcounts(ov), sorted(_feasible(ph8, n, mn, mx, cut))).sum()), n_ov)
    assert filt[CUT][1] != filt[CUT_B][1] and len(want[CUT_B]["row"]) > 0
    with knobs({}):
        ctx.chi2_scan_begin(ph8, None, mn, mx, CUT, True, m)
        assert ctx.last_scan_filter() == filt[CUT]
        ctx.chi2_scan_begin(ph8, None, mn, mx, CUT_B, True, m)
        assert ctx.last_scan_filter() == filt[CUT_B]
        _same(ctx.get_results(ctx.scan_end()), want[CUT], "first in flight")
        _same(ctx.get_results(ctx.scan_end()), want[CUT_B], "second in flight")
        ctx.rescan_timed(2)
        assert ctx.last_scan_filter() == filt[CUT_B]
        _same(ctx.get_results(ctx.scan_end()), want[CUT_B], "repeated")
