"""The index form of the side-matrix chi2 scan (chi2_scan_kernel_cx_side_idx) and the encoder's index of the side matrix
by popcount that it walks (cx_pc_index, read back through psk_cx_pc_index).

The index: a permutation of [0, n_ov) whose popcounts do not decrease, bucket edges = the exclusive prefix of the
popcount histogram.  The form: default knobs against PSK_CX_PC_INDEX=0 (the popcount-filtered kernel) against
PSK_SCAN_DENSE=1, row / stat / p / n_with bit for bit, with psk_last_scan_form asserted per case from the rule restated
here (a filtered side-kernel plan whose feasible rows lie in at most 4 index ranges and number at most n_ov / 8).

The matrices: slot rows of one exception (test_gpu_side_filter._matrix); the overflow rows are T "planted" rows -- pure
case rows of a popcount L just above the lowest one the small cut (1e-9, omit_B) leaves feasible for the alternating
phenotype, so every one of them survives that scan -- shuffled among low-band rows (8 to 20 samples present or absent),
which that cut rules out and the cut 0.01 does not.  So (alternating, 1e-9) runs the index form over exactly T rows,
and the other phenotypes and the cut 0.01 run whatever the rule says, mostly the popcount filter or the plain side kernel.

A bitmap of five ranges cannot be reached through a scan's parameters -- psk_cx_pc_plan leaves at most two intervals of
popcounts (one per end of a's range) and buckets next to each other in the index merge -- so five ranges are the CPU
test's (tests/test_cx_idx_plan_host.py); here the two-interval bitmap of the n1 = 3 phenotype and a share above the
limit run the popcount form with equal results."""
import os

import numpy as np
import pytest

from test_gpu_side_filter import CUT, CUT_B, _feasible, _matrix, _overflow_rows, _popcounts, _rows_of_k
from test_gpu_side_scan import _new_ctx, _phenotypes, _same

pytestmark = pytest.mark.gpu

KNOBS = ("PSK_SCAN_DENSE", "PSK_CX_SIDE_KERNEL", "PSK_CX_PC_FILTER", "PSK_CX_PC_INDEX", "PSK_CHI2_MODE", "PSK_SCAN_WAIT")
INDEX_TILE = 4096       # rows a workgroup of cx_pc_index_kernel places (presence_compact.hip)


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
    c = _new_ctx()      # PSK_GRID_MULT=1: at most 256 workgroups
    yield c
    c.close()


def _threads():
    from phenotypeseeker_amd.engine import cx_idx_shape
    return cx_idx_shape(0, 256)[2]


# ---- the encoder's index -------------------------------------------------------------------------------------------------
def _index_cases():
    rng = np.random.default_rng(250)
    return [("one row", np.array([100])), ("33 rows", rng.integers(8, 249, 33)),
            ("one scatter tile + 1", np.where(rng.random(INDEX_TILE + 1) < 0.9, rng.integers(8, 12, INDEX_TILE + 1), rng.integers(8, 249, INDEX_TILE + 1))),
            ("one popcount: the contended bin", np.full(3 * INDEX_TILE + 5, 9)),
            ("every row another popcount", rng.permutation(np.arange(8, 249)))]


@pytest.mark.parametrize("what,k", _index_cases(), ids=[c[0] for c in _index_cases()])
def test_index_is_a_permutation_grouped_by_popcount(ctx, what, k):
    n = 256
    ov = _rows_of_k(np.random.default_rng(len(k)), n, k)
    bits, at = _matrix(n, ov, seed=len(k) + 1)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, len(k))
    index, start = ctx.cx_pc_index()
    assert np.array_equal(np.sort(index), np.arange(len(k)))
    pcs = _popcounts(ov)[index.astype(np.int64)]          # (side-matrix row j is the j-th overflow row: ascending row ids)
    assert np.all(np.diff(pcs) >= 0)
    want = np.concatenate([[0], np.cumsum(np.bincount(k, minlength=n + 1))])
    assert len(start) == n + 2 and np.array_equal(start.astype(np.int64), want)


def test_index_of_a_narrow_matrix_with_its_popcounts_over_the_valid_samples(ctx):
    n = 100
    k = np.random.default_rng(7).integers(8, n - 7, 700)
    ov = _rows_of_k(np.random.default_rng(8), n, k)
    bits, at = _matrix(n, ov, seed=9)
    ctx.set_presence(bits, n)
    index, start = ctx.cx_pc_index()
    assert np.array_equal(np.sort(index), np.arange(len(k)))
    assert np.all(np.diff(k[index.astype(np.int64)]) >= 0)
    assert np.array_equal(start.astype(np.int64), np.concatenate([[0], np.cumsum(np.bincount(k, minlength=n + 1))]))


# ---- the form against the popcount filter and the dense kernel ------------------------------------------------------------
def _planted(n, t_rows, n_ov, seed):
    """(overflow rows [n_ov][wpr], which of them are planted, L)"""
    rng = np.random.default_rng(seed)
    ph8 = _phenotypes(n)[0][1]
    feas = _feasible(ph8, n, 2, n - 2, CUT_B)
    lo = min(pc for pc in feas if pc >= 8) + 1
    assert lo - 2 not in feas and lo <= int((ph8 == 1).sum())
    ov = _overflow_rows(rng, n, n_ov, ph8, kinds=(0,))
    planted = np.zeros(n_ov, bool)
    planted[rng.choice(n_ov, t_rows, replace=False)] = True
    ov[planted] = _rows_of_k(rng, n, np.full(t_rows, lo), among=np.nonzero(ph8 == 1)[0])
    return ov, planted, lo


def _want_form(ov, n, ph8, mn, mx, cut):
    from phenotypeseeker_amd.engine import cx_idx_plan
    feas = _feasible(ph8, n, mn, mx, cut)
    hist = np.bincount(_popcounts(ov), minlength=n + 1)
    runs, n_runs, rows, chosen = cx_idx_plan(feas, hist, len(ov))
    if rows == len(ov):
        return "cx_side", rows
    return ("cx_side_idx" if chosen else "cx_side_pc"), rows


def _scan(c, env, sa):
    with knobs(env):
        res = c.get_results(c.chi2_scan(*sa))
        return res, c.last_scan_form(), c.last_scan_plan(), c.last_scan_filter()


def _three_ways(c, ov, n, what, forms_seen=None):
    """three phenotypes x two cuts: default = PSK_CX_PC_INDEX=0 = dense, the form as the rule says.  Returns the survivors
    of (alternating, CUT_B)"""
    out = None
    for tag, ph8, (mn, mx) in _phenotypes(n):
        for cut in (CUT, CUT_B):
            sa = (ph8, None, mn, mx, cut, True, c.presence_shape()[0])
            want, rows = _want_form(ov, n, ph8, mn, mx, cut)
            got, form, plan, filt = _scan(c, {}, sa)
            assert plan == (True, 0, True), (what, tag, cut, plan)
            assert form == want, (what, tag, cut, form, want, rows)
            assert filt == (rows < len(ov), rows, len(ov)), (what, tag, cut, filt)
            pc, form, plan, filt = _scan(c, {"PSK_CX_PC_INDEX": "0"}, sa)
            assert form == ("cx_side_pc" if want == "cx_side_idx" else want) and filt == (rows < len(ov), rows, len(ov))
            dense, form, plan, filt = _scan(c, {"PSK_SCAN_DENSE": "1"}, sa)
            assert form == "dense" and not plan[0]
            _same(got, dense, (what, tag, cut, "dense"))
            _same(got, pc, (what, tag, cut, "popcount filter"))
            if forms_seen is not None:
                forms_seen.add(want)
            if tag == "alternating" and cut == CUT_B:
                out = got
    return out


@pytest.mark.parametrize("n", [256, 100])
@pytest.mark.parametrize("t_rows", [0, 1, 63, 64, 65])
def test_index_form_equals_popcount_filter_and_dense(ctx, t_rows, n):
    n_ov = max(8 * t_rows, 64) + 3
    ov, planted, lo = _planted(n, t_rows, n_ov, seed=11 * t_rows + n)
    bits, at = _matrix(n, ov, seed=13 * t_rows + n)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, n_ov)
    seen = set()
    got = _three_ways(ctx, ov, n, (t_rows, n), seen)
    assert "cx_side_idx" in seen                      # (alternating, CUT_B) at least: T rows of n_ov >= 8 T
    assert np.array_equal(got["row"].astype(np.int64), at[planted]) and np.all(got["n_with"] == lo)


def test_shared_segments_and_a_second_pass(ctx):
    """T = 256 x threads + 1: under the default grid cap 257 workgroups, so segment 0 has two; under PSK_GRID_MULT=1 (256
    workgroups at most) workgroup 0 takes the last row in a second pass"""
    from phenotypeseeker_amd.engine import PskContext, cx_idx_shape
    n, thr = 256, _threads()
    t_rows = 256 * thr + 1
    n_ov = 8 * t_rows
    ov, planted, lo = _planted(n, t_rows, n_ov, seed=21)
    bits, at = _matrix(n, ov, seed=22)
    ctx.set_presence(bits, n)
    assert cx_idx_shape(t_rows, 256)[:2] == (256, 2 * thr)
    got = _three_ways(ctx, ov, n, "second pass")
    assert np.array_equal(got["row"].astype(np.int64), at[planted])
    with PskContext(0) as wide:                        # the build's grid multiple: the cap is far above 257
        wide.set_presence(bits, n)
        tag, ph8, (mn, mx) = _phenotypes(n)[0]
        sa = (ph8, None, mn, mx, CUT_B, True, len(bits))
        got2, form, plan, filt = _scan(wide, {}, sa)
        assert form == "cx_side_idx" and filt == (True, t_rows, n_ov)
        _same(got2, got, "shared segments")


def test_every_feasible_row_survives_and_fills_its_segment(ctx):
    """T = 3 x threads planted rows: three workgroups, each appends a full segment (seg_cap = threads, as the shape
    says) and nothing overflows: no PSK_ERANGE from psk_scan_end, every planted row is there"""
    from phenotypeseeker_amd.engine import cx_idx_shape
    n, thr = 256, _threads()
    t_rows = 3 * thr
    blocks, rpb, _, seg_cap = cx_idx_shape(t_rows, 256)
    assert (blocks, rpb, seg_cap) == (3, thr, thr) and blocks * seg_cap == t_rows
    ov, planted, lo = _planted(n, t_rows, 8 * t_rows, seed=31)
    bits, at = _matrix(n, ov, seed=32)
    ctx.set_presence(bits, n)
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    sa = (ph8, None, mn, mx, CUT_B, True, len(bits))
    got, form, plan, filt = _scan(ctx, {}, sa)
    assert form == "cx_side_idx" and filt == (True, t_rows, 8 * t_rows)
    assert np.array_equal(got["row"].astype(np.int64), at[planted])
    _same(got, _scan(ctx, {"PSK_SCAN_DENSE": "1"}, sa)[0], "segments filled")


def test_two_intervals_and_a_share_above_the_limit_run_the_popcount_form(ctx):
    """n1 = 3 at the cut 0.01: the feasible popcounts are an interval at either end (cases present, cases absent), two
    index ranges; and planted rows above an eighth of the side matrix: the rule declines, the popcount filter runs"""
    n = 256
    t_rows = 200
    ov, planted, lo = _planted(n, t_rows, 8 * t_rows - 8, seed=41)      # rows_feasible x 8 > n_ov
    bits, at = _matrix(n, ov, seed=42)
    ctx.set_presence(bits, n)
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    sa = (ph8, None, mn, mx, CUT_B, True, len(bits))
    got, form, plan, filt = _scan(ctx, {}, sa)
    assert form == "cx_side_pc" and filt == (True, t_rows, len(ov))
    _same(got, _scan(ctx, {"PSK_SCAN_DENSE": "1"}, sa)[0], "share above the limit")
    assert np.array_equal(got["row"].astype(np.int64), at[planted])
    tag, few, (mn, mx) = _phenotypes(n)[2]
    feas = sorted(pc for pc in _feasible(few, n, mn, mx, CUT) if 8 <= pc <= n - 8)
    assert tag == "n1=3" and len(feas) and np.any(np.diff(feas) > 1)      # two intervals
    _three_ways(ctx, ov, n, "two intervals")


def _pairs(c, a, b, env_b, n_pairs):
    """n_pairs times: scan a (default knobs), scan b (under env_b) begun while a is in flight; returns the counts"""
    counts = np.zeros((n_pairs, 2), np.int64)
    forms = set()
    c.chi2_scan_begin(*a)
    forms.add(c.last_scan_form())
    for i in range(n_pairs):
        os.environ.update(env_b)
        c.chi2_scan_begin(*b)
        forms.add(c.last_scan_form())
        for k in env_b:
            os.environ.pop(k, None)
        counts[i, 0] = c.scan_end()
        c.chi2_scan_begin(*a)
        counts[i, 1] = c.scan_end()
    last = c.get_results(c.scan_end())
    return counts, forms, last


@pytest.mark.parametrize("other", ["cx_side_pc", "cx"])
def test_two_in_flight_alternating_forms(ctx, other):
    """2,000 pairs of scans, two in flight: the index form alternating with the popcount form (the cut 0.01 of the same
    phenotype: the rule's own choice) or the mixed kernel (PSK_CX_SIDE_KERNEL=0); the counts alternate.  Then the same
    waited for by events (PSK_SCAN_WAIT=0): the stamps' counts are the events'"""
    n, t_rows = 256, 130
    ov, planted, lo = _planted(n, t_rows, 2000, seed=51)
    near = np.flatnonzero(~planted)[::40]               # rows near the case mask: feasible and kept under both cuts
    ov[near] = _overflow_rows(np.random.default_rng(53), n, len(near), _phenotypes(n)[0][1], kinds=(2,))
    weak = np.flatnonzero(~planted)[1::40]              # pure case rows of 12 samples: kept under the cut 0.01 (12.6 against 9.21) only
    ov[weak] = _rows_of_k(np.random.default_rng(55), n, np.full(len(weak), 12), among=np.nonzero(_phenotypes(n)[0][1] == 1)[0])
    bits, at = _matrix(n, ov, seed=54)
    ctx.set_presence(bits, n)
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    a = (ph8, None, mn, mx, CUT_B, True, len(bits))
    b = (ph8, None, mn, mx, CUT, True, len(bits))
    env_b = {} if other == "cx_side_pc" else {"PSK_CX_SIDE_KERNEL": "0"}
    with knobs({"PSK_SCAN_DENSE": "1"}):
        want_a = ctx.get_results(ctx.chi2_scan(*a))
        want_b = ctx.get_results(ctx.chi2_scan(*b))
    na, nb = len(want_a["row"]), len(want_b["row"])
    assert na >= t_rows and nb >= na + len(weak)
    for wait in ("1", "0"):
        with knobs({"PSK_SCAN_WAIT": wait}):
            counts, forms, last = _pairs(ctx, a, b, env_b, 2000)
        assert forms == {"cx_side_idx", other}, forms
        assert np.all(counts[:, 0] == na) and np.all(counts[:, 1] == nb), (wait, counts[:3])
        _same(last, want_a, ("last of the pairs", wait))
