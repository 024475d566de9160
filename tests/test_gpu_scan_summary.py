"""A stamped chi2 scan of at most 64 workgroups (the index form's launches: the flagship's has 28) is ended by ONE line of
pinned memory: the scan's last publisher -- found by a ticket that every segment's publisher draws with its count,
csrc/scan_stamps.h -- writes the end clock and n_pass beside the start clock, psk_scan_end polls that line alone
(PSK_SCAN_SUMMARY=1, the default), and the 256 per-segment count words are read by the first result call, or never.
PSK_SCAN_SUMMARY=0 waits for the count words as well and sums them on the host; PSK_SCAN_WAIT=0 is the event pair.  A larger
launch stamps a clock beside every count and is waited for word by word, as every launch was before.

The three must hand out the same scan bit for bit -- n_pass and every field of psk_get_results -- on every single-kernel
form (the index form, cx_side_pc, cx_side, cx, the dense kernel in MODE 0 and MODE 2), at grids of 1, 2, 64, 65, 256 and 257
workgroups; a summary of another scan must never be taken for this scan's (20,000 begin / end pairs, two in flight, over
four forms and two phenotypes whose counts differ: the ticket line is re-armed by every fourth scan, between launches that
never touch it); per-segment counts of another scan must never be handed out (two in flight, both orders, the result call
before and after a third scan takes the set); and the scans that keep their events (weighted, Welch) go on working between
and behind summary scans.

The matrices are test_gpu_side_index.py's: slot rows of one exception, T planted overflow rows that all survive
(alternating phenotype, cut 1e-9) among low-band rows.  A segment overflow cannot be reached through a scan's parameters
(a segment's capacity is the rows its workgroups can visit), so the summary's overflow flag and the eager read behind it are
covered by the CPU test alone (tests/scan_summary_check.cpp)."""
import math
import os
import time

import numpy as np
import pytest

from test_gpu_side_filter import CUT, CUT_B, _matrix, _overflow_rows, _rows_of_k
from test_gpu_side_index import _planted, _threads, _want_form
from test_gpu_side_scan import _new_ctx, _phenotypes

pytestmark = pytest.mark.gpu

KNOBS = ("PSK_SCAN_SUMMARY", "PSK_SCAN_WAIT", "PSK_SCAN_DENSE", "PSK_CX_SIDE_KERNEL", "PSK_CX_PC_FILTER", "PSK_CX_PC_INDEX", "PSK_CHI2_MODE")
FIELDS = ("row", "word", "stat", "p", "mean_x", "mean_y", "n_with")
# (tag, knobs, the form psk_last_scan_form reports given the form the rule picks under default knobs)
FORMS = [("index", {}, lambda w: w),
         ("cx_side_pc", {"PSK_CX_PC_INDEX": "0"}, lambda w: "cx_side_pc" if w == "cx_side_idx" else w),
         ("cx_side", {"PSK_CX_PC_FILTER": "0"}, lambda w: "cx_side"),
         ("cx", {"PSK_CX_SIDE_KERNEL": "0"}, lambda w: "cx"),
         ("dense mode 0", {"PSK_SCAN_DENSE": "1", "PSK_CHI2_MODE": "0"}, lambda w: "dense"),
         ("dense mode 2", {"PSK_SCAN_DENSE": "1", "PSK_CHI2_MODE": "2"}, lambda w: "dense")]
WAYS = [("summary", {"PSK_SCAN_SUMMARY": "1"}), ("counts", {"PSK_SCAN_SUMMARY": "0"}), ("events", {"PSK_SCAN_WAIT": "0"})]


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


def _same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f, len(a[f]), len(b[f]))


def _scan(c, env, sa):
    """one blocking scan under the knobs -> (n_pass, results, form, reported ms, wall-clock s of the scan call)"""
    with knobs(env):
        t0 = time.perf_counter()
        npass = c.chi2_scan(*sa)
        wall = time.perf_counter() - t0
        return npass, c.get_results(npass), c.last_scan_form(), c.last_scan_ms(), wall


def _check_ms(ms, wall_s, what):
    assert math.isfinite(ms) and ms > 0, (what, ms)
    assert ms <= wall_s * 1e3, "%s: %.3f us reported, the call took %.1f us" % (what, ms * 1e3, wall_s * 1e6)


def _mixed_matrix(n, seed):
    """test_gpu_side_index.py's two-in-flight matrix: 130 planted rows among 2,000 overflow rows, with rows near the case
    mask (kept under both cuts) and pure case rows of 12 samples (kept under the cut 0.01 only)"""
    t_rows = 130
    ov, planted, lo = _planted(n, t_rows, 2000, seed=seed)
    ph8 = _phenotypes(n)[0][1]
    near = np.flatnonzero(~planted)[::40]
    ov[near] = _overflow_rows(np.random.default_rng(seed + 2), n, len(near), ph8, kinds=(2,))
    weak = np.flatnonzero(~planted)[1::40]
    ov[weak] = _rows_of_k(np.random.default_rng(seed + 4), n, np.full(len(weak), 12), among=np.nonzero(ph8 == 1)[0])
    bits, at = _matrix(n, ov, seed=seed + 3)
    return bits, ov, t_rows


@pytest.fixture(scope="module")
def mixed256():
    return _mixed_matrix(256, 310)


# ---- summary = counts = events, bit for bit, on every form -----------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 100])
def test_summary_counts_and_events_hand_out_the_same_scan_on_every_form(ctx, mixed256, n):
    bits, ov, t_rows = mixed256 if n == 256 else _mixed_matrix(n, 311)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, len(ov))
    survivors, forms_seen = 0, set()
    for tag, ph8, (mn, mx) in _phenotypes(n):          # alternating, the same with NA samples, n1 = 3
        for cut in (CUT, CUT_B):
            sa = (ph8, None, mn, mx, cut, True, len(bits))
            want_form = _want_form(ov, n, ph8, mn, mx, cut)[0]
            first = None
            for form, env, reported in FORMS:
                got = {}
                for way, env_w in WAYS:
                    what = (n, tag, cut, form, way)
                    got[way] = _scan(ctx, dict(env, **env_w), sa)
                    assert got[way][2] == reported(want_form), (what, got[way][2], want_form)
                    _check_ms(got[way][3], got[way][4], what)
                n_pass = got["events"][0]
                assert got["summary"][0] == got["counts"][0] == n_pass == len(got["events"][1]["row"]), (n, tag, cut, form, [g[0] for g in got.values()])
                _same(got["summary"][1], got["events"][1], (n, tag, cut, form, "summary against events"))
                _same(got["counts"][1], got["events"][1], (n, tag, cut, form, "counts against events"))
                if first is None:
                    first = got["summary"][1]
                _same(got["summary"][1], first, (n, tag, cut, form, "against", FORMS[0][0]))
                forms_seen.add(got["summary"][2])
                survivors += n_pass
    assert survivors > 0 and forms_seen == {"cx_side_idx", "cx_side_pc", "cx_side", "cx", "dense"}, forms_seen


# ---- the index form's grids: 1 workgroup that only publishes ... 257 workgroups --------------------------------------------
@pytest.mark.parametrize("t_rows", [0, 1, 64, 65, 64 * 64, 64 * 64 + 1])
def test_index_form_grids_below_256_workgroups(ctx, t_rows):
    """T rows on ceil(T / threads) workgroups (one for T = 0): the segments beyond them are unowned, take no ticket and are
    published by workgroup 0; n_pass is T.  At 64 threads 4,096 rows are the last launch that writes a summary (64
    workgroups) and 4,097 the first that stamps a clock per segment instead (65, and 191 unowned segments with clocks)"""
    n = 256
    n_ov = max(8 * t_rows, 64) + 3
    ov, planted, lo = _planted(n, t_rows, n_ov, seed=17 * t_rows + 5)
    bits, at = _matrix(n, ov, seed=19 * t_rows + 5)
    ctx.set_presence(bits, n)
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    sa = (ph8, None, mn, mx, CUT_B, True, len(bits))
    got = {way: _scan(ctx, env_w, sa) for way, env_w in WAYS}
    for way in got:
        assert got[way][2] == "cx_side_idx" and got[way][0] == t_rows, (t_rows, way, got[way][0], got[way][2])
        _same(got[way][1], got["events"][1], (t_rows, way))
    assert np.array_equal(got["summary"][1]["row"].astype(np.int64), at[planted])
    # a second summary scan straight after: the ticket line was re-armed by a launch of fewer than 256 publishers
    again = _scan(ctx, {}, sa)
    assert again[0] == t_rows
    _same(again[1], got["events"][1], (t_rows, "again"))


def test_index_form_at_256_workgroups_twice_over_and_at_257():
    """T = 256 x threads + 1: under PSK_GRID_MULT=1 256 workgroups, workgroup 0 with a second pass; under the build's grid
    multiple 257 workgroups, so segment 0 has two and still one publisher: 256 tickets either way"""
    from phenotypeseeker_amd.engine import PskContext, cx_idx_shape
    n, thr = 256, _threads()
    t_rows = 256 * thr + 1
    ov, planted, lo = _planted(n, t_rows, 8 * t_rows, seed=61)
    bits, at = _matrix(n, ov, seed=62)
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    sa = (ph8, None, mn, mx, CUT_B, True, len(bits))
    assert cx_idx_shape(t_rows, 256)[0] == 256 and cx_idx_shape(t_rows, 1 << 16)[0] == 257
    want = None
    for make in (_new_ctx, lambda: PskContext(0)):
        with make() as c:
            c.set_presence(bits, n)
            got = {way: _scan(c, env_w, sa) for way, env_w in WAYS}
            for way in got:
                assert got[way][2] == "cx_side_idx" and got[way][0] == t_rows, (way, got[way][0], got[way][2])
                _same(got[way][1], got["events"][1], way)
            if want is None:
                want = got["events"][1]
                assert np.array_equal(want["row"].astype(np.int64), at[planted])
            _same(got["summary"][1], want, "257 workgroups against 256")


# ---- two in flight: whose counts a result call reads ------------------------------------------------------------------------
def test_two_in_flight_both_orders_and_a_third_scan_that_takes_the_set(ctx, mixed256):
    from phenotypeseeker_amd._lib import PskError
    bits, ov, t_rows = mixed256
    n = 256
    ctx.set_presence(bits, n)
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    a = (ph8, None, mn, mx, CUT_B, True, len(bits))
    b = (ph8, None, mn, mx, CUT, True, len(bits))
    want = [_scan(ctx, {"PSK_SCAN_WAIT": "0"}, sa)[:2] for sa in (a, b)]
    assert want[0][0] != want[1][0] and min(want[0][0], want[1][0]) > 0
    with knobs({}):
        for rnd in range(4):             # both result sets, both launch orders
            first, second = (0, 1) if rnd % 2 == 0 else (1, 0)
            ctx.chi2_scan_begin(*(a, b)[first])
            ctx.chi2_scan_begin(*(a, b)[second])
            assert ctx.scan_end() == want[first][0], rnd
            if rnd < 2:                  # the ended scan's counts are read now, with the other scan in flight behind it
                _same(ctx.get_results(want[first][0]), want[first][1], (rnd, "first, before the third begins"))
            ctx.chi2_scan_begin(*(a, b)[first])      # a third scan takes the ended scan's set: its counts, read or not, are gone
            with pytest.raises(PskError, match="no ended scan whose results are still held"):
                ctx.get_results(want[first][0])
            assert ctx.scan_end() == want[second][0], rnd
            _same(ctx.get_results(want[second][0]), want[second][1], (rnd, "second"))
            assert ctx.scan_end() == want[first][0], rnd
            _same(ctx.get_results(want[first][0]), want[first][1], (rnd, "third"))
            _same(ctx.get_results(want[first][0]), want[first][1], (rnd, "third, asked twice"))


# ---- 20,000 pairs: the re-arm, and no stale summary ---------------------------------------------------------------------------
def test_20000_pairs_over_four_forms_never_take_another_scans_summary(ctx, mixed256):
    """begin / end 20,000 times with two scans in flight.  Scan i takes phenotype (i >> 1) & 1 -- so the two scans that
    follow one another on a result set differ in their count -- and form (i + (i >> 2)) & 3 of the index form, cx_side_pc,
    cx_side and cx, so every form meets both phenotypes and every form's publish is followed by every other's.  n_pass is
    checked at every step, the results at every 1,000th only: the other sets' count words are never read."""
    bits, ov, t_rows = mixed256
    n = 256
    ctx.set_presence(bits, n)
    phs = _phenotypes(n)
    scans = [(phs[0][1], None, phs[0][2][0], phs[0][2][1], CUT_B, True, len(bits)), (phs[1][1], None, phs[1][2][0], phs[1][2][1], CUT, True, len(bits))]
    want = [_scan(ctx, {"PSK_SCAN_WAIT": "0"}, sa)[:2] for sa in scans]
    assert want[0][0] != want[1][0] and min(want[0][0], want[1][0]) > 0, (want[0][0], want[1][0])
    envs = [env for _, env, _ in FORMS[:4]]
    steps = 20_000
    which = lambda i: ((i >> 1) & 1, (i + (i >> 2)) & 3)
    wrong, forms_seen = [], set()

    def begin(i):
        p, f = which(i)
        os.environ.update(envs[f])
        ctx.chi2_scan_begin(*scans[p])
        for k in envs[f]:
            del os.environ[k]
        if p == 0 and i < 64:
            forms_seen.add(ctx.last_scan_form())

    with knobs({}):
        begin(0)
        for i in range(steps):
            if i + 1 < steps:
                begin(i + 1)
            npass = ctx.scan_end()
            p = which(i)[0]
            if npass != want[p][0]:
                wrong.append((i, npass))
            elif i % 1000 == 999:
                _same(ctx.get_results(npass), want[p][1], ("step", i))
        ms = ctx.last_scan_ms()
    assert not wrong, (len(wrong), wrong[:5], want[0][0], want[1][0])
    assert forms_seen == {"cx_side_idx", "cx_side_pc", "cx_side", "cx"}, forms_seen
    assert math.isfinite(ms) and 0 < ms < 1.0, ms


# ---- scans that keep their events, between and behind summary scans -----------------------------------------------------------
def test_weighted_and_welch_scans_between_and_behind_summary_scans(ctx, mixed256):
    bits, ov, t_rows = mixed256
    n = 256
    ctx.set_presence(bits, n)
    tag, ph8, (mn, mx) = _phenotypes(n)[0]
    a = (ph8, None, mn, mx, CUT_B, True, len(bits))
    b = (ph8, None, mn, mx, CUT, True, len(bits))
    rng = np.random.default_rng(31)
    w = np.round(rng.uniform(0.2, 3.0, n), 6)
    vals = np.round(3.0 + 1.5 * (np.where(np.arange(n) % 2 == 0, 1.0, -1.0) + rng.normal(0, 0.6, n)), 4)
    valid = rng.random(n) > 0.06
    weighted_args = (ph8, w, mn, mx, CUT, True, len(bits))

    def weighted():
        npass = ctx.chi2_scan(*weighted_args)
        return npass, ctx.get_results(npass)

    def welch():
        npass = ctx.ttest_scan(vals, valid, None, 2, n - 2, 0.05, len(bits))
        return npass, ctx.get_results(npass)

    with knobs({"PSK_SCAN_WAIT": "0"}):
        want_a, want_b = _scan(ctx, {"PSK_SCAN_WAIT": "0"}, a)[:2], _scan(ctx, {"PSK_SCAN_WAIT": "0"}, b)[:2]
        want_w, want_t = weighted(), welch()
    assert min(want_a[0], want_b[0], want_w[0], want_t[0]) > 0 and want_a[0] != want_b[0]
    with knobs({}):
        for mid, want in ((weighted, want_w), (welch, want_t)):
            for sa, want_u in ((a, want_a), (b, want_b)):
                got = _scan(ctx, {}, sa)
                assert got[0] == want_u[0]
                _same(got[1], want_u[1], ("summary scan before", mid.__name__))
                got = mid()
                assert got[0] == want[0]
                _same(got[1], want[1], mid.__name__)
                assert ctx.last_scan_ms() > 0
                got = _scan(ctx, {}, sa)
                assert got[0] == want_u[0]
                _same(got[1], want_u[1], ("summary scan after", mid.__name__))
                _check_ms(got[3], got[4], ("summary scan after", mid.__name__))
        # a weighted scan queued behind a summary scan, then a summary scan queued behind a weighted one
        ctx.chi2_scan_begin(*b)
        ctx.chi2_scan_begin(*weighted_args)
        npass = ctx.scan_end()
        assert npass == want_b[0]
        _same(ctx.get_results(npass), want_b[1], "summary scan, a weighted one behind it")
        npass = ctx.scan_end()
        assert npass == want_w[0]
        _same(ctx.get_results(npass), want_w[1], "weighted scan behind a summary scan")
        ctx.chi2_scan_begin(*weighted_args)
        ctx.chi2_scan_begin(*a)
        assert ctx.scan_end() == want_w[0]
        npass = ctx.scan_end()
        assert npass == want_a[0]
        _same(ctx.get_results(npass), want_a[1], "summary scan behind a weighted one")


# ---- the empty matrix, and a knob that is neither 0 nor 1 ------------------------------------------------------------------------
def test_a_matrix_of_no_rows_and_a_bad_knob(ctx):
    from phenotypeseeker_amd._lib import PskError
    from phenotypeseeker_amd.engine import words_per_row
    n = 130
    ctx.set_presence(np.zeros((0, words_per_row(n)), np.uint64), n)
    ph = (np.arange(n) % 2 == 0).astype(np.int8)
    for way, env_w in WAYS:
        with knobs(env_w):
            assert ctx.chi2_scan(ph, None, 2, n - 2, 0.05, True, 1) == 0
            ctx.chi2_scan_begin(ph, None, 2, n - 2, 0.05, True, 1)
            t0 = time.perf_counter()
            assert ctx.scan_end() == 0
            assert time.perf_counter() - t0 < 0.5
            assert len(ctx.get_results(0)["row"]) == 0
    with knobs({"PSK_SCAN_SUMMARY": "2"}):
        with pytest.raises(PskError, match="PSK_SCAN_SUMMARY=2: expected one of 0, 1"):
            ctx.chi2_scan(ph, None, 2, n - 2, 0.05, True, 1)
