"""The plan of the exception-coded chi2 scan on the device (chi2_scan_kernel_cx with the class mask and the corner table of
cx_plan): which header classes a scan decodes, and that a scan none of whose classes is feasible reads the side matrix only.

* Class boundaries: for every class (e = 1 ... 7, base) the largest statistic S a row of that class can reach is computed
  here from the restated statistic; scans with omit_B and cut-offs exp(-S (1 -+ 1e-6) / 2) straddle the class's feasibility
  (the pre-test's own margin is 1e-9), the class mask reported by psk_last_scan_plan flips exactly there, and the survivors
  equal the dense kernel's (PSK_SCAN_DENSE=1, read per call) bit for bit and the oracle's rows.
* Skipped and decoded scans alternate on one context -- one call, two in flight, psk_rescan_timed -- at 300 rows (fewer
  than the workgroups that publish the result segments need) and at 4,096: the counters re-armed by workgroups that only
  publish serve the next scan.
* A matrix with no overflow rows: a skipped scan returns no survivor and valid counts."""
import math

import numpy as np
import pytest

from helpers import chi2_every_table, pack_presence, scan_knobs

pytestmark = pytest.mark.gpu

FIELDS = ("row", "stat", "p", "n_with")
M = 4096


def _matrix(n, m, seed, ov_share=0.05):
    """m hand-made rows at n samples: row i is of class e = i % 8, base = (i // 8) % 2 (every class has m / 16 rows); its
    exceptions are the first e samples, e even samples, or e random ones, so that for the phenotypes below a class reaches
    the largest statistic it can.  About ov_share of the rows have 8 ... n / 2 exceptions instead (the side matrix), a third
    of them associated with the even samples."""
    rng = np.random.default_rng(seed)
    pres = np.zeros((m, n), dtype=bool)
    even = np.arange(0, n, 2)
    for i in range(m):
        e = i % 8
        how = (i // 16) % 3
        idx = np.arange(e) if how == 0 else rng.choice(even, e, replace=False) if how == 1 else rng.choice(n, e, replace=False)
        pres[i, idx] = True
        if (i // 8) % 2:
            pres[i] = ~pres[i]
    ov = np.nonzero(rng.random(m) < ov_share)[0]
    for j, i in enumerate(ov):
        if j % 3 == 0:
            pres[i] = np.where(np.arange(n) % 2 == 0, rng.random(n) < 0.9, rng.random(n) < 0.1)
        else:
            pres[i] = False
            pres[i, rng.choice(n, rng.integers(8, n // 2 + 1), replace=False)] = True
            if j % 3 == 2:
                pres[i] = ~pres[i]
    return pack_presence(pres), len(ov)


def _phenotypes(n, seed):
    rng = np.random.default_rng(seed)
    few = np.zeros(n, np.int8)
    few[:3] = 1
    return {"no NA": (np.arange(n) % 2 == 0).astype(np.int8),
            "8 % NA": np.where(rng.random(n) < 0.08, -1, np.arange(n) % 2 == 0).astype(np.int8),
            "n1 = 3": few}


def _class_max_stat(n1, n0, n_na, mn, mx, stat):
    """[16] the largest finite statistic over the tables a row of class (e | base << 3) can have and the frequency filter
    passes (-inf: none)"""
    out = np.full(16, -np.inf)
    for h in range(16):
        e, base = h & 7, h >> 3
        for ap in range(min(e, n1) + 1):
            for cp in range(min(e - ap, n0) + 1):
                if e - ap - cp > n_na:
                    continue
                a, c = (n1 - ap, n0 - cp) if base else (ap, cp)
                n_w, n_wo = a + c, (n1 - a) + (n0 - c)
                if n_w < mn or n_wo < 2 or n_w > mx or not np.isfinite(stat[a, c]):
                    continue
                out[h] = max(out[h], stat[a, c])
    return out


def _scan(ctx, env, ph8, mn, mx, cut, omit, nk):
    with scan_knobs(env):
        res = ctx.get_results(ctx.chi2_scan(ph8, None, mn, mx, cut, omit, nk))
    return res, ctx.last_scan_plan()


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", [65, 130, 256])
def test_class_mask_flips_at_the_largest_statistic_of_each_class(ctx, oracle, n):
    bits, n_ov = _matrix(n, M, n)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, n_ov) and 0.03 * M < n_ov < 0.08 * M
    mn, mx = 1, n      # min 1: the all-absent table (0, 0), which NA exceptions reach and whose statistic is NaN, is filtered
    flips = 0
    for what, ph8 in _phenotypes(n, n).items():
        n1, n0 = int((ph8 == 1).sum()), int((ph8 == 0).sum())
        stat_t, _ = chi2_every_table(n1, n0)
        smax = _class_max_stat(n1, n0, n - n1 - n0, mn, mx, stat_t)
        ph_list = [("NA" if v < 0 else int(v)) for v in ph8]
        assert smax[0] == -np.inf and smax[8] == -np.inf
        for h in [e | base << 3 for e in range(1, 8) for base in (0, 1)]:
            S = smax[h]
            if S == -np.inf:       # e. g. one absent sample, no NA: n_without = 1 fails the frequency filter
                continue
            assert S > 0.5, (what, h, S)
            for sign in (-1, 1):
                cut = math.exp(-S * (1 + sign * 1e-6) / 2)
                thr = -2.0 * math.log(cut)
                want_mask = sum(1 << k for k in range(16) if smax[k] > thr * (1 - 1e-9))
                assert bool((want_mask >> h) & 1) == (sign < 0)
                got, (enc, mask, skipped) = _scan(ctx, {}, ph8, mn, mx, cut, True, M)
                print("n=%d %s class e=%d base=%d S=%.6f sign=%+d mask=%04x want=%04x skipped=%d survivors=%d"
                      % (n, what, h & 7, h >> 3, S, sign, mask, want_mask, skipped, len(got["row"])))
                assert enc and mask == want_mask, (what, h, sign, hex(mask), hex(want_mask))
                assert skipped == (mask == 0)
                dense, dplan = _scan(ctx, {"PSK_SCAN_DENSE": "1"}, ph8, mn, mx, cut, True, M)
                assert dplan == (False, 0, False)
                for f in FIELDS:
                    assert np.array_equal(got[f], dense[f]), (what, h, sign, f)
                ref = oracle.chi2_scan(bits, ph_list, np.ones(n), n, mn, mx, cut, True, M)
                assert np.array_equal(got["row"], np.nonzero(ref["keep"])[0].astype(np.uint64)), (what, h, sign)
                flips += 1
    assert flips >= 3 * 2 * 10


def _same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS)


@pytest.mark.parametrize("m", [300, M])
def test_skipped_and_decoded_scans_alternate_on_one_context(ctx, m):
    n = 256
    bits, n_ov = _matrix(n, m, 1000 + m)
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, n_ov) and n_ov > 0
    ph8 = _phenotypes(n, 5)["no NA"]
    skip = (ph8, None, 2, n - 2, 0.05, False, m)      # Bonferroni: no slot row can pass
    deco = (ph8, None, 2, n - 2, 0.05, True, m)       # omit_B: the classes of 6 and 7 exceptions can
    with scan_knobs({"PSK_SCAN_DENSE": "1"}):
        want_skip = ctx.get_results(ctx.chi2_scan(*skip))
        want_deco = ctx.get_results(ctx.chi2_scan(*deco))
    assert 0 < len(want_skip["row"]) < len(want_deco["row"])
    with scan_knobs({}):
        # one call at a time
        for args, want, skipped in ((skip, want_skip, True), (deco, want_deco, False), (skip, want_skip, True)):
            c = ctx.chi2_scan(*args)
            enc, mask, was_skipped = ctx.last_scan_plan()
            assert enc and was_skipped == skipped and (mask == 0) == skipped
            assert c == len(want["row"]) and _same(ctx.get_results(c), want)
        # two in flight, either order
        for order in (((skip, want_skip, True), (deco, want_deco, False)), ((deco, want_deco, False), (skip, want_skip, True)),
                      ((skip, want_skip, True), (skip, want_skip, True))):
            for args, _, skipped in order:
                ctx.chi2_scan_begin(*args)
                assert ctx.last_scan_plan()[2] == skipped
            for _, want, _ in order:
                c = ctx.scan_end()
                assert c == len(want["row"]) and _same(ctx.get_results(c), want)
        # repeated launches of the last scan
        for args, want, skipped in ((skip, want_skip, True), (deco, want_deco, False), (skip, want_skip, True)):
            assert ctx.chi2_scan(*args) == len(want["row"])
            assert ctx.rescan_timed(3) > 0
            assert ctx.last_scan_plan()[2] == skipped
            c = ctx.scan_end()
            assert c == len(want["row"]) and _same(ctx.get_results(c), want)


@pytest.mark.parametrize("m", [300, M])
def test_skipped_scan_of_a_matrix_without_overflow_rows(ctx, m):
    n = 200
    bits, n_ov = _matrix(n, m, 7, ov_share=0.0)
    assert n_ov == 0
    ctx.set_presence(bits, n)
    assert ctx.compact_info() == (True, 0)
    ph8 = _phenotypes(n, 6)["8 % NA"]
    with scan_knobs({}):
        for _ in range(2):      # twice: the first scan's workgroups, which only publish, re-armed the counters
            assert ctx.chi2_scan(ph8, None, 2, n - 2, 0.05, False, m) == 0
            assert ctx.last_scan_plan() == (True, 0, True)
            assert len(ctx.get_results(0)["row"]) == 0
        c = ctx.chi2_scan(ph8, None, 2, n - 2, 0.05, True, m)
        got, plan = ctx.get_results(c), ctx.last_scan_plan()
        assert c > 0 and plan[0] and plan[1] != 0 and not plan[2]
        assert ctx.chi2_scan(ph8, None, 2, n - 2, 0.05, False, m) == 0
    with scan_knobs({"PSK_SCAN_DENSE": "1"}):
        assert ctx.chi2_scan(ph8, None, 2, n - 2, 0.05, False, m) == 0
        assert _same(ctx.get_results(ctx.chi2_scan(ph8, None, 2, n - 2, 0.05, True, m)), got)
