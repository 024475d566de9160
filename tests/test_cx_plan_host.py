"""The per-scan plan of the exception-coded chi2 scan (psk_cx_plan: host code, no GPU) against brute force over the full
(a, c) table built from psk_chi2_pretest and the frequency filter as modeling.py:770-772 states it.  Every corner bit
equals the brute-force bit of its table point, and a header class (e, base) is feasible exactly when some table a row of
that class can have is a candidate.  Booleans: no tolerance."""
import ctypes
import math

import numpy as np
import pytest

CONFIGS = [(33, 32, 0), (128, 128, 0), (3, 125, 0), (0, 65, 0), (100, 90, 10), (5, 4, 191)]   # (n1, n0, n_na)


def _thresholds(n1, n0):
    """The statistic thresholds of a Bonferroni run (22.8 M and 20,000 k-mers), omit_B at 0.05, a cut >= 1, a cut of 0, a
    tiny cut, and values around what the small classes can reach"""
    return [-2.0 * math.log(0.05 / 22.8e6), -2.0 * math.log(0.05 / 2e4), -2.0 * math.log(0.05), 0.0, math.inf,
            -2.0 * math.log(1e-30), 1.0, 2.5, 4.0, 7.2, 8.09]


def _filters(n):
    return [(0, n), (2, n - 2), (n // 2, n // 2), (3, 5)]


def _pretest_table(lib, n1, n0, thr):
    t = np.zeros((n1 + 1, n0 + 1), dtype=bool)
    for a in range(n1 + 1):
        for c in range(n0 + 1):
            t[a, c] = bool(lib.psk_chi2_pretest(float(a), float(n1 - a), float(c), float(n0 - c), thr))
    return t


def _plan(lib, n1, n0, n, mn, mx, thr):
    mask = ctypes.c_uint32(0xdeadbeef)
    corner = (ctypes.c_uint64 * 2)(~0, ~0)
    assert lib.psk_cx_plan(n1, n0, n, mn, mx, thr, ctypes.byref(mask), corner) == 0
    return mask.value, (corner[0], corner[1])


@pytest.mark.parametrize("n1,n0,n_na", CONFIGS)
def test_plan_equals_brute_force(n1, n0, n_na):
    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    n = n1 + n0 + n_na
    a = np.arange(n1 + 1)[:, None]
    c = np.arange(n0 + 1)[None, :]
    n_w, n_wo = a + c, (n1 - a) + (n0 - c)
    seen_infeasible = seen_mixed = 0
    for thr in _thresholds(n1, n0):
        pre = _pretest_table(lib, n1, n0, thr)
        for mn, mx in _filters(n):
            cand = pre & ~((n_w < mn) | (n_wo < 2) | (n_w > mx))       # the full (a, c) candidate table
            mask, corner = _plan(lib, n1, n0, n, mn, mx, thr)
            assert mask >> 16 == 0
            for base in (0, 1):
                for ap in range(8):
                    for cp in range(8):
                        inside = ap <= n1 and cp <= n0
                        ai, ci = (n1 - ap, n0 - cp) if base else (ap, cp)
                        want = bool(inside and cand[ai, ci])
                        assert bool((corner[base] >> (ap * 8 + cp)) & 1) == want, (thr, mn, mx, base, ap, cp)
                for e in range(8):
                    # a row of e exceptions: a' of them cases, c' controls, the other e - a' - c' NA samples
                    reach = [(ap, cp) for ap in range(min(e, n1) + 1) for cp in range(min(e - ap, n0) + 1)
                             if e - ap - cp <= n_na]
                    want = any(cand[(n1 - ap, n0 - cp) if base else (ap, cp)] for ap, cp in reach)
                    assert bool((mask >> (e | base << 3)) & 1) == want, (thr, mn, mx, base, e)
            seen_infeasible += mask == 0
            seen_mixed += mask != 0
    # the sweep reaches both outcomes: no class feasible (the slot stream is skipped), and some
    assert seen_infeasible > 0 and seen_mixed > 0


def test_plan_at_bonferroni_cutoffs_skips_every_class():
    """The flagship scan (128 + 128 samples, 22.8 M k-mers) and the 65- and 130-sample ones: no class of at most 7
    exceptions reaches the Bonferroni threshold; with omit_B at 0.05 the larger classes do"""
    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    for n1, n0 in ((128, 128), (33, 32), (65, 65)):
        n = n1 + n0
        assert _plan(lib, n1, n0, n, 2, n - 2, -2.0 * math.log(0.05 / 22.8e6))[0] == 0
        assert _plan(lib, n1, n0, n, 2, n - 2, -2.0 * math.log(0.05 / 2e4))[0] == 0
        mask = _plan(lib, n1, n0, n, 2, n - 2, -2.0 * math.log(0.05))[0]
        assert mask & (1 << 7) and mask & (1 << 15) and not mask & (1 << 2)


def test_plan_rejects_bad_arguments():
    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    mask = ctypes.c_uint32()
    corner = (ctypes.c_uint64 * 2)()
    assert lib.psk_cx_plan(10, 10, 19, 0, 19, 1.0, ctypes.byref(mask), corner) < 0     # n1 + n0 > n_samples
    assert lib.psk_cx_plan(-1, 10, 19, 0, 19, 1.0, ctypes.byref(mask), corner) < 0
    assert lib.psk_cx_plan(10, 9, 19, 0, 19, 1.0, None, corner) < 0
