"""The popcount plan of the side-matrix chi2 scan (psk_cx_pc_plan: host code, no GPU) against brute force over the full
(a, c) table built from psk_chi2_pretest and the frequency filter as the scan kernels state it: bit pc is set exactly
when some table with a + c in [max(0, pc - n_na), min(pc, n1 + n0)] is a candidate.  Booleans: no tolerance."""
import ctypes

import numpy as np
import pytest

from test_cx_plan_host import CONFIGS, _pretest_table, _thresholds

SHAPES = CONFIGS + ([] if (3, 125, 0) in CONFIGS else [(3, 125, 0)])   # (n1, n0, n_na)


def _filters(n):
    return [(0, n), (2, n - 2), (8, n - 8), (n // 2, n // 2)]


def _feas(lib, n1, n0, n, mn, mx, thr):
    words = (ctypes.c_uint64 * 4)(~0, ~0, ~0, ~0)
    assert lib.psk_cx_pc_plan(n1, n0, n, mn, mx, thr, words) == 0
    return np.array([(words[pc >> 6] >> (pc & 63)) & 1 for pc in range(256)], dtype=bool)


def _runs(bits):
    """maximal runs of set bits"""
    d = np.diff(np.concatenate([[0], bits.astype(np.int8), [0]]))
    return int((d == 1).sum())


def test_pc_plan_equals_brute_force():
    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    seen_empty = seen_full = seen_two_runs = 0
    for n1, n0, n_na in SHAPES:
        n = n1 + n0 + n_na
        a = np.arange(n1 + 1)[:, None]
        c = np.arange(n0 + 1)[None, :]
        n_w, n_wo = a + c, (n1 - a) + (n0 - c)
        for thr in _thresholds(n1, n0):
            pre = _pretest_table(lib, n1, n0, thr)
            for mn, mx in _filters(n):
                cand = pre & ~((n_w < mn) | (n_wo < 2) | (n_w > mx))       # the full (a, c) candidate table
                by_sum = np.zeros(n1 + n0 + 1, dtype=bool)                 # some table of that a + c is a candidate
                np.logical_or.at(by_sum, n_w[cand], True)
                want = np.zeros(256, dtype=bool)
                for pc in range(256):
                    lo, hi = max(0, pc - n_na), min(pc, n1 + n0)
                    want[pc] = lo <= hi and bool(by_sum[lo:hi + 1].any())
                got = _feas(lib, n1, n0, n, mn, mx, thr)
                assert np.array_equal(got, want), ((n1, n0, n_na), thr, mn, mx, np.nonzero(got != want)[0][:8])
                band = got[8:n - 8 + 1]                                     # the popcounts a side-matrix row can have
                seen_empty += not got.any()
                seen_full += n >= 16 and bool(band.all())
                seen_two_runs += _runs(got) >= 2
    assert seen_empty > 0 and seen_full > 0 and seen_two_runs > 0, (seen_empty, seen_full, seen_two_runs)


def test_pc_plan_of_the_issues_examples():
    """n1 = 3, n0 = 125, rows of 8 <= pc <= 120: at the flagship's Bonferroni threshold only {8, 9} and {119, 120} are left,
    at omit_B with 0.01 [8, 32] and [96, 120]; the flagship scan itself keeps [35, 221]"""
    import math
    from phenotypeseeker_amd.engine import cx_pc_plan
    band = set(range(8, 121))
    assert cx_pc_plan(3, 125, 128, 2, 126, 39.9) & band == {8, 9, 119, 120}
    assert cx_pc_plan(3, 125, 128, 2, 126, 9.21) & band == set(range(8, 33)) | set(range(96, 121))
    assert cx_pc_plan(128, 128, 256, 2, 254, -2.0 * math.log(0.05 / 22950458)) == set(range(35, 222))


def test_pc_plan_rejects_bad_arguments():
    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    words = (ctypes.c_uint64 * 4)()
    assert lib.psk_cx_pc_plan(10, 10, 19, 0, 19, 1.0, words) < 0     # n1 + n0 > n_samples
    assert lib.psk_cx_pc_plan(-1, 10, 19, 0, 19, 1.0, words) < 0
    assert lib.psk_cx_pc_plan(10, 9, 19, 0, 19, 1.0, None) < 0
    assert lib.psk_cx_pc_plan(128, 129, 257, 0, 257, 1.0, words) < 0   # more samples than four words of popcounts hold
    assert lib.psk_cx_pc_plan(10, 9, 19, 0, 19, 1.0, words) == 0
