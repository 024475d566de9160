"""The host's side of the index form of the chi2 scan (chi2_scan_kernel_cx_side_idx), no GPU: psk_cx_idx_plan -- where
the feasible rows lie in the encoder's index of the side matrix by popcount, and whether the form is chosen -- against a
brute-force walk over the index positions, and psk_cx_idx_shape against a simulation of the kernel's sweep.  Integers:
no tolerance."""
import numpy as np
import pytest

SC_NSEG = 256
RUNS = 4      # CX_IDX_RUNS
SHARE = 8     # CX_IDX_SHARE


def _brute(feas, hist):
    """maximal stretches of index positions that belong to feasible buckets: [(begin, len)]"""
    marked = np.zeros(int(sum(hist)) + 1, bool)       # (+1: a sentinel that ends the last stretch)
    pos = 0
    for pc, h in enumerate(hist):
        if pc in feas and pc < 256:
            marked[pos:pos + h] = True
        pos += h
    edges = np.flatnonzero(np.diff(np.concatenate([[False], marked]).astype(np.int8)))
    return [(int(b), int(e - b)) for b, e in zip(edges[0::2], edges[1::2])]


def _check(feas, hist, n_ov=None, knob=True):
    from phenotypeseeker_amd.engine import cx_idx_plan
    n_ov = int(sum(hist)) if n_ov is None else n_ov
    want = _brute(feas, hist)
    runs, n_runs, rows, chosen = cx_idx_plan(feas, hist, n_ov, knob)
    assert n_runs == len(want), (feas, hist, runs, want)
    assert runs == want[:RUNS]
    assert rows == sum(ln for _, ln in want)
    assert chosen == (knob and n_runs <= RUNS and rows * SHARE <= n_ov)
    return runs, n_runs, rows, chosen


def _hist(n=256, fill=3):
    return [fill] * (n + 1)


def test_empty_and_full_bitmap():
    h = _hist()
    assert _check(set(), h) == ([], 0, 0, True)                       # no row at all: chosen, one workgroup that only publishes
    runs, n_runs, rows, chosen = _check(set(range(256)), h)
    assert runs == [(0, 3 * 256)] and n_runs == 1 and not chosen      # (bin 256 has no bit: a side-matrix row has fewer)
    assert _check(set(range(256)), []) == ([], 0, 0, True)            # no histogram


def test_one_and_two_runs():
    h = _hist()
    assert _check(set(range(35, 222)), h, n_ov=10 ** 6)[:3] == ([(35 * 3, 187 * 3)], 1, 187 * 3)
    runs, n_runs, rows, chosen = _check(set(range(10, 20)) | set(range(200, 205)), h, n_ov=10 ** 6)
    assert runs == [(30, 30), (600, 15)] and n_runs == 2 and chosen


def test_four_runs_are_taken_and_five_decline():
    h = _hist()
    four = {10, 20, 30, 40}
    assert _check(four, h, n_ov=10 ** 6)[1:] == (4, 12, True)
    runs, n_runs, rows, chosen = _check(four | {50}, h, n_ov=10 ** 6)
    assert n_runs == 5 and rows == 15 and not chosen and len(runs) == 4
    assert _check(four | {50, 60, 61}, h, n_ov=10 ** 6)[1:] == (6, 21, False)


def test_feasible_buckets_separated_only_by_empty_ones_merge():
    h = _hist()
    for pc in (21, 22, 23):
        h[pc] = 0
    runs, n_runs, rows, _ = _check({20, 24}, h)                       # infeasible but empty between them: one range
    assert runs == [(60, 6)] and n_runs == 1
    runs, n_runs, rows, _ = _check({20, 22, 24}, h)                   # a feasible empty bucket between them as well
    assert runs == [(60, 6)] and n_runs == 1
    h[22] = 1
    assert _check({20, 24}, h)[:2] == ([(60, 3), (64, 3)], 2)         # one infeasible row between them: two ranges
    # five feasible buckets of which empty ones make three ranges: chosen, where five ranges would not be
    h2 = _hist()
    for pc in (11, 12, 31):
        h2[pc] = 0
    assert _check({10, 13, 30, 32, 50}, h2, n_ov=10 ** 6)[1:] == (3, 15, True)


def test_feasible_bucket_that_is_empty_at_either_end():
    h = _hist()
    h[10] = h[19] = 0
    runs, n_runs, rows, _ = _check(set(range(10, 20)), h)
    assert runs == [(30, 24)] and rows == 24
    h0 = _hist()
    h0[0] = h0[255] = 0
    runs, n_runs, rows, _ = _check({0, 1, 254, 255}, h0)
    assert runs == [(0, 3), (3 * 253, 3)]
    only_empty = [0] * 257
    only_empty[100] = 7
    assert _check({99, 101}, only_empty) == ([], 0, 0, True)          # every feasible bucket empty


def test_share_rule_on_both_sides_of_its_edge():
    h = [0] * 257
    h[40], h[100] = 1000, 125
    assert _check({100}, h, n_ov=SHARE * 125)[3] is True
    assert _check({100}, h, n_ov=SHARE * 125 - 1)[3] is False
    assert _check({100}, h, n_ov=SHARE * 125, knob=False)[3] is False
    assert _check({100}, h)[3] is True and _check({40}, h)[3] is False


def test_random_bitmaps_and_histograms():
    rng = np.random.default_rng(25)
    for _ in range(300):
        n = int(rng.integers(65, 257))
        hist = (rng.integers(0, 50, n + 1) * (rng.random(n + 1) < rng.random())).tolist()
        feas = set(np.flatnonzero(rng.random(256) < rng.random()).tolist())
        _check(feas, hist, n_ov=int(sum(hist)) * int(rng.integers(1, 3)))


@pytest.mark.parametrize("cap", [256, 2048])
def test_shape_against_a_simulated_sweep(cap):
    from phenotypeseeker_amd.engine import cx_idx_shape
    thr = cx_idx_shape(0, cap)[2]
    assert thr in (64, 256)
    sizes = [0, 1, thr - 1, thr, thr + 1, SC_NSEG * thr - 1, SC_NSEG * thr, SC_NSEG * thr + 1,
             cap * thr - 1, cap * thr, cap * thr + 1, 2 * cap * thr, 2 * cap * thr + 1]
    for t_rows in sizes:
        blocks, rpb, th, seg_cap = cx_idx_shape(t_rows, cap)
        assert th == thr
        assert blocks == min(max(-(-t_rows // thr), 1), cap), (t_rows, cap)      # what the rows need: NOT raised to the segments
        # the kernel's loop: t0 = b * thr; while t0 < T: rows t0 .. t0 + thr - 1 below T; t0 += blocks * thr
        seen = np.zeros(t_rows, np.int32)
        per_block = np.zeros(blocks, np.int64)
        passes = 0
        t0 = np.arange(blocks, dtype=np.int64) * thr
        while (t0 < t_rows).any():
            passes += 1
            for b in np.flatnonzero(t0 < t_rows):
                hi = min(int(t0[b]) + thr, t_rows)
                seen[int(t0[b]):hi] += 1
                per_block[b] += hi - int(t0[b])
            t0 += blocks * thr
        assert np.all(seen == 1) and per_block.sum() == t_rows
        assert rpb == passes * thr and per_block.max() <= rpb
        per_seg = np.bincount(np.arange(blocks) % SC_NSEG, weights=per_block, minlength=SC_NSEG)
        assert per_seg.max() <= seg_cap
        assert seg_cap == max(64, -(-blocks // SC_NSEG) * rpb)
    assert cx_idx_shape(cap * thr + 1, cap)[1] == 2 * thr                         # beyond cap x threads: a second pass


def test_shape_rejects_bad_arguments():
    import ctypes

    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    blocks, rpb = ctypes.c_uint32(), ctypes.c_uint64()
    assert lib.psk_cx_idx_shape(100, 0, ctypes.byref(blocks), ctypes.byref(rpb), None, None) < 0
    assert lib.psk_cx_idx_shape(100, 1 << 32, ctypes.byref(blocks), ctypes.byref(rpb), None, None) < 0
    assert lib.psk_cx_idx_shape(100, 256, None, ctypes.byref(rpb), None, None) < 0
    assert lib.psk_cx_idx_shape(100, 256, ctypes.byref(blocks), ctypes.byref(rpb), None, None) == 0
    assert blocks.value == -(-100 // rpb.value)      # one pass: rows_per_block is the workgroup's threads
