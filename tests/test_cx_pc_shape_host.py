"""The launch shape of the popcount-filtered side-matrix kernel (psk_cx_pc_shape: host code, no GPU) against a simulation
of the sweep's index arithmetic as chi2_scan_kernel_cx_side_pc does it: wave w of the W = 4 * blocks waves takes the
batches w, w + W, ... of batch_rows rows each, one row per lane.  Every row is visited exactly once, and no workgroup
visits more rows -- counting the rows a batch's lanes stand for, past the end included, as the kernel's bound does -- than
rows_per_block, which sizes the result segments.  Integers: no tolerance."""
import ctypes

import numpy as np
import pytest

SC_NSEG = 256
WAVES = 4
CAPS = [256, 2048]


def _shape(lib, n_ov, cap):
    blocks, rpb, batch = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32()
    assert lib.psk_cx_pc_shape(n_ov, cap, ctypes.byref(blocks), ctypes.byref(rpb), ctypes.byref(batch)) == 0
    return blocks.value, rpb.value, batch.value


@pytest.mark.parametrize("cap", CAPS)
def test_sweep_visits_every_row_once_within_rows_per_block(cap):
    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    batch = _shape(lib, 0, cap)[2]
    assert batch in (256, 512)                               # 64 rows x an unroll of 4 or 8: at least 512 rows per wave and round at 8
    one_each = cap * WAVES * batch                           # one batch per wave of the capped grid
    for n_ov in [0, 1, 511, 512, 513, one_each - 1, one_each, one_each + 1]:
        blocks, rpb, b = _shape(lib, n_ov, cap)
        assert b == batch
        assert SC_NSEG <= blocks <= max(cap, SC_NSEG), (n_ov, cap)
        n_batches = -(-n_ov // batch)
        waves = blocks * WAVES
        # the kernel's loop: b = wave; while b < n_batches: rows b * batch .. (b + 1) * batch - 1; b += waves
        edges = np.zeros(n_ov + 1, dtype=np.int64)          # +1 where a batch's rows begin, -1 where they end
        per_wave_real = np.zeros(waves, dtype=np.int64)
        per_wave_batches = np.zeros(waves, dtype=np.int64)
        bi = np.arange(waves, dtype=np.int64)
        while True:
            live = bi < n_batches
            if not live.any():
                break
            per_wave_batches += live
            first = bi[live] * batch
            np.add.at(edges, np.minimum(first, n_ov), 1)
            np.add.at(edges, np.minimum(first + batch, n_ov), -1)
            per_wave_real[live] += np.clip(np.minimum(first + batch, n_ov) - first, 0, None)
            bi = bi + waves
        assert np.all(np.cumsum(edges)[:n_ov] == 1), (n_ov, cap)
        per_block_real = per_wave_real.reshape(blocks, WAVES).sum(axis=1)
        assert per_block_real.sum() == n_ov
        assert per_block_real.max(initial=0) <= rpb, (n_ov, cap)
        # rows_per_block is the bound of the batches a workgroup's waves take, full or not -- and no looser than that
        assert (per_wave_batches.reshape(blocks, WAVES).sum(axis=1) * batch).max(initial=0) <= rpb
        assert rpb == per_wave_batches.max(initial=0) * WAVES * batch


def test_shape_rejects_bad_arguments():
    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    blocks, rpb = ctypes.c_uint32(), ctypes.c_uint64()
    assert lib.psk_cx_pc_shape(100, 0, ctypes.byref(blocks), ctypes.byref(rpb), None) < 0
    assert lib.psk_cx_pc_shape(100, 1 << 32, ctypes.byref(blocks), ctypes.byref(rpb), None) < 0
    assert lib.psk_cx_pc_shape(100, 256, None, ctypes.byref(rpb), None) < 0
    assert lib.psk_cx_pc_shape(100, 256, ctypes.byref(blocks), None, None) < 0
    assert lib.psk_cx_pc_shape(100, 256, ctypes.byref(blocks), ctypes.byref(rpb), None) == 0
    assert blocks.value == SC_NSEG
