"""The launch shape of the side-matrix chi2 kernel (psk_cx_side_shape: host code, no GPU) against a simulation of the
sweep's index arithmetic as chi2_scan_kernel_cx_side does it: wave w of the W = 4 * blocks waves takes the batches
w, w + W, ... of batch_rows rows each.  Every row is visited exactly once, and no workgroup visits more rows -- counting
the rows a batch's lanes stand for, past the end included, as the kernel's bound does -- than rows_per_block, which sizes
the result segments.  Integers: no tolerance."""
import ctypes

import numpy as np
import pytest

SC_NSEG = 256
WAVES = 4
N_OV = [0, 1, 31, 32, 33, 127, 128, 129] + [(1 << k) + d for k in range(16, 21) for d in (-1, 0, 1)]
CAPS = [1, 255, 256, 257, 1024, 4096]


def _shape(lib, n_ov, cpr, cap):
    blocks, rpb, batch = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32()
    assert lib.psk_cx_side_shape(n_ov, cpr, cap, ctypes.byref(blocks), ctypes.byref(rpb), ctypes.byref(batch)) == 0
    return blocks.value, rpb.value, batch.value


@pytest.mark.parametrize("cpr", [1, 2])
@pytest.mark.parametrize("cap", CAPS)
def test_sweep_visits_every_row_once_within_rows_per_block(cpr, cap):
    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    rpw = 64 // cpr
    for n_ov in N_OV:
        blocks, rpb, batch = _shape(lib, n_ov, cpr, cap)
        assert blocks >= SC_NSEG, (n_ov, cap)
        assert blocks <= max(cap, SC_NSEG), (n_ov, cap)
        assert batch % rpw == 0 and batch > 0
        unroll = batch // rpw
        n_steps = -(-n_ov // rpw)
        waves = blocks * WAVES
        # the kernel's loop: s0 = wave * unroll; while s0 < n_steps: steps s0 .. s0 + unroll - 1; s0 += waves * unroll
        wave = np.arange(waves, dtype=np.int64)
        edges = np.zeros(n_ov + 1, dtype=np.int64)          # +1 where a batch's rows begin, -1 where they end
        per_wave_real = np.zeros(waves, dtype=np.int64)
        per_wave_batches = np.zeros(waves, dtype=np.int64)
        s0 = wave * unroll
        while True:
            live = s0 < n_steps
            if not live.any():
                break
            per_wave_batches += live
            first = s0[live] * rpw                          # first row of each live wave's batch
            np.add.at(edges, np.minimum(first, n_ov), 1)
            np.add.at(edges, np.minimum(first + batch, n_ov), -1)
            per_wave_real[live] += np.clip(np.minimum(first + batch, n_ov) - first, 0, None)
            s0 = s0 + waves * unroll
        assert np.all(np.cumsum(edges)[:n_ov] == 1), (n_ov, cap, cpr)
        per_block_real = per_wave_real.reshape(blocks, WAVES).sum(axis=1)
        assert per_block_real.sum() == n_ov
        assert per_block_real.max(initial=0) <= rpb, (n_ov, cap, cpr)
        # rows_per_block is the bound of the batches a workgroup's waves take, full or not -- and no looser than that
        assert (per_wave_batches.reshape(blocks, WAVES).sum(axis=1) * batch).max(initial=0) <= rpb
        assert rpb == per_wave_batches.max(initial=0) * WAVES * batch


def test_shape_rejects_bad_arguments():
    from phenotypeseeker_amd import _lib
    lib = _lib.load()
    blocks, rpb = ctypes.c_uint32(), ctypes.c_uint64()
    assert lib.psk_cx_side_shape(100, 3, 256, ctypes.byref(blocks), ctypes.byref(rpb), None) < 0
    assert lib.psk_cx_side_shape(100, 2, 0, ctypes.byref(blocks), ctypes.byref(rpb), None) < 0
    assert lib.psk_cx_side_shape(100, 2, 256, None, ctypes.byref(rpb), None) < 0
    assert lib.psk_cx_side_shape(100, 2, 256, ctypes.byref(blocks), ctypes.byref(rpb), None) == 0
    assert blocks.value == SC_NSEG
