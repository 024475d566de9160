"""The time a scan reports (psk_last_scan_ms, psk_rescan_times, psk_rescan_timed, the stream-read ceiling) comes from an
event pair that rides on the kernel's own dispatch (scan_common.h launch_timed).  Whatever the mechanism, a reported
kernel time is positive, finite, and no longer than the host's wall-clock of the call that launched the kernel and
waited for it; and timing a scan must not change what it finds.  Two matrices: one the encoder takes
(chi2_scan_kernel_cx), one it declines (chi2_scan_kernel)."""
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M_ROWS = 20_000
FIELDS = ("row", "stat", "p", "n_with")


def _bits_from_presence(pres, wpr):
    m, n = pres.shape
    bits = np.zeros((m, wpr), dtype=np.uint64)
    for i in range(n):
        bits[:, i >> 6] |= pres[:, i].astype(np.uint64) << np.uint64(i & 63)
    return bits


def _core_or_rare(n, m, seed):
    """The builder of tests/test_gpu_compact_scan.py: rows within 0..7 samples of all-absent or all-present, about 3 %
    of rows with 8 or more exceptions, and about 1.5 % of rows associated with the even / odd phenotype."""
    rng = np.random.default_rng(seed)
    pres = np.zeros((m, n), dtype=bool)
    e = rng.integers(0, 8, m)
    e[:50] = 0
    e[50:100] = 7
    ovf = rng.random(m) < 0.03
    e[ovf] = rng.integers(8, n // 2 + 1, ovf.sum())
    e[100:150] = 8
    flip = rng.random(m) < 0.4
    flip[:25] = True
    flip[25:50] = False
    for r in range(m):
        if e[r]:
            pres[r, rng.choice(n, e[r], replace=False)] = True
    pres[flip] = ~pres[flip]
    assoc = rng.random(m) < 0.015
    even = (np.arange(n) % 2) == 0
    pres[assoc] = np.where(even, rng.random((assoc.sum(), n)) < 0.9, rng.random((assoc.sum(), n)) < 0.1)
    from phenotypeseeker_amd.engine import words_per_row
    return _bits_from_presence(pres, words_per_row(n))


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def encoded_bits():
    return _core_or_rare(130, M_ROWS, 11)


def _load(ctx, kind, encoded_bits):
    """Puts the matrix of `kind` into the context -> its sample count.  The encoder must take the first and decline the
    second: a test of the wrong kernel fails here, it does not skip."""
    if kind == "encoded":
        ctx.set_presence(encoded_bits, 130)
        assert ctx.compact_info()[0], "the core-or-rare matrix was not exception-coded"
        return 130
    ctx.synth_presence(M_ROWS, 256, seed=5)
    assert not ctx.compact_info()[0], "the synthetic matrix was exception-coded"
    return 256


def _phenos(n):
    rng = np.random.default_rng(3)
    a = (np.arange(n) % 2 == 0).astype(np.int8)
    b = np.where(rng.random(n) < 0.08, -1, a).astype(np.int8)     # the same association, some samples NA
    return a, b


def _scan_args(ph, n):
    return (ph, None, 2, n - 2, 0.05, True, M_ROWS)


def _check_ms(ms, wall_s, what):
    print("%s: reported %.3f us, wall-clock %.1f us" % (what, ms * 1e3, wall_s * 1e6))
    assert math.isfinite(ms) and ms > 0, what
    assert ms <= wall_s * 1e3, "%s: the kernel cannot have run longer than the call that waited for it" % what


def _blocking(ctx, args):
    t0 = time.perf_counter()
    npass = ctx.chi2_scan(*args)
    wall = time.perf_counter() - t0
    return ctx.get_results(npass), ctx.last_scan_ms(), wall


@pytest.mark.parametrize("kind", ["encoded", "dense"])
def test_blocking_scan_time_is_positive_and_within_the_call(ctx, encoded_bits, kind):
    n = _load(ctx, kind, encoded_bits)
    for i, ph in enumerate(_phenos(n)):
        res, ms, wall = _blocking(ctx, _scan_args(ph, n))
        assert len(res["row"]) > 0
        _check_ms(ms, wall, "%s blocking scan %d" % (kind, i))


@pytest.mark.parametrize("kind", ["encoded", "dense"])
def test_two_scans_in_flight_time_and_results(ctx, encoded_bits, kind):
    n = _load(ctx, kind, encoded_bits)
    pa, pb = _phenos(n)
    ref = [_blocking(ctx, _scan_args(ph, n))[0] for ph in (pa, pb)]
    assert not np.array_equal(ref[0]["row"], ref[1]["row"]) or not np.array_equal(ref[0]["stat"], ref[1]["stat"])
    t_begin = []
    for ph in (pa, pb):
        t_begin.append(time.perf_counter())
        ctx.chi2_scan_begin(*_scan_args(ph, n))
    for i in range(2):
        npass = ctx.scan_end()
        wall = time.perf_counter() - t_begin[i]
        ms = ctx.last_scan_ms()
        res = ctx.get_results(npass)
        for f in FIELDS:
            assert np.array_equal(res[f], ref[i][f]), (kind, i, f)
        _check_ms(ms, wall, "%s scan %d of two in flight" % (kind, i))
    # both result sets, and with them both event pairs, have been used once: two more scans reuse them
    for i, ph in enumerate((pa, pb)):
        t0 = time.perf_counter()
        ctx.chi2_scan_begin(*_scan_args(ph, n))
        npass = ctx.scan_end()
        wall = time.perf_counter() - t0
        res = ctx.get_results(npass)
        for f in FIELDS:
            assert np.array_equal(res[f], ref[i][f]), (kind, "reused", i, f)
        _check_ms(ctx.last_scan_ms(), wall, "%s scan on a reused event pair %d" % (kind, i))


@pytest.mark.parametrize("kind", ["encoded", "dense"])
def test_repeated_scans_times(ctx, encoded_bits, kind):
    n = _load(ctx, kind, encoded_bits)
    ctx.chi2_scan(*_scan_args(_phenos(n)[0], n))
    t0 = time.perf_counter()
    each = ctx.rescan_times(8)
    wall = time.perf_counter() - t0
    print("%s rescan_times(8): %s us, wall-clock %.1f us" % (kind, np.round(each * 1e3, 3).tolist(), wall * 1e6))
    assert each.shape == (8,) and np.isfinite(each).all() and (each > 0).all()
    assert each.sum() <= wall * 1e3
    t0 = time.perf_counter()
    mean = ctx.rescan_timed(8)
    wall = time.perf_counter() - t0
    _check_ms(mean, wall / 8, "%s rescan_timed(8) mean" % kind)      # the mean of 8 within an eighth of the call: the sum within the call


def test_weighted_scan_time_spans_both_kernels(ctx, encoded_bits):
    """The weighted form is chi2_scan_kernel<..., 1, ...> and chi2w_finalize_kernel.  Its time must span both: an
    unweighted scan of the same matrix reads the exception-coded copy and does no second pass, so it is the shorter
    one; a start event on the finalize kernel alone would make the weighted scan look shorter than that."""
    n = _load(ctx, "encoded", encoded_bits)
    ph = _phenos(n)[0]
    w = np.round(np.random.default_rng(8).uniform(0.2, 3.0, n), 6)
    args_w = (ph, w, 2, n - 2, 0.05, True, M_ROWS)
    ref = ctx.get_results(ctx.chi2_scan(*args_w))
    assert len(ref["row"]) >= 300, "the finalize kernel needs a few hundred candidates to work on"
    ctx.chi2_scan_begin(*args_w)                      # the same scan through the begin / end path
    res = ctx.get_results(ctx.scan_end())
    for f in FIELDS:
        assert np.array_equal(res[f], ref[f]), f
    ms_w, ms_u = [], []
    for _ in range(5):
        _, ms, wall = _blocking(ctx, args_w)
        _check_ms(ms, wall, "weighted scan")
        ms_w.append(ms)
        _, ms, wall = _blocking(ctx, _scan_args(ph, n))
        _check_ms(ms, wall, "unweighted scan")
        ms_u.append(ms)
    print("weighted %s us, unweighted %s us" % (np.round(np.array(ms_w) * 1e3, 3).tolist(), np.round(np.array(ms_u) * 1e3, 3).tolist()))
    assert np.median(ms_w) >= np.median(ms_u)


def test_stream_ceiling_and_welch_scan_times(ctx, encoded_bits, oracle):
    n = _load(ctx, "dense", encoded_bits)
    t0 = time.perf_counter()
    ms, nbytes, shape = ctx.stream_read_ceiling(3)
    wall = time.perf_counter() - t0
    assert nbytes == M_ROWS * 8 * ctx.presence_shape()[1]
    _check_ms(ms, wall / 12, "stream-read ceiling (%s)" % shape)   # four shapes of three launches: the fastest shape's mean launch
    bits = ctx.get_rows(np.arange(M_ROWS, dtype=np.uint64)).reshape(M_ROWS, -1)
    rng = np.random.default_rng(21)
    base = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) + rng.normal(0, 0.6, n)   # follows the even / odd split of the gene rows
    vals = np.round(3.0 + 1.5 * base, 4)
    valid = rng.random(n) > 0.06
    pheno = [float(v) if ok else "NA" for v, ok in zip(vals, valid)]
    ref = oracle.ttest_scan(bits, pheno, np.ones(n), n, 2, n - 2, 0.05, M_ROWS)
    keep = np.nonzero(ref["keep"])[0]
    assert len(keep) > 0
    t0 = time.perf_counter()
    npass = ctx.ttest_scan(vals, valid, None, 2, n - 2, 0.05, M_ROWS)
    wall = time.perf_counter() - t0
    _check_ms(ctx.last_scan_ms(), wall, "Welch scan")
    res = ctx.get_results(npass)
    assert np.array_equal(res["row"], keep.astype(np.uint64))
    assert np.array_equal(res["stat"], ref["stat"][keep])
    assert np.array_equal(res["mean_x"], ref["mean_x"][keep]) and np.array_equal(res["mean_y"], ref["mean_y"][keep])
    assert np.array_equal(res["n_with"], ref["n_with"][keep])
