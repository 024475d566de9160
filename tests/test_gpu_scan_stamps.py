"""An unweighted chi2 scan launched through psk_chi2_scan_begin carries no events: psk_scan_end learns that it is done, its
counts and its time from the words its kernel stamps into pinned memory (csrc/scan_stamps.h; PSK_SCAN_WAIT=1, the
default).  PSK_SCAN_WAIT=0 is the event pair on the dispatch.  The two must hand out the same scan bit for bit on every
single-kernel form -- chi2_scan_kernel_cx_side_pc, _cx_side (PSK_CX_PC_FILTER=0), _cx (PSK_CX_SIDE_KERNEL=0), the dense
kernel in MODE 0 and MODE 2 (PSK_SCAN_DENSE=1 with PSK_CHI2_MODE) --, a stamp of another scan must never be taken for
this scan's (70,000 scans in a row, past the wrap of the clock words' 16-bit tag, alternating two phenotypes with
different counts), and the scans that keep their events (weighted, Welch) must go on working between stamped ones.

Two matrices of 20,000 rows: A, 130 samples, core-or-rare, which the encoder takes; B, psk_synth_presence at 256
samples, which it declines.  Three phenotypes: alternating, the same with NA samples, n1 = 3; two cuts: Bonferroni and
omit_B at 0.05."""
import math
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M_ROWS = 20_000
FIELDS = ("row", "stat", "p", "n_with")
KNOBS = ("PSK_SCAN_WAIT", "PSK_SCAN_DENSE", "PSK_CX_SIDE_KERNEL", "PSK_CX_PC_FILTER", "PSK_CHI2_MODE")
FORMS = [("cx_side_pc", {}), ("cx_side", {"PSK_CX_PC_FILTER": "0"}), ("cx", {"PSK_CX_SIDE_KERNEL": "0"}),
         ("dense mode 0", {"PSK_SCAN_DENSE": "1", "PSK_CHI2_MODE": "0"}), ("dense mode 2", {"PSK_SCAN_DENSE": "1", "PSK_CHI2_MODE": "2"})]


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


def _bits_from_presence(pres, wpr):
    m, n = pres.shape
    bits = np.zeros((m, wpr), dtype=np.uint64)
    for i in range(n):
        bits[:, i >> 6] |= pres[:, i].astype(np.uint64) << np.uint64(i & 63)
    return bits


def _core_or_rare(n, m, seed):
    """Rows within 0..7 samples of all-absent or all-present, about 3 % of rows with 8 or more exceptions (the side
    matrix), and about 1.5 % of rows associated with the even / odd phenotype."""
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
def bits_a():
    return _core_or_rare(130, M_ROWS, 19)


def _load(ctx, kind, bits_a):
    """Puts matrix A or B into the context -> its sample count.  The encoder must take A and decline B."""
    if kind == "A":
        ctx.set_presence(bits_a, 130)
        assert ctx.compact_info()[0], "the core-or-rare matrix was not exception-coded"
        return 130
    ctx.synth_presence(M_ROWS, 256, seed=5)
    assert not ctx.compact_info()[0], "the synthetic matrix was exception-coded"
    return 256


def _phenotypes(n):
    rng = np.random.default_rng(1900 + n)
    alt = (np.arange(n) % 2 == 0).astype(np.int8)
    na = np.where(rng.random(n) < 0.08, -1, alt).astype(np.int8)
    few = np.zeros(n, np.int8)
    few[[0, n // 2, n - 2]] = 1
    return [("alternating", alt), ("na", na), ("n1=3", few)]


def _cuts(n):
    """(min, max, cut-off, omit_B, n_kmers_global): Bonferroni, and omit_B at 0.05"""
    return [("bonferroni", (2, n - 2, 0.05, False, M_ROWS)), ("omit_B", (2, n - 2, 0.05, True, M_ROWS))]


def _scan(ctx, env, ph, cut):
    """one blocking scan under the knobs -> (n_pass, results, reported ms, wall-clock s of the scan call)"""
    with knobs(env):
        t0 = time.perf_counter()
        npass = ctx.chi2_scan(ph, None, *cut)
        wall = time.perf_counter() - t0
        ms = ctx.last_scan_ms()
        return npass, ctx.get_results(npass), ms, wall


def _same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


def _check_ms(ms, wall_s, what):
    assert math.isfinite(ms) and ms > 0, (what, ms)
    assert ms <= wall_s * 1e3, "%s: %.3f us reported, the call took %.1f us" % (what, ms * 1e3, wall_s * 1e6)


def _check_form_ran(ctx, form, cut_tag, plan, what):
    """Matrix A, the alternating phenotype (65 + 65 samples): what the library reports of the scan just run is what the
    form's name says.  Bonferroni (threshold 25.8): a row of at most 7 exceptions reaches 130 x 7 / 123 = 7.4, so no slot
    class is feasible and the plan reads the side matrix alone; its rows of 8 exceptions (8.5 at most) are ruled out by
    their popcount, so the filtered kernel runs unless PSK_CX_PC_FILTER=0.  omit_B at 0.05 (threshold 5.99): slot
    classes are feasible, so every coded form is the mixed kernel reading the slots.  (With the slots skipped the
    library's reports do not tell the mixed kernel, PSK_CX_SIDE_KERNEL=0, from the unfiltered side kernel: that choice
    is the plan's `side_kernel && class_mask == 0`, which tests/cx_plan_check.cpp pins.)"""
    filtered, feasible, n_ov = ctx.last_scan_filter()
    if form.startswith("dense"):
        assert plan == (False, 0, False) and (filtered, feasible, n_ov) == (False, 0, 0), (what, plan)
        return
    assert n_ov > 0, what
    if cut_tag == "omit_B":
        assert plan[0] and plan[1] != 0 and not plan[2] and not filtered, (what, plan, filtered)
        return
    assert plan == (True, 0, True), (what, plan)
    if form == "cx_side_pc":
        assert filtered and 0 < feasible < n_ov, (what, filtered, feasible, n_ov)
    else:
        assert (filtered, feasible) == (False, n_ov), (what, filtered, feasible, n_ov)


@pytest.mark.parametrize("kind", ["A", "B"])
def test_stamps_and_events_hand_out_the_same_scan_on_every_form(ctx, bits_a, kind):
    n = _load(ctx, kind, bits_a)
    forms = FORMS if kind == "A" else FORMS[3:]      # B has no exception-coded copy: the dense kernel's two modes
    survivors = 0
    for tag, ph in _phenotypes(n):
        for cut_tag, cut in _cuts(n):
            first = None
            for form, env in forms:
                what = (kind, tag, cut_tag, form)
                n_ev, by_events, ms_ev, wall_ev = _scan(ctx, dict(env, PSK_SCAN_WAIT="0"), ph, cut)
                plan_ev, filt_ev = ctx.last_scan_plan(), ctx.last_scan_filter()
                n_st, by_stamps, ms_st, wall_st = _scan(ctx, dict(env, PSK_SCAN_WAIT="1"), ph, cut)
                assert ctx.last_scan_plan() == plan_ev and ctx.last_scan_filter() == filt_ev, what
                assert plan_ev[0] == (kind == "A" and not form.startswith("dense")), (what, plan_ev)
                if kind == "A" and tag == "alternating":
                    _check_form_ran(ctx, form, cut_tag, plan_ev, what)
                assert n_st == n_ev == len(by_events["row"]), (what, n_st, n_ev)
                _same(by_stamps, by_events, what)
                _check_ms(ms_ev, wall_ev, what + ("events",))
                _check_ms(ms_st, wall_st, what + ("stamps",))
                if first is None:
                    first = by_stamps
                _same(by_stamps, first, what + ("against", forms[0][0]))
                survivors += n_st
    assert survivors > 0


@pytest.mark.parametrize("kind", ["A", "B"])
def test_two_stamped_scans_in_flight_each_get_their_own(ctx, bits_a, kind):
    n = _load(ctx, kind, bits_a)
    (_, pa), (_, pb), _ = _phenotypes(n)
    cut = _cuts(n)[1][1]
    want = [_scan(ctx, {"PSK_SCAN_WAIT": "0"}, ph, cut) for ph in (pa, pb)]
    assert want[0][0] != want[1][0] and min(want[0][0], want[1][0]) > 0
    with knobs({}):
        for rnd in range(3):             # both result sets and both launch orders
            order = (0, 1) if rnd != 1 else (1, 0)
            t_begin = []
            for i in order:
                t_begin.append(time.perf_counter())
                ctx.chi2_scan_begin((pa, pb)[i], None, *cut)
            for j, i in enumerate(order):
                npass = ctx.scan_end()
                wall = time.perf_counter() - t_begin[j]
                _check_ms(ctx.last_scan_ms(), wall, (kind, rnd, i))
                assert npass == want[i][0], (kind, rnd, i)
                _same(ctx.get_results(npass), want[i][1], (kind, rnd, i))


def test_70000_scans_in_a_row_never_take_another_scans_stamp(ctx, bits_a):
    """begin / end, 70,000 times, alternating two phenotypes whose counts differ: the clock words' 16-bit tag wraps on the
    way, both result sets are reused 35,000 times, and a stale word accepted anywhere would show as the wrong count"""
    n = _load(ctx, "A", bits_a)
    (_, pa), (_, pb), _ = _phenotypes(n)
    cut = _cuts(n)[1][1]
    want = [_scan(ctx, {"PSK_SCAN_WAIT": "0"}, ph, cut)[0] for ph in (pa, pb)]
    assert want[0] != want[1] and min(want) > 0
    phs = (np.ascontiguousarray(pa), np.ascontiguousarray(pb))
    wrong = []
    with knobs({}):
        for i in range(70_000):
            ctx.chi2_scan_begin(phs[i & 1], None, *cut)
            npass = ctx.scan_end()
            if npass != want[i & 1]:
                wrong.append((i, npass))
        ms = ctx.last_scan_ms()
    assert not wrong, (len(wrong), wrong[:5], want)
    assert math.isfinite(ms) and 0 < ms < 1.0, ms
    with knobs({}):
        _same(ctx.get_results(ctx.chi2_scan(pb, None, *cut)), _scan(ctx, {"PSK_SCAN_WAIT": "0"}, pb, cut)[1], "after the run")


def test_weighted_and_welch_scans_between_stamped_scans(ctx, bits_a):
    n = _load(ctx, "A", bits_a)
    (_, pa), (_, pb), _ = _phenotypes(n)
    cut = _cuts(n)[1][1]
    rng = np.random.default_rng(23)
    w = np.round(rng.uniform(0.2, 3.0, n), 6)
    vals = np.round(3.0 + 1.5 * (np.where(np.arange(n) % 2 == 0, 1.0, -1.0) + rng.normal(0, 0.6, n)), 4)
    valid = rng.random(n) > 0.06

    def weighted():
        t0 = time.perf_counter()
        npass = ctx.chi2_scan(pa, w, *cut)
        wall = time.perf_counter() - t0
        return npass, ctx.get_results(npass), ctx.last_scan_ms(), wall

    def welch():
        t0 = time.perf_counter()
        npass = ctx.ttest_scan(vals, valid, None, 2, n - 2, 0.05, M_ROWS)
        wall = time.perf_counter() - t0
        return npass, ctx.get_results(npass), ctx.last_scan_ms(), wall

    with knobs({"PSK_SCAN_WAIT": "0"}):      # every scan by its events
        want_a, want_b = _scan(ctx, {"PSK_SCAN_WAIT": "0"}, pa, cut), _scan(ctx, {"PSK_SCAN_WAIT": "0"}, pb, cut)
    with knobs({"PSK_SCAN_WAIT": "0"}):
        want_w, want_t = weighted(), welch()
    assert min(want_a[0], want_b[0], want_w[0], want_t[0]) > 0
    with knobs({}):
        for mid, want in ((weighted, want_w), (welch, want_t)):
            for ph, want_u in ((pa, want_a), (pb, want_b)):
                got = _scan(ctx, {}, ph, cut)
                assert got[0] == want_u[0]
                _same(got[1], want_u[1], "stamped scan before")
                _check_ms(got[2], got[3], "stamped scan before")
                got = mid()
                assert got[0] == want[0]
                _same(got[1], want[1], mid.__name__)
                if mid is welch:
                    assert np.array_equal(got[1]["mean_x"], want[1]["mean_x"]) and np.array_equal(got[1]["mean_y"], want[1]["mean_y"])
                _check_ms(got[2], got[3], mid.__name__)
                got = _scan(ctx, {}, ph, cut)
                assert got[0] == want_u[0]
                _same(got[1], want_u[1], "stamped scan after")
                _check_ms(got[2], got[3], "stamped scan after")
        # a weighted scan through begin / end while a stamped one is in flight: each by its own mechanism
        ctx.chi2_scan_begin(pb, None, *cut)
        ctx.chi2_scan_begin(pa, w, *cut)
        npass = ctx.scan_end()
        assert npass == want_b[0]
        _same(ctx.get_results(npass), want_b[1], "stamped scan, a weighted one behind it")
        npass = ctx.scan_end()
        assert npass == want_w[0]
        _same(ctx.get_results(npass), want_w[1], "weighted scan behind a stamped one")


def _loaded_hip_runtime():
    """the HIP runtime the library has brought into this process, by the path it was mapped from (for hipDeviceSynchronize)"""
    import ctypes
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64.so" in line})
    assert paths, "libpsk.so is loaded but no HIP runtime is mapped"
    return ctypes.CDLL(paths[0])


def test_async_export_on_another_stream_is_ordered_behind_a_stamped_scan(bits_a):
    """psk_export_survivors_async runs on the caller's stream -- here the null stream, which does not wait for the
    context's non-blocking one -- right after psk_scan_end has returned on the stamps: its records must be those of the
    blocking export of the same scan.  From then on the context's scans carry events again (the multi-GPU step), and
    stay right with an export between two scans in flight.  A context of its own: the mark is the context's."""
    from phenotypeseeker_amd.engine import PskContext
    with PskContext(0) as c, knobs({}):
        hip = _loaded_hip_runtime()
        n = _load(c, "A", bits_a)
        (_, pa), (_, pb), _ = _phenotypes(n)
        cut = _cuts(n)[1][1]
        want = {}
        for key, ph in (("a", pa), ("b", pb)):
            with knobs({"PSK_SCAN_WAIT": "0"}):
                npass = c.chi2_scan(ph, None, *cut)
                want[key] = (npass, c.get_results(npass))
        assert want["a"][0] != want["b"][0] and min(want["a"][0], want["b"][0]) > 0
        cap = max(want["a"][0], want["b"][0]) + 8
        rec_bytes = (6 + c.presence_shape()[1]) * 8
        nbytes = (1 + cap) * rec_bytes
        buf_async, buf_sync = c.dev_alloc(nbytes), c.dev_alloc(nbytes)
        try:
            def exported(buf, npass):
                raw = c.dev_download(buf, nbytes).view(np.uint64).reshape(1 + cap, -1)
                assert raw[0, 0] == npass
                return raw[1:1 + npass]

            for rnd, key in enumerate(("a", "b", "a")):          # the first is a stamped scan, the others carry events
                ph = pa if key == "a" else pb
                c.dev_upload(buf_async, np.zeros(nbytes, np.uint8))
                c.chi2_scan_begin(ph, None, *cut)
                npass = c.scan_end()
                c.export_survivors_async(buf_async, cap, 0)
                assert hip.hipDeviceSynchronize() == 0
                assert npass == want[key][0], (rnd, key)
                assert c.export_survivors(buf_sync, cap) == npass
                got, ref = exported(buf_async, npass), exported(buf_sync, npass)
                assert np.array_equal(got, ref), (rnd, key)
                assert np.array_equal(np.sort(got[:, 0]), np.sort(c.get_results(npass)["word"])), (rnd, key)
            # the multi-GPU step: two in flight, the export of the first beside the second, a third scan into the exported set
            c.chi2_scan_begin(pa, None, *cut)
            c.chi2_scan_begin(pb, None, *cut)
            assert c.scan_end() == want["a"][0]
            c.export_survivors_async(buf_async, cap, 0)
            c.chi2_scan_begin(pa, None, *cut)
            npass = c.scan_end()
            assert npass == want["b"][0]
            _same(c.get_results(npass), want["b"][1], "second in flight")
            npass = c.scan_end()
            assert npass == want["a"][0]
            _same(c.get_results(npass), want["a"][1], "third, into the exported set")
            assert hip.hipDeviceSynchronize() == 0
            assert len(exported(buf_async, want["a"][0])) == want["a"][0]
        finally:
            c.dev_free(buf_async)
            c.dev_free(buf_sync)


def test_a_matrix_of_no_rows_returns_an_empty_result_at_once(ctx):
    from phenotypeseeker_amd.engine import words_per_row
    n = 130
    ctx.set_presence(np.zeros((0, words_per_row(n)), np.uint64), n)
    ph = (np.arange(n) % 2 == 0).astype(np.int8)
    with knobs({}):
        assert ctx.chi2_scan(ph, None, 2, n - 2, 0.05, True, 1) == 0
        ctx.chi2_scan_begin(ph, None, 2, n - 2, 0.05, True, 1)
        t0 = time.perf_counter()
        assert ctx.scan_end() == 0
        assert time.perf_counter() - t0 < 0.5
        assert len(ctx.get_results(0)["row"]) == 0
