#!/usr/bin/env python3
"""Decision values of a fitted SVM on new rows: PskContext.svc_decision (psk_svc_decision) against the host loop of model.SVC
(_libsvm_decision without a context) at m = 4096 rows, n_sv = 2048 support vectors, p = 1000 k-mers, for a 0/1 design (the
packed route) and a count design with values 0..5 (the dense route), linear and rbf kernel; and at the shape of the command-line
test (m = 20, n_sv = 18, p = 100).  The model is drawn, not fitted: the cost does not depend on the coefficients.  After a
warm-up call, REPS calls of each are timed by a host clock around the call (the device call ends in a stream synchronise, so
this is check + pack + upload + kernels + read-back, not kernel time); the median and the spread are printed, and the largest
difference between the two results.  Run it under `rocprofv3 --kernel-trace --stats` for the durations of svc_decision_kernel
and the two norm kernels (docs/NOTEBOOK.md).
usage: tools/svc_decision_probe.py [m n_sv p]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, HOST_REPS = 20, 5


def timed(call, reps):
    """(median, min, max) in ms of `reps` calls after one warm-up call."""
    call()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ms)), min(ms), max(ms)


def drawn_model(kernel, SV, rng):
    from phenotypeseeker_amd.model import SVC
    m = SVC(kernel=kernel, gamma=1.0 / SV.shape[1])
    m.support_ = np.arange(len(SV), dtype=np.int32)
    m.support_vectors_ = SV
    m.dual_coef_ = rng.uniform(-1.0, 1.0, (1, len(SV)))
    m.intercept_ = np.array([0.25])
    m._gamma = 1.0 / SV.shape[1]
    return m


from phenotypeseeker_amd.engine import PskContext  # noqa: E402

shapes = [tuple(int(a) for a in sys.argv[1:4])] if len(sys.argv) >= 4 else [(4096, 2048, 1000), (20, 18, 100)]
with PskContext(0) as ctx:
    for m_rows, n_sv, p in shapes:
        for name in ("0/1", "counts"):
            rng = np.random.default_rng(7)
            draw = (lambda r: (rng.random((r, p)) < 0.4).astype(np.float64)) if name == "0/1" else \
                (lambda r: rng.integers(0, 6, (r, p)).astype(np.float64))
            X, SV = draw(m_rows), draw(n_sv)
            for kernel in ("linear", "rbf"):
                model = drawn_model(kernel, SV, rng)
                dev, host = model._libsvm_decision(X, ctx), model._libsvm_decision(X)
                d = timed(lambda: model._libsvm_decision(X, ctx), REPS)
                h = timed(lambda: model._libsvm_decision(X), HOST_REPS)
                print("m=%d n_sv=%d p=%d %-6s %-6s device median %.3f ms (%.3f..%.3f)  host median %.3f ms (%.3f..%.3f)  "
                      "largest |device - host| %.3g" % ((m_rows, n_sv, p, name, kernel) + d + h + (float(np.abs(dev - host).max()),)),
                      flush=True)
