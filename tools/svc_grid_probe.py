#!/usr/bin/env python3
"""The grid search of `-bc SVM` (13 values of C x 10 folds + 13 refits = 143 fits, tol 1e-4, max_iter 1000) through
psk_svc_fit, next to psk_logreg_l1_fit on the same designs: gene-block 0/1 designs of (n, p) = (256, 1000) and
(2048, 1000).  Prints wall-clock and iteration counts; run it under `rocprofv3 --kernel-trace --stats` for the durations
of svc_gram_bits_kernel and svc_smo_kernel (docs/NOTEBOOK.md).
usage: tools/svc_grid_probe.py [n ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_svm_golden import CS, design  # noqa: E402
from phenotypeseeker_amd import cv  # noqa: E402
from phenotypeseeker_amd.engine import PskContext  # noqa: E402

sizes = [int(a) for a in sys.argv[1:]] or [256, 2048]
with PskContext(0) as ctx:
    for n in sizes:
        X, y = design(n, 1000, 2, 0.42)
        folds = cv.stratified_kfold(y, 10)
        fp = [C for C in CS for _ in range(10)] + list(CS)
        ff = [f for _ in CS for f in range(10)] + [-1] * len(CS)
        for kern in ("linear", "rbf"):
            ctx.svc_fit(X, y, folds, fp[:2], ff[:2], kernel=kern, fit_gamma=1e-3, tol=1e-4, max_iter=10)   # code objects
            t = time.perf_counter()
            _, _, _, it = ctx.svc_fit(X, y, folds, fp, ff, kernel=kern, fit_gamma=1.0 / 1000, tol=1e-4, max_iter=1000)
            print("psk_svc_fit %-6s n=%d p=1000: %d fits in %.1f ms, iterations %d..%d (%d at the limit)"
                  % (kern, n, len(fp), 1e3 * (time.perf_counter() - t), it.min(), it.max(), int(np.sum(it >= 1000))), flush=True)
        ctx.logreg_l1_fit(X, y, folds, fp[:2], ff[:2], 1e-4, 10)
        t = time.perf_counter()
        _, _, it = ctx.logreg_l1_fit(X, y, folds, fp, ff, 1e-4, 1000)
        print("psk_logreg_l1_fit n=%d p=1000: %d fits in %.1f ms" % (n, len(fp), 1e3 * (time.perf_counter() - t)), flush=True)
