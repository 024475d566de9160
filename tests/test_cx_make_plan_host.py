"""CPU test (-m "not gpu") of csrc/chi2_plan.h, everything the host decides about an exception-coded chi2 scan:
tests/cx_plan_check.cpp includes that header alone and checks which kernel form cx_make_plan picks over knobs, class masks
and popcount histograms, simulates the index arithmetic of the three exception-coded kernels on the shapes the plan returns
(every slot pair and side-matrix row once, within the bound that sizes the result segments), and pins the flagship plan."""
import os
import subprocess

from helpers import ROOT


def _hipcc():
    """The compiler csrc/Makefile builds the library with (HIPCC overrides it, as there): without it nothing here builds, so
    its absence fails the test."""
    if os.environ.get("HIPCC"):
        return os.environ["HIPCC"]
    with open(os.path.join(ROOT, "phenotypeseeker_amd", "csrc", "Makefile")) as f:
        return next(line.split("=", 1)[1].strip() for line in f if line.startswith("HIPCC ?="))


def test_form_selection_sweeps_and_the_flagship_plan(tmp_path):
    cxx = _hipcc()
    exe = os.path.join(tmp_path, "cx_plan_check")
    # -ffp-contract=off: the pre-test's A * D - B * C must not be fused on the host either
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", os.path.join(ROOT, "tests", "cx_plan_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " checks, 0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
