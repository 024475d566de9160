"""CPU test (-m "not gpu") of csrc/stage_pipeline.h, the three-thread pipeline of the .gz runs: tests/stage_pipeline_check.cpp
runs it with stub stages and checks the wait rules and the hand-over of the first failure from a log of start and end marks."""
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


def test_the_stage_pipeline_keeps_its_wait_rules_and_hands_the_first_failure_over(tmp_path):
    cxx = _hipcc()
    exe = os.path.join(tmp_path, "stage_pipeline_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(ROOT, "tests", "stage_pipeline_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and ", 0 failures" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
