"""CPU test (-m "not gpu") of csrc/gz_plan.h, the host's part of the device inflate: tests/gz_plan_check.cpp builds gzip images
with zlib, plays the device's find and counting passes from zlib's own block boundaries and checks which files the walk along
the links accepts, and the layout of their texts and members, against zlib."""
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


def test_the_chain_walk_and_the_text_layout_agree_with_zlib(tmp_path):
    cxx = _hipcc()
    exe = os.path.join(tmp_path, "gz_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "gz_plan_check.cpp"), "-o", exe, "-lz"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " checks, 0 failures" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
