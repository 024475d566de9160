"""CPU test (-m "not gpu") of csrc/scan_stamps.h, the words through which a scan's kernels tell the host their counts, that
they are done and how long they took: tests/scan_stamps_check.cpp includes that header alone and checks the encodings at
their ends, "ready" against every single stale or unwritten word either side of the 16-bit and 32-bit tag wraps, the clock
difference across the 48-bit wrap, and a poll that runs while another thread publishes the words in a shuffled order."""
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


def test_stamp_words_ready_rule_clock_and_a_polling_reader(tmp_path):
    cxx = _hipcc()
    exe = os.path.join(tmp_path, "scan_stamps_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-pthread", os.path.join(ROOT, "tests", "scan_stamps_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " checks, 0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
