"""CPU test (-m "not gpu") of the summary line of csrc/scan_stamps.h, the four words through which a single-kernel scan's
last publisher tells the host that the scan has ended, its n_pass and its time, and of the ticket arithmetic that finds
that publisher: tests/scan_summary_check.cpp includes that header alone and checks the words at the ends of n_pass and
either side of the 16-bit and 32-bit wraps of the launch number, "ready" against every single stale or unwritten word, the
tickets of 1, 28, 256 and 257 workgroups in shuffled order with counts adding up past 2^32 (exactly one "last", the right
total, the sticky overflow flag -- a segment overflow cannot be reached through a scan's parameters, so this is where that
path is covered), and a poll that runs while another thread publishes 400 launches.  The same program is run again under
the thread sanitizer and under the address and undefined-behaviour sanitizers, as a program of its own."""
import os
import subprocess

import pytest

from helpers import ROOT


def _hipcc():
    """The compiler csrc/Makefile builds the library with (HIPCC overrides it, as there): without it nothing here builds, so
    its absence fails the test."""
    if os.environ.get("HIPCC"):
        return os.environ["HIPCC"]
    with open(os.path.join(ROOT, "phenotypeseeker_amd", "csrc", "Makefile")) as f:
        return next(line.split("=", 1)[1].strip() for line in f if line.startswith("HIPCC ?="))


@pytest.mark.parametrize("tag,flags", [("plain", ["-O1"]), ("tsan", ["-O1", "-g", "-fsanitize=thread"]),
                                       ("asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_summary_words_ready_rule_tickets_and_a_polling_reader(tmp_path, tag, flags):
    cxx = _hipcc()
    exe = os.path.join(tmp_path, "scan_summary_check_" + tag)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-pthread"] + flags + [os.path.join(ROOT, "tests", "scan_summary_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " checks, 0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
