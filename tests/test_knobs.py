"""CPU tests (-m "not gpu") of the PSK_* environment knobs: the library reads the environment in one place only, the
knobs the code reads are the ones docs/KNOBS.md's table names, every knob a test sets is one the code reads, and the
Python host reads a flag by the library's rule."""
import glob
import os
import re

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "phenotypeseeker_amd", "csrc")
TEST_OWN = {"PSK_TEST_DATASET", "PSK_PINS_DIR", "PSK_CFG1_TARBALL"}   # read by the tests themselves, not by the package


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _csrc_files():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def _names_the_code_reads():
    names = set()
    for path in _csrc_files():
        names |= set(re.findall(r'\benv_(?:flag|str|int|choice|real)\([^";]*"(PSK_\w+)"', _read(path)))
    for path in glob.glob(os.path.join(ROOT, "phenotypeseeker_amd", "*.py")):
        names |= set(re.findall(r'(?:environ\.get\(|environ\[|getenv\(|env_flag\()\s*["\'](PSK_\w+)["\']', _read(path)))
    return names


def _names_in_the_table():
    names = set()
    for line in _read(os.path.join(ROOT, "docs", "KNOBS.md")).splitlines():
        if line.startswith("| `PSK_"):
            names |= set(re.findall(r"`(PSK_\w+)`", line.split("|")[1]))
    return names


def test_the_library_reads_the_environment_in_one_place():
    hits = [(os.path.basename(p), i + 1, line.strip()) for p in _csrc_files()
            for i, line in enumerate(_read(p).splitlines()) if "getenv(" in line]
    assert len(hits) == 1 and hits[0][0] == "api.hip", hits
    assert re.search(r"env_str\(const char \*name\)\s*\{\s*const char \*v = getenv\(name\);", _read(os.path.join(CSRC, "api.hip")))


def test_the_knob_table_names_every_knob_the_code_reads():
    code, table = _names_the_code_reads(), _names_in_the_table()
    assert len(code) >= 60
    assert code == table, ("read but not in the table", sorted(code - table), "in the table but never read", sorted(table - code))


def test_every_knob_the_tests_set_is_read_by_the_code():
    pats = [r'setenv\(\s*["\'](PSK_\w+)["\']', r'environ\[\s*["\'](PSK_\w+)["\']\s*\]\s*=[^=]', r'["\'](PSK_\w+)["\']\s*:',
            r'[(,]\s*(PSK_\w+)\s*=[^=]']
    set_by_tests = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        txt = _read(path)
        for p in pats:
            set_by_tests |= set(re.findall(p, txt))
    assert len(set_by_tests) >= 40
    dead = set_by_tests - _names_the_code_reads() - TEST_OWN
    assert not dead, sorted(dead)


@pytest.mark.parametrize("value,on", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True), ("00", True)])
def test_python_flags_follow_the_librarys_rule(monkeypatch, value, on):
    from phenotypeseeker_amd._lib import env_flag
    if value is None:
        monkeypatch.delenv("PSK_NO_GPU_GZ", raising=False)
    else:
        monkeypatch.setenv("PSK_NO_GPU_GZ", value)
    assert env_flag("PSK_NO_GPU_GZ") is on
