"""CPU tests (-m "not gpu") of the `-a/--assembly` path's host side: the Python restatement (tests/asm_restated.py) against the
reference's recorded assemblies (tests/golden/asm_kat.json, tools/gen_asm_golden.py) in both strand modes, the package's path
(assembly.py, modeling.py) with the engine served by the restatement -- the FASTA, the knobs, the three cases without an
assembly, the warning-and-no-file route of a cap, today's warning without PSK_ASM -- and csrc/asm_host.h through the
stand-alone program tests/asm_host_check.cpp, plain and under the address and undefined-behaviour sanitizers."""
import os
import random
import subprocess

import numpy as np
import pytest

import asm_restated as R
from helpers import ROOT
from test_gz_plan_host import _hipcc

CASES = ["a_windows_k13", "b_windows_k32", "c_palindromes_k12", "d_two_bubbles", "e_three_bubbles", "f_no_overlaps", "g_single", "h_word_edges"]
SKIPPED = "\x1b[1;33m-a/--assembly is outside the accelerated path and is skipped.\x1b[0m\n"


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


@pytest.fixture(scope="module")
def restated(fx):
    """The restatement's assembly of every golden case in both modes; computed once."""
    return {(name, both): R.assemble(kmers, k, both) for name, k, kmers, both, _ in fx.runs()}


def test_fixture_holds_what_the_tests_need(fx):
    assert fx.names == CASES and os.path.getsize(fx.path) < 1 << 20
    for name in CASES:
        c = fx.cases[name]
        k, kmers = c["k"], c["kmers"]
        assert kmers and len(set(kmers)) == len(kmers) and all(len(s) == k and s == min(s, R.revcomp(s)) for s in kmers), name
        for mode in ("one_strand", "both_strands"):
            assert c[mode]["assembled"] and 0 <= c[mode]["seconds"] < 150, (name, mode)
    both = lambda name: sorted(map(len, fx.cases[name]["both_strands"]["assembled"]), reverse=True)
    assert both("a_windows_k13") == [60, 60, 30, 15] and both("b_windows_k32") == [100, 100, 60, 40]
    assert both("h_word_edges") == [65, 64, 63, 33, 32, 31] and both("g_single") == [13]
    assert both("f_no_overlaps") == [13] * 300 and fx.cases["f_no_overlaps"]["one_strand"]["assembled"] == fx.cases["f_no_overlaps"]["kmers"]
    assert both("d_two_bubbles") == [200] * 4 and both("e_three_bubbles") == [200] * 8
    assert fx.cases["c_palindromes_k12"]["k"] % 2 == 0 and sum(s == R.revcomp(s) for s in fx.cases["c_palindromes_k12"]["kmers"]) >= 2
    # the live reference, one strand: fragments
    assert len(fx.cases["a_windows_k13"]["one_strand"]["assembled"]) > 4


def test_the_indexed_round_is_the_round_of_the_definition(fx):
    rng = random.Random(7)
    seq = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    g = seq(300)
    lists = [[g[i:i + 13] for i in range(0, 40)] + [g[5:18], g[5:18]],                                     # a chain, one string at three positions
             [g[0:60], g[10:40], g[0:20], g[40:60], g[50:80], g[50:63], g[13:60]],                         # inside, prefix, suffix, t == |a|
             [u + u + u[:12] for u in [seq(20)]] + [seq(30)],                                               # a string that overlaps at two starts
             [seq(13) for _ in range(40)], [g[0:13]]]
    u = seq(6)
    lists.append([(u * 6)[:30], (u * 6)[2:32], (u * 6)[:18]])                                               # periodic: several starts match one b
    for c in ("a_windows_k13", "c_palindromes_k12"):
        km = fx.cases[c]["kmers"]
        lists.append(km + [R.revcomp(s) for s in km])
    for lst in lists:
        k1 = len(min(lst, key=len)) - 1
        for m in {k1, 12, 11} if k1 >= 12 else {k1}:
            assert R.round_indexed(lst, m) == R.round_bruteforce(lst, m), (lst[:3], m)
        assert R.contained_flags(lst) == R.round_bruteforce(lst, k1)[1], lst[:3]
    pairs, contained = R.round_bruteforce(lists[1], 12)
    assert (2, 0, 20) in pairs and (0, 3, 20) in pairs and (5, 4, 13) in pairs and contained == [False, True, True, True, False, True, True]
    assert R.round_bruteforce([g[0:13], g[0:13]], 12) == ([(0, 1, 13), (1, 0, 13)], [False, False])       # equal strings: a pair, not a containment


def test_restatement_reproduces_the_reference_on_every_golden_case(fx, restated):
    for name, k, kmers, both, ref in fx.runs():
        seqs, rounds = restated[(name, both)]
        assert R.canonical_set(seqs) == R.canonical_set(ref), (name, both)
        assert sorted(map(len, seqs)) == sorted(map(len, ref)), (name, both)
        assert len(R.canonical_set(seqs)) == len(seqs), (name, both)                                    # no sequence twice, on either strand
        assert seqs == sorted(seqs, key=lambda s: (-len(s), s)), (name, both)
        assert rounds == 0 if name in ("f_no_overlaps", "g_single") else rounds > 0, (name, both)
        if not both:                                                                                    # one strand: every sequence is spelt by the input's own k-mers
            assert all(s[i:i + k] in set(kmers) for s in seqs for i in range(len(s) - k + 1)), name


def test_the_canonical_set_does_not_depend_on_the_input_order(fx, restated):
    rng = random.Random(11)
    for name, k, kmers, both, ref in fx.runs():
        shuffled = list(kmers)
        rng.shuffle(shuffled)
        seqs, _ = R.assemble(shuffled, k, both)
        assert seqs == restated[(name, both)][0], (name, both)          # the port's rule: the same text, not only the same set


def test_restated_caps():
    rng = random.Random(3)
    u = "".join(rng.choice("ACGT") for _ in range(20))
    rep = u + u + u[:12]
    km = sorted({min(rep[i:i + 13], R.revcomp(rep[i:i + 13])) for i in range(len(rep) - 12)})
    with pytest.raises(R.CapExceeded, match="PSK_ASM_MAX_LEN=256: a string of round"):
        R.assemble(km, 13, True, max_len=256)
    chain = [u[i:i + 13] for i in range(3)]
    assert R.assemble(chain, 13, max_strings=3, max_pairs=2, max_len=15) == ([u[:15]], 2)
    for kw, text in ((dict(max_strings=2), "PSK_ASM_MAX_STRINGS=2: the list of round 0 has 3 strings"), (dict(max_pairs=1), "PSK_ASM_MAX_PAIRS=1: round 0 has 2 overlapping pairs"),
                     (dict(max_len=14), "PSK_ASM_MAX_LEN=14: a string of round 2 has 15 bases")):
        with pytest.raises(R.CapExceeded) as e:
            R.assemble(chain, 13, **kw)
        assert str(e.value) == text


class _Pheno:
    def __init__(self, name, kmers):
        self.name, self.ML = name, {"kmers": list(kmers)}


def test_assembly_writes_the_references_fasta(tmp_path, monkeypatch, capfd, fx, restated):
    from phenotypeseeker_amd import assembly
    os.chdir(tmp_path)
    for knob in ("PSK_ASM_BOTH_STRANDS", "PSK_ASM_MAX_STRINGS", "PSK_ASM_MAX_PAIRS", "PSK_ASM_MAX_LEN"):
        monkeypatch.delenv(knob, raising=False)
    a, h = fx.cases["a_windows_k13"], fx.cases["h_word_edges"]
    phenos = [_Pheno("Pheno", a["kmers"]), _Pheno("MIC", h["kmers"])]
    assert assembly.run(R.Engine(), phenos, 13) == ["assembled_kmers_Pheno.fasta", "assembled_kmers_MIC.fasta"]
    err = capfd.readouterr().err
    assert err == ("\x1b[1;32mAssembling the k-mers used in modeling of: \x1b[0m\n\x1b[1;32m\tPheno data.\x1b[0m\n\x1b[1;32m\tMIC data.\x1b[0m\n")
    for ph, name in ((phenos[0], "a_windows_k13"), (phenos[1], "h_word_edges")):
        seqs = restated[(name, False)][0]
        lines = open("assembled_kmers_%s.fasta" % ph.name).read().split("\n")
        assert lines[-1] == "" and lines[0:-1:2] == [">seq_%d_length_%d" % (i + 1, len(s)) for i, s in enumerate(seqs)] and lines[1:-1:2] == seqs
        assert [len(s) for s in seqs] == sorted(map(len, seqs), reverse=True)
    # PSK_ASM_BOTH_STRANDS: the list as the reference's code is written to build it
    for value, both in (("1", True), ("0", False)):
        monkeypatch.setenv("PSK_ASM_BOTH_STRANDS", value)
        assembly.run(R.Engine(), phenos[:1], 13)
        assert open("assembled_kmers_Pheno.fasta").read() == R.fasta_text(restated[("a_windows_k13", both)][0])
    assert [len(s) for s in restated[("a_windows_k13", True)][0]] == [60, 60, 30, 15]
    capfd.readouterr()


def test_the_three_cases_without_an_assembly_warn_and_write_nothing(tmp_path, capfd, fx):
    from phenotypeseeker_amd import assembly
    os.chdir(tmp_path)
    ph = [_Pheno("Pheno", fx.cases["g_single"]["kmers"])]
    for kw, needle in ((dict(pca=True), "--pca"), (dict(model_stage=False), "-jt PCA")):
        assert assembly.run(R.Engine(), ph, 13, **kw) == []
        err = capfd.readouterr().err
        assert err.startswith("\x1b[1;33m-a/--assembly: ") and err.endswith("no file is written.\x1b[0m\n") and needle in err
    assert assembly.run(R.Engine(), [], 13) == []
    assert "no phenotype is left to analyse" in capfd.readouterr().err
    assert os.listdir(tmp_path) == []


def test_a_cap_is_a_warning_and_no_file(tmp_path, monkeypatch, capfd, fx):
    from phenotypeseeker_amd import assembly
    from phenotypeseeker_amd._lib import PskError
    os.chdir(tmp_path)
    monkeypatch.setenv("PSK_ASM_MAX_LEN", "50")          # on both strands case a reaches 60 bases; a single k-mer stays a k-mer
    monkeypatch.setenv("PSK_ASM_BOTH_STRANDS", "1")
    phenos = [_Pheno("Long", fx.cases["a_windows_k13"]["kmers"]), _Pheno("Short", fx.cases["g_single"]["kmers"])]
    assert assembly.run(R.Engine(), phenos, 13) == ["assembled_kmers_Short.fasta"]
    err = capfd.readouterr().err
    assert "\x1b[1;33m-a/--assembly of Long stopped at a cap, no file is written: " in err and "PSK_ASM_MAX_LEN=50: a string of round" in err
    assert os.listdir(tmp_path) == ["assembled_kmers_Short.fasta"]

    class Broken:
        def assemble(self, *a):
            raise PskError("psk_assemble failed (-3): hipMemcpy failed", code=-3)
    with pytest.raises(PskError):                        # any other error is fatal, as elsewhere
        assembly.run(Broken(), phenos, 13)
    with pytest.raises(ValueError):
        assembly.assemble(R.Engine(), ["ACGT"], 13)


class _HostEngine(R.Engine):
    """The assembly from the restatement, the logistic fits from scikit-learn on the CPU."""

    def __init__(self, device=0):
        pass

    def close(self):
        pass

    def logreg_l1_fit(self, X, y, folds, fit_param, fit_fold, tol, max_iter):
        from sklearn.linear_model import LogisticRegression
        coef, icpt = np.zeros((len(fit_param), X.shape[1])), np.zeros(len(fit_param))
        for j, (C, f) in enumerate(zip(fit_param, fit_fold)):
            tr = np.asarray(folds) != f
            m = LogisticRegression(penalty="l1", solver="liblinear", C=C, tol=tol, max_iter=max_iter).fit(X[tr], np.asarray(y)[tr])
            coef[j], icpt[j] = m.coef_[0], m.intercept_[0]
        return coef, icpt, np.ones(len(fit_param), dtype=np.int32)


def _write_run(fx):
    kmers = fx.cases["a_windows_k13"]["kmers"]
    rng = np.random.default_rng(2)
    n = 24
    y = np.arange(n) % 2
    X = (rng.random((n, len(kmers))) < 0.3).astype(int)
    X[:, :10] = y[:, None]                        # ten columns carry the phenotype: a model, and under --pca a component, to find
    with open("data.pheno", "w") as f:
        f.write("ID\tAddresses\tPheno\n" + "".join("S%02d\tS%02d.fasta\t%d\n" % (i, i, y[i]) for i in range(n)))
    with open("Pheno_MLdf.csv", "w") as f:
        f.write(",".join([""] + kmers + ["weights", "phenotype"]) + "\n")
        for i in range(n):
            f.write(",".join(["S%02d" % i] + [str(v) for v in X[i]] + ["1", str(y[i])]) + "\n")
    return kmers


def test_modeling_with_and_without_the_knob(tmp_path, monkeypatch, capfd, fx, restated):
    """`modeling -jt modelling -a` end to end on the host: without PSK_ASM today's warning, byte for byte, and no file; with it
    the FASTA of the model's k-mers; -jt PCA and a cap write nothing and the run ends normally."""
    pytest.importorskip("sklearn")
    from test_host_modeling import _args
    from phenotypeseeker_amd import modeling as M
    os.chdir(tmp_path)
    _write_run(fx)
    monkeypatch.setattr(M, "PskContext", _HostEngine)
    for knob in ("PSK_ASM", "PSK_ASM_BOTH_STRANDS", "PSK_ASM_MAX_LEN", "WORLD_SIZE", "RANK"):
        monkeypatch.delenv(knob, raising=False)
    fasta = "assembled_kmers_Pheno.fasta"
    for value in (None, "0"):
        if value is not None:
            monkeypatch.setenv("PSK_ASM", value)
        M.modeling(_args(["-jt", "modelling", "-a"]))
        err = capfd.readouterr().err
        assert err.count(SKIPPED) == 1 and "Assembling" not in err and not os.path.exists(fasta)
        assert err.endswith(SKIPPED + "\n\x1b[1;1;101m######          PhenotypeSeeker modeling finished          ######\x1b[0m\n")
    monkeypatch.setenv("PSK_ASM", "1")
    M.modeling(_args(["-jt", "modelling"]))                                      # the knob without -a changes nothing
    assert "ssembl" not in capfd.readouterr().err and not os.path.exists(fasta)
    M.modeling(_args(["-jt", "modelling", "-a"]))
    err = capfd.readouterr().err
    assert SKIPPED not in err and "\x1b[1;32mAssembling the k-mers used in modeling of: \x1b[0m\n\x1b[1;32m\tPheno data.\x1b[0m\n" in err
    assert open(fasta).read() == R.fasta_text(restated[("a_windows_k13", False)][0])
    assert os.path.exists("log_reg_model_Pheno.pkl")
    monkeypatch.setenv("PSK_ASM_BOTH_STRANDS", "1")
    M.modeling(_args(["-jt", "modelling", "-a"]))
    assert open(fasta).read() == R.fasta_text(restated[("a_windows_k13", True)][0])
    os.remove(fasta)
    monkeypatch.setenv("PSK_ASM_MAX_LEN", "40")                                  # both strands reach 60 bases
    capfd.readouterr()
    M.modeling(_args(["-jt", "modelling", "-a"]))
    err = capfd.readouterr().err
    assert "stopped at a cap, no file is written" in err and "PSK_ASM_MAX_LEN=40" in err and not os.path.exists(fasta)
    assert err.endswith("PhenotypeSeeker modeling finished          ######\x1b[0m\n") and os.path.exists("summary_of_log_reg_analysis_Pheno.txt")
    monkeypatch.delenv("PSK_ASM_MAX_LEN")
    M.modeling(_args(["-jt", "PCA", "-a"]))
    err = capfd.readouterr().err
    assert "-jt PCA" in err and "no file is written" in err and not os.path.exists(fasta)
    monkeypatch.delenv("PSK_ASM")
    M.modeling(_args(["-jt", "PCA", "-a"]))
    assert capfd.readouterr().err.count(SKIPPED) == 1
    M.phenotypes.pred_scale = "binary"


def test_pca_has_no_assembly(tmp_path, monkeypatch, capfd, fx):
    """--pca: the model's columns are components; the warning says so and the model's own files are written."""
    pytest.importorskip("sklearn")
    import pca_restated
    from test_host_modeling import _args
    from phenotypeseeker_amd import modeling as M

    class Engine(_HostEngine, pca_restated.Engine):
        pass
    os.chdir(tmp_path)
    _write_run(fx)
    monkeypatch.setattr(M, "PskContext", Engine)
    monkeypatch.setenv("PSK_ASM", "1")
    monkeypatch.setenv("PSK_PCA", "1")
    M.modeling(_args(["-jt", "modelling", "-a", "--pca"]))
    err = capfd.readouterr().err
    assert "-a/--assembly: with --pca" in err and not os.path.exists("assembled_kmers_Pheno.fasta")
    assert os.path.exists("PCs_and_coefficients_in_log_reg_model_Pheno.txt")


def test_abi_names_the_assembly_entry_points():
    from phenotypeseeker_amd import _lib
    with open(os.path.join(ROOT, "include", "psk.h")) as f:
        header = f.read()
    assert "---- f15:" in header
    for name in ("psk_asm_round", "psk_assemble"):
        assert name in _lib.exported_names() and hasattr(_lib.load(), name)
        decl = header.split("int %s(psk_ctx *ctx" % name)[1].split(");")[0]
        assert decl.count(",") + 1 == len(_lib._SIGNATURES[name][1]), name


def test_pack_strings_is_the_librarys_layout():
    from phenotypeseeker_amd.engine import pack_strings
    words, off, lens = pack_strings(["ACGT", "T" * 32, "C" + "A" * 32, "acgu"])
    assert list(off) == [0, 1, 2, 4] and list(lens) == [4, 32, 33, 4] and words.dtype == np.uint64
    assert [int(w) for w in words] == [0x1B << 56, (1 << 64) - 1, 1 << 62, 0, 0x1B << 56]
    with pytest.raises(ValueError):
        pack_strings(["ACGN"])


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_host_header_against_character_strings(tmp_path, sanitize):
    cxx = _hipcc()
    exe = os.path.join(tmp_path, "asm_host_check")
    flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall"] + flags + [os.path.join(ROOT, "tests", "asm_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " checks, 0 failures" in r.stdout and not r.stderr, (r.stdout[-500:], r.stderr[-2000:])
