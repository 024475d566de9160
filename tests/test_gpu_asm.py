"""GPU tests (-m gpu) of the k-mer assembly (csrc/asm.hip): psk_asm_round against the restated round of tests/asm_restated.py
-- integers, so the sorted pair triples and the contained flags must be EQUAL -- on lists that reach every place the kernel can
go wrong (more strings than a wave and than a workgroup, one bucket of 200 strings, strings that end at, before and past a
32-base word with matches starting at offsets 0, 1, 31, 32 and 33, prefix / suffix / interior containment, t == |a|, k = 32,
equal strings at two positions, periodic strings whose suffixes match at several starts, no overlap at all, one string);
the pair cap; psk_assemble on every golden case in both strand modes against the reference's record; a tandem repeat ended by
the length cap; and `modeling -a` end to end."""
import os
import random

import numpy as np
import pytest

import asm_restated as R
from helpers import load_dataset
from test_host_modeling import _write_dataset

pytestmark = pytest.mark.gpu


def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _lists():
    """name -> (strings, min_olap)"""
    rng = random.Random(19)
    g = _seq(rng, 3000)
    out = {}
    out["five"] = ([g[0:13], g[1:14], g[2:15], g[700:713], g[1:14]], 12)
    for n in (257, 1025):                                   # the k-mers of one sequence, shuffled: past one wave, past one workgroup
        km = [g[i:i + 13] for i in range(n)]
        rng.shuffle(km)
        out["chain_%d" % n] = (km, 12)
    # one bucket: 200 strings with the same first 12 bases, of 13 to 82 bases; half of them extend another one (t == |a|, and the
    # shorter lies inside the longer); 20 more strings end in the start of one of them, some in all of it
    head = _seq(rng, 12)
    bucket = [head + _seq(rng, 1 + i % 70) for i in range(100)]
    bucket += [bucket[i] + _seq(rng, 1 + i % 9) for i in range(100)]
    tails = []
    for j in range(20):
        b = bucket[(j * 7) % 200]
        t = len(b) if j % 4 == 0 else 12 + j % (len(b) - 11)
        tails.append(_seq(rng, 10 + j) + b[:t])
    mixed = bucket + tails
    rng.shuffle(mixed)
    out["one_bucket_200"] = (mixed, 12)
    # word boundaries: strings of 31 .. 129 bases; a match that starts at offset o of a (an overlap into b) and a 14-base string
    # inside a at offset o, for o = 0, 1, 31, 32, 33
    edges = []
    for i, n in enumerate((31, 32, 33, 63, 64, 65, 129)):
        a = g[200 * i + 100: 200 * i + 100 + n]
        edges.append(a)
        for o in (0, 1, 31, 32, 33):
            if n - o >= 12:
                edges.append(a[o:] + _seq(rng, 3 + o))      # a[o:] is a prefix of it: t = n - o
            if o + 14 <= n:
                edges.append(a[o:o + 14])                   # inside a at o
        edges.append(a[n - 12:] + _seq(rng, 52))            # the shortest overlap, into a 64-base string
    out["word_edges"] = (edges, 12)
    out["prefix_suffix_interior"] = ([g[0:60], g[0:20], g[40:60], g[20:45], g[0:30], g[0:50]], 12)
    big = _seq(rng, 100)
    k32 = [big[i:i + 32] for i in range(69)]
    out["k32"] = (k32 + [R.revcomp(s) for s in k32], 31)
    out["duplicates"] = ([g[0:13], g[1:14], g[0:13], g[2:15], g[1:14], g[500:520], g[500:520]], 12)
    u = _seq(rng, 6)
    out["periodic"] = ([(u * 12)[:50], (u * 12)[:40], (u * 12)[3:70], _seq(rng, 20) + (u * 3)], 12)
    lone = []
    while len(lone) < 50:
        s = _seq(rng, 13)
        if not R.round_indexed(lone + [s], 12)[0]:
            lone.append(s)
    out["no_overlap"] = (lone, 12)
    out["one_string"] = ([g[0:13]], 12)
    return out


LISTS = _lists()


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    with PskContext(0) as c:
        yield c


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


@pytest.fixture(scope="module")
def restated(fx):
    """The restatement's assembly of every golden case in both modes; computed once."""
    return {(name, both): R.assemble(kmers, k, both)[0] for name, k, kmers, both, _ in fx.runs()}


@pytest.mark.parametrize("name", list(LISTS))
def test_round_equals_the_restated_round(ctx, name):
    strings, m = LISTS[name]
    want_pairs, want_contained = R.round_indexed(strings, m)
    pairs, contained = ctx.asm_round(strings, m)
    got = sorted(map(tuple, pairs.tolist()))
    print("%s: %d strings, %d pairs, %d contained" % (name, len(strings), len(want_pairs), sum(want_contained)))
    assert got == want_pairs
    assert contained.tolist() == want_contained
    # what the list is there for
    if name == "one_bucket_200":
        assert max(sum(s[:12] == t[:12] for s in strings) for t in strings[:1] + [s for s in strings if sum(x[:12] == s[:12] for x in strings) > 128][:1]) >= 200
        assert any(t == len(strings[a]) for a, _, t in want_pairs) and sum(want_contained) >= 100
    if name == "word_edges":
        assert {len(strings[a]) - t for a, _, t in want_pairs} >= {0, 1, 31, 32, 33} and sum(want_contained) >= 25
    if name == "periodic":
        assert (0, 1, 38) in want_pairs and (0, 2, 47) in want_pairs       # the largest of several matching starts
    if name == "duplicates":
        assert (0, 2, 13) in want_pairs and (2, 0, 13) in want_pairs and not any(want_contained[:5])
    if name in ("no_overlap", "one_string"):
        assert not want_pairs and not any(want_contained)
    if name == "prefix_suffix_interior":
        assert want_contained == [False, True, True, True, True, True] and (4, 5, 30) in want_pairs and (1, 0, 20) in want_pairs


def test_pair_cap_reports_the_true_count_and_leaves_the_context_usable(ctx):
    from phenotypeseeker_amd._lib import PskError
    strings, m = LISTS["chain_257"]
    want, _ = R.round_indexed(strings, m)
    assert len(want) == 256
    with pytest.raises(PskError) as e:
        ctx.asm_round(strings, m, pair_cap=len(want) - 1)
    assert e.value.code == -4 and e.value.n_pairs == len(want) and "pair_cap=255" in str(e.value)
    pairs, _ = ctx.asm_round(strings, m, pair_cap=len(want))
    assert sorted(map(tuple, pairs.tolist())) == want
    for bad in (0, 32):
        with pytest.raises(PskError) as e:
            ctx.asm_round(strings, bad)
        assert e.value.code == -1
    with pytest.raises(PskError):
        ctx.asm_round(["ACGTACGT"], 12)                     # shorter than the overlap asked for
    assert ctx.asm_round([], 12)[0].shape == (0, 3)


def test_assemble_reproduces_the_reference_on_every_golden_case(ctx, fx, restated):
    from phenotypeseeker_amd import formats
    for name, k, kmers, both, ref in fx.runs():
        seqs, rounds = ctx.assemble([formats.kmer_to_word(s) for s in kmers], k, both)
        assert R.canonical_set(seqs) == R.canonical_set(ref), (name, both)
        assert len(seqs) == len(ref) and sorted(map(len, seqs)) == sorted(map(len, ref)), (name, both)
        assert seqs == sorted(seqs, key=lambda s: (-len(s), s)), (name, both)
        assert seqs == restated[(name, both)], (name, both)             # the port's rule decides the strand and the order
    assert ctx.assemble([], 13) == ([], 0)
    assert ctx.assemble([formats.kmer_to_word("T" * 32)], 32, True) == (["A" * 32], 0)


def test_a_tandem_repeat_ends_at_the_length_cap(ctx, monkeypatch):
    """The reference never returns from this input; the call does, with the knob's name, and the context goes on working."""
    from phenotypeseeker_amd import formats
    from phenotypeseeker_amd._lib import PskError
    rng = random.Random(5)
    u = _seq(rng, 20)
    rep = u + u + u[:12]
    km = sorted({min(rep[i:i + 13], R.revcomp(rep[i:i + 13])) for i in range(len(rep) - 12)})
    words = [formats.kmer_to_word(s) for s in km]
    monkeypatch.setenv("PSK_ASM_MAX_LEN", "256")
    with pytest.raises(R.CapExceeded, match="PSK_ASM_MAX_LEN=256"):
        R.assemble(km, 13, True, max_len=256)
    with pytest.raises(PskError) as e:
        ctx.assemble(words, 13, True)
    assert e.value.code == -4 and "PSK_ASM_MAX_LEN=256: a string of round" in str(e.value)
    assert ctx.assemble(words[:1], 13, True) == ([min(km[0], R.revcomp(km[0]))], 0)
    for knob, value in (("PSK_ASM_MAX_STRINGS", "3"), ("PSK_ASM_MAX_PAIRS", "2")):
        monkeypatch.delenv("PSK_ASM_MAX_LEN", raising=False)
        monkeypatch.setenv(knob, value)
        with pytest.raises(PskError) as e:
            ctx.assemble(words, 13, True)
        assert e.value.code == -4 and knob + "=" + value + ":" in str(e.value) and "round 0" in str(e.value)
        monkeypatch.setenv(knob, "x")
        with pytest.raises(PskError) as e:
            ctx.assemble(words, 13, True)
        assert e.value.code == -1 and knob in str(e.value)
        monkeypatch.delenv(knob)


def test_modeling_writes_the_fasta_behind_the_knob(tmp_path, monkeypatch):
    from phenotypeseeker_amd import assembly
    from phenotypeseeker_amd.cli import build_parser
    ds = load_dataset("ds_omitB")
    _write_dataset(ds, str(tmp_path))
    os.chdir(tmp_path)

    def run(argv):
        args = build_parser().parse_args(argv)
        args.func(args)
    for knob in ("PSK_ASM_BOTH_STRANDS", "PSK_ASM_MAX_STRINGS", "PSK_ASM_MAX_PAIRS", "PSK_ASM_MAX_LEN"):
        monkeypatch.delenv(knob, raising=False)
    monkeypatch.setenv("PSK_ASM", "1")
    run(["modeling", "data.pheno", "-a", "--omit_B_correction", "--n_kmers", "100"])
    with open("Pheno_MLdf.csv") as f:
        kmers = f.readline().rstrip("\n").split(",")[1:-2]
    assert len(kmers) == 100
    want = assembly.fasta_text(assembly.assemble(R.Engine(), kmers, 13))
    got = open("assembled_kmers_Pheno.fasta").read()
    assert got == want and got.startswith(">seq_1_length_")
    os.remove("assembled_kmers_Pheno.fasta")
    monkeypatch.delenv("PSK_ASM")
    run(["modeling", "data.pheno", "-jt", "modelling", "-a", "--omit_B_correction", "--n_kmers", "100"])
    assert not os.path.exists("assembled_kmers_Pheno.fasta") and os.path.exists("log_reg_model_Pheno.pkl")
