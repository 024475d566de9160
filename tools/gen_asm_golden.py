#!/usr/bin/env python3
"""Records tests/golden/asm_kat.json from the reference's own assembler (PhenotypeSeeker/modeling.py:1526-1605): the known
answers of psk_assemble and of tests/asm_restated.py.  Run in the build container only (it imports the unmodified reference
through oracle/ref_shim.py); inputs and recorded outputs are committed, no reference text.

The reference's five assembler methods (ReverseComplement, string_set, overlap, pick_overlaps, kmer_assembler) are bound to a
stub object that carries what they read: ML_df.columns (the k-mers + two more columns) and kmers_for_ML.  Every case runs in
two modes: kmers_for_ML empty -- the reference as it executes, :585 sets it to {} and nothing fills it -- and kmers_for_ML
filled with the k-mers, as the comment at :1570 intends (the reverse complement of every k-mer joins the list).  The k-mers
are canonical (the smaller of a k-mer and its reverse complement), as the package's are, in a seeded random order that stands
for the p-value order.  Each run's wall time is recorded.

Cases:
  a_windows_k13     windows of 15, 30 and 60 bases of a random genome and a SNP variant of the 60-base one, k = 13
  b_windows_k32     the same with windows of 40, 60 and 100 bases, k = 32
  c_palindromes_k12 k = 12 (even: a k-mer can be its own reverse complement): three 50/52-base windows, two with a palindromic
                    12-mer in the middle (where the two strands cross: four paths per window; two palindromes in ONE
                    window would let a path switch strands for ever) and one with the tandem AACGTTAACG, whose 10 bases of
                    a 6-base period repeat no 11-mer, so nothing cycles
  d_two_bubbles     a 200-base region and its variant with two SNPs 80 bases apart: 4 haplotype paths, k = 13
  e_three_bubbles   the same with three SNPs 50 bases apart: 8 paths
  f_no_overlaps     300 random 13-mers, no two of which (nor their reverse complements) overlap by 12
  g_single          one 13-mer
  h_word_edges      windows of 31, 32, 33, 63, 64 and 65 bases, k = 13: contigs that end at, before and past a 32-base word
No case holds a repeat: the reference does not terminate on one.
usage: tools/gen_asm_golden.py"""
import json
import os
import random
import signal
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import asm_restated as R  # noqa: E402

METHODS = ("ReverseComplement", "string_set", "overlap", "pick_overlaps", "kmer_assembler")


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def snp(seq, at):
    return seq[:at] + {"A": "C", "C": "G", "G": "T", "T": "A"}[seq[at]] + seq[at + 1:]


def canonical_kmers(seqs, k, rng):
    """The distinct canonical k-mers of the sequences, shuffled."""
    out = sorted({min(s[i:i + k], R.revcomp(s[i:i + k])) for s in seqs for i in range(len(s) - k + 1)})
    rng.shuffle(out)
    return out


def windows(rng, lengths):
    genome = rand_seq(rng, 4000)
    out, at = [], 100
    for n in lengths:
        out.append(genome[at:at + n])
        at += n + 300
    return out


def cases():
    rng = random.Random(20240611)
    w = windows(rng, (15, 30, 60))
    yield "a_windows_k13", 13, canonical_kmers(w + [snp(w[2], 30)], 13, rng)
    w = windows(rng, (40, 60, 100))
    yield "b_windows_k32", 32, canonical_kmers(w + [snp(w[2], 50)], 32, rng)
    w = [rand_seq(rng, 20) + mid + rand_seq(rng, 20) for mid in ("GATTACGTAATC", "TGCAGATCTGCA", "AACGTTAACG")]
    palindromes = [sum(s[i:i + 12] == R.revcomp(s[i:i + 12]) for i in range(len(s) - 11)) for s in w]
    assert palindromes == [1, 1, 0], palindromes      # one strand crossing per contig at most: two in one contig would make a cycle
    yield "c_palindromes_k12", 12, canonical_kmers(w, 12, rng)
    region = rand_seq(rng, 200)
    yield "d_two_bubbles", 13, canonical_kmers([region, snp(snp(region, 60), 140)], 13, rng)
    region = rand_seq(rng, 200)
    yield "e_three_bubbles", 13, canonical_kmers([region, snp(snp(snp(region, 50), 100), 150)], 13, rng)
    lone = []
    while len(lone) < 300:
        km = rand_seq(rng, 13)
        km = min(km, R.revcomp(km))
        trial = lone + [km]
        both = trial + [R.revcomp(s) for s in trial]
        if km not in lone and km != R.revcomp(km) and not R.round_indexed(both, 12)[0]:
            lone.append(km)
    yield "f_no_overlaps", 13, lone
    yield "g_single", 13, [min(s, R.revcomp(s)) for s in [rand_seq(rng, 13)]]
    yield "h_word_edges", 13, canonical_kmers(windows(rng, (31, 32, 33, 63, 64, 65)), 13, rng)


def reference_run(M, kmers, k, filled):
    stub = types.SimpleNamespace()
    for name in METHODS:
        setattr(stub, name, types.MethodType(getattr(M.phenotypes, name), stub))
    stub.ML_df = types.SimpleNamespace(columns=list(kmers) + ["weights", "phenotype"])
    stub.kmers_for_ML = list(kmers) if filled else {}
    M.Samples.kmer_length = str(k)
    t0 = time.time()
    signal.alarm(240)          # the reference does not end on every input: a case that takes this long is not a fixture
    out = stub.kmer_assembler()
    signal.alarm(0)
    return {"assembled": list(out), "seconds": round(time.time() - t0, 3)}


def main():
    import ref_shim
    M = ref_shim.load_modeling()
    doc = {"reference": "PhenotypeSeeker/modeling.py:1526-1605 through oracle/ref_shim.py", "python_hash_seed": os.environ.get("PYTHONHASHSEED", "random"),
           "cases": []}
    for name, k, kmers in cases():
        rec = {"name": name, "k": k, "kmers": kmers}
        for mode, filled in (("one_strand", False), ("both_strands", True)):
            rec[mode] = reference_run(M, kmers, k, filled)
            print("%-18s k=%2d %4d k-mers %-12s -> %3d sequences, lengths %s%s  (%.1f s)"
                  % (name, k, len(kmers), mode, len(rec[mode]["assembled"]), sorted(map(len, rec[mode]["assembled"]), reverse=True)[:8],
                     "..." if len(rec[mode]["assembled"]) > 8 else "", rec[mode]["seconds"]), flush=True)
        doc["cases"].append(rec)
    path = os.path.join(ROOT, "tests", "golden", "asm_kat.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
