"""`-a/--assembly` of `phenotypeseeker modeling` (the reference's assembling, modeling.py:1607-1622, and its call, :1700-1707):
the k-mers of every analysed phenotype's model assembled into longer sequences by the engine (psk_assemble) and written as
assembled_kmers_<phenotype>.fasta.

Behind PSK_ASM=1; without it modeling.py prints its warning and skips the option.  The reference as it runs assembles one
strand only -- kmers_for_ML, whose reverse complements its list is written to take (:1572), is set to {} (:585) and never
filled --; PSK_ASM_BOTH_STRANDS=1 assembles the list as the code is written, with the reverse complement of every k-mer behind it.
The order of the file is the engine's rule (include/psk.h, f15): longest first, lexicographically among equal lengths."""
import sys

from . import _lib, formats
from ._lib import PSK_ERANGE, PskError

GREEN = "\x1b[1;32m%s\x1b[0m"
YELLOW = "\x1b[1;33m%s\x1b[0m\n"


def _err(text):
    sys.stderr.write(text)
    sys.stderr.flush()


def assemble(engine, kmers, k, both_strands=False):
    """The sequences of the k-mer strings `kmers` (all of k bases), in the file's order."""
    kmers = list(kmers)
    if any(len(km) != int(k) for km in kmers):
        raise ValueError("every k-mer must have %d bases" % int(k))
    seqs, _ = engine.assemble([formats.kmer_to_word(km) for km in kmers], int(k), bool(both_strands))
    return seqs


def fasta_text(seqs):
    """(:1619-1621)"""
    return "".join(">seq_%d_length_%d\n%s\n" % (i + 1, len(s), s) for i, s in enumerate(seqs))


def run(engine, phenos, k, pca=False, model_stage=True):
    """What `-a` does under PSK_ASM=1, on rank 0, after the model stage: `phenos` are the analysed phenotypes (their .name and
    their .ML["kmers"], the columns of <pheno>_MLdf.csv in its order).  Returns the names of the files written."""
    if not model_stage:
        _err(YELLOW % "-a/--assembly: no model stage ran (-jt PCA), so there are no model k-mers to assemble; no file is written.")
        return []
    if pca:
        _err(YELLOW % "-a/--assembly: with --pca the model's columns are principal components, not k-mers; no file is written.")
        return []
    phenos = list(phenos)
    if not phenos:
        _err(YELLOW % "-a/--assembly: no phenotype is left to analyse; no file is written.")
        return []
    both = _lib.env_flag("PSK_ASM_BOTH_STRANDS")
    _err(GREEN % "Assembling the k-mers used in modeling of: " + "\n")
    written = []
    for ph in phenos:
        _err("\x1b[1;32m\t" + ph.name + " data.\x1b[0m\n")
        try:
            seqs = assemble(engine, ph.ML["kmers"], k, both)
        except PskError as e:
            if e.code != PSK_ERANGE:
                raise
            _err(YELLOW % ("-a/--assembly of %s stopped at a cap, no file is written: %s" % (ph.name, e)))
            continue
        path = "assembled_kmers_" + ph.name + ".fasta"
        with open(path, "w") as f:
            f.write(fasta_text(seqs))
        written.append(path)
    return written
