"""The k-mer assembly of `-a/--assembly` restated in plain Python `str` operations, from its definition (include/psk.h, f15): the
CPU yardstick of psk_asm_round / psk_assemble (csrc/asm.hip, csrc/asm_host.h), the reader of tests/golden/asm_kat.json
(tools/gen_asm_golden.py) and a stand-in for the engine in host tests.

  one round over a list (positions 0 .. n - 1), min_olap = k - 1:
      pair (a, b), a != b as POSITIONS: t = the largest t with min_olap <= t <= min(|a|, |b|) and a[-t:] == b[:t]; pairs with
      such a t are the round's pairs.  contained[b]: b is a substring of a member that differs from it as a STRING.
  the loop: sort the list by (length, text).  Per round: members that are contained leave; the rest are paired; no pair:
      stop; every member in no pair is emitted, in list order, unless its reverse complement has been emitted; the next list is
      the sorted set of all a + b[t:].  At the stop the remaining members are emitted under the same rule.  The output is
      sorted by length, longest first, and by text among equal lengths.
  caps (the engine's knobs, PSK_ERANGE): strings in a round's list (before the contained members leave), pairs in a round
      (among the members that stay), bases in one string.

round_bruteforce is the definition, pair by pair; round_indexed gives the same answer from a dictionary of the members' first
min_olap bases, and contained_flags the same flags from one text search per member (tests/test_asm_host.py holds the three
against each other); the last two serve the loops, whose later rounds merge thousands of strings of which dozens stay."""
import json
import os

_RC = str.maketrans("ACGT", "TGCA")

MAX_STRINGS, MAX_PAIRS, MAX_LEN = 1 << 20, 1 << 22, 65535
ERANGE = -4


def revcomp(s):
    return s.translate(_RC)[::-1]


def canonical_set(seqs):
    """The strand-canonical set of a list of sequences: what does not depend on the order a set is walked in."""
    return {min(s, revcomp(s)) for s in seqs}


def overlap(a, b, min_olap):
    """The largest t with min_olap <= t <= min(|a|, |b|) and a[-t:] == b[:t]; 0 when there is none."""
    for t in range(min(len(a), len(b)), min_olap - 1, -1):
        if a.endswith(b[:t]):
            return t
    return 0


def round_bruteforce(strings, min_olap):
    """(sorted [(a, b, t)], [contained])"""
    n = len(strings)
    pairs = []
    for a in range(n):
        for b in range(n):
            if a != b:
                t = overlap(strings[a], strings[b], min_olap)
                if t:
                    pairs.append((a, b, t))
    contained = [any(strings[b] != s and strings[b] in s for s in strings) for b in range(n)]
    return sorted(pairs), contained


def round_indexed(strings, min_olap):
    """The same result as round_bruteforce: every window of min_olap bases of a is looked up among the members' first min_olap bases."""
    m = min_olap
    heads = {}
    for b, s in enumerate(strings):
        heads.setdefault(s[:m], []).append(b)
    best, contained = {}, [False] * len(strings)
    for a, sa in enumerate(strings):
        for s in range(len(sa) - m + 1):       # ascending: the first start that matches gives the pair's largest t
            tail = sa[s:]
            for b in heads.get(sa[s:s + m], ()):
                sb = strings[b]
                if b == a:
                    continue
                if len(tail) <= len(sb):
                    if sb.startswith(tail):
                        best.setdefault((a, b), len(tail))
                        if len(tail) == len(sb) and sb != sa:
                            contained[b] = True
                elif tail.startswith(sb):
                    contained[b] = True
    return sorted((a, b, t) for (a, b), t in best.items()), contained


def contained_flags(strings):
    """contained[] alone, for the loop's merged lists (tens of thousands of strings, of which hundreds stay).  A string inside a
    different string lies inside a longer one, and then inside one that is itself inside nothing; so the distinct strings are
    taken longest first and each is looked for in the text -- one per line -- of those found inside nothing so far."""
    inside, text = {}, ""
    for s in sorted(set(strings), key=len, reverse=True):
        inside[s] = s in text
        if not inside[s]:
            text += "\n" + s
    return [inside[s] for s in strings]


class CapExceeded(Exception):
    pass


def assemble(kmers, k, both_strands=False, max_strings=MAX_STRINGS, max_pairs=MAX_PAIRS, max_len=MAX_LEN, match=round_indexed):
    """(sequences in the output's order, rounds that merged something)"""
    order = lambda s: (len(s), s)
    lst = sorted(list(kmers) + ([revcomp(s) for s in kmers] if both_strands else []), key=order)
    emitted, seen, rounds, rnd = [], set(), 0, 0

    def offer(s):
        if revcomp(s) not in seen:
            seen.add(s)
            emitted.append(s)

    while lst:
        if len(lst) > max_strings:
            raise CapExceeded("PSK_ASM_MAX_STRINGS=%d: the list of round %d has %d strings" % (max_strings, rnd, len(lst)))
        if max(map(len, lst)) > max_len:
            raise CapExceeded("PSK_ASM_MAX_LEN=%d: a string of round %d has %d bases" % (max_len, rnd, max(map(len, lst))))
        contained = contained_flags(lst)
        lst = [s for s, c in zip(lst, contained) if not c]
        pairs, _ = match(lst, k - 1)
        if len(pairs) > max_pairs:
            raise CapExceeded("PSK_ASM_MAX_PAIRS=%d: round %d has %d overlapping pairs" % (max_pairs, rnd, len(pairs)))
        if not pairs:
            break
        in_pair = {a for a, _, _ in pairs} | {b for _, b, _ in pairs}
        for i, s in enumerate(lst):
            if i not in in_pair:
                offer(s)
        merged = {lst[a] + lst[b][t:] for a, b, t in pairs}
        if max(map(len, merged)) > max_len:
            raise CapExceeded("PSK_ASM_MAX_LEN=%d: a string of round %d has %d bases" % (max_len, rnd + 1, max(map(len, merged))))
        lst = sorted(merged, key=order)
        rounds += 1
        rnd += 1
    for s in lst:
        offer(s)
    return sorted(emitted, key=lambda s: (-len(s), s)), rounds


def fasta_text(seqs):
    return "".join(">seq_%d_length_%d\n%s\n" % (i + 1, len(s), s) for i, s in enumerate(seqs))


def word_to_kmer(w, k):
    return "".join("ACGT"[(int(w) >> (2 * (k - 1 - i))) & 3] for i in range(k))


class Engine:
    """Stands in for PskContext.assemble / asm_round in CPU tests: the same arguments, results and refusals (the caps are read
    from the environment per call, as the library reads them), computed here."""

    def asm_round(self, strings, min_olap, pair_cap=None):
        import numpy as np
        from phenotypeseeker_amd._lib import PskError
        pairs, contained = round_indexed(list(strings), min_olap)
        n = len(strings)
        if len(pairs) > (n * (n - 1) if pair_cap is None else pair_cap):
            e = PskError("psk_asm_round failed (-4): pair_cap=%d: the list has %d overlapping pairs" % (pair_cap, len(pairs)), code=ERANGE)
            e.n_pairs = len(pairs)
            raise e
        return np.array(pairs, dtype=np.int32).reshape(-1, 3), np.array(contained, dtype=bool)

    def assemble(self, kmer_words, k, both_strands=False):
        from phenotypeseeker_amd._lib import PskError
        knob = lambda name, default: int(os.environ.get(name) or default)
        try:
            return assemble([word_to_kmer(w, k) for w in kmer_words], k, both_strands, knob("PSK_ASM_MAX_STRINGS", MAX_STRINGS),
                            knob("PSK_ASM_MAX_PAIRS", MAX_PAIRS), knob("PSK_ASM_MAX_LEN", MAX_LEN))
        except CapExceeded as e:
            raise PskError("psk_assemble failed (-4): %s" % e, code=ERANGE)


class Fixture:
    """tests/golden/asm_kat.json: cases[name] = {k, kmers (in order), one_strand: {assembled, seconds}, both_strands: {...}} --
    `assembled` is the list the reference's kmer_assembler() returned with kmers_for_ML empty / filled."""

    def __init__(self, path=None):
        self.path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "asm_kat.json")
        with open(self.path) as f:
            doc = json.load(f)
        self.meta = {k: v for k, v in doc.items() if k != "cases"}
        self.cases = {c["name"]: c for c in doc["cases"]}
        self.names = [c["name"] for c in doc["cases"]]

    def runs(self):
        """(case name, k, kmers, both_strands, the reference's list) for every case in both modes"""
        for name in self.names:
            c = self.cases[name]
            for mode in ("one_strand", "both_strands"):
                yield name, c["k"], c["kmers"], mode == "both_strands", c[mode]["assembled"]
