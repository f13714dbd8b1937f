"""CPU: the N-aware 6-mer score cap (kmer_weight / kmer_cap in tredparse_amd/csrc/sw_ladder.hip) against the
oracle's alignments.  For ladders with an N in the motif or the flanks and one without, and for every read and every template
of both strands, the oracle's Smith-Waterman score must not exceed match * (W + 5), W = cnt - ceil(J / 6) from the restated
tables (tests/kmer_weight_model.py).  The bound is reached (slack 0), on the N-free ladder and on a ladder with a class table,
so the check is not vacuous; on the N-free ladder W is the plain count."""
import random

import pytest

from oracle import pyoracle as po

from . import kmer_weight_model as km

OPMD = ("CCAGTCTGAGCGGCGATG", "GGGGCTGCGGGCGGTCGG")      # 18-base flanks of data/treds.json
BPES = ("GCCAGGGCTACCGGGGCC", "CATCTGGCAGGAGGCATA")
HD = ("GAGTCCCTCAAGTCCTTC", "CAACAGCCGCCACCGCCG")
LADDERS = {
    "GCN": (OPMD[0], "GCN", OPMD[1], 20),
    "NGC": (BPES[0], "NGC", BPES[1], 20),
    "N": (OPMD[0], "N", OPMD[1], 60),
    "GCNGCA": (OPMD[0], "GCNGCA", OPMD[1], 10),
    "12mer": (BPES[0], "GCATNCGGATCN", BPES[1], 5),
    "flankN": ("CCAGTCTGANCGGCGATG", "CAG", "GGGGCTGCGGNCGGTCGG", 20),
    "CAG": (HD[0], "CAG", HD[1], 20),                     # N-free
}
SCORINGS = [(1, 5, 7, 2), (2, 10, 12, 3)]                 # min(mismatch, gap_open) >= 5 * match: the bound's premise


def _fill(rng, s):
    return "".join(rng.choice("ACGT") if c == "N" else c for c in s)


def _mutate(rng, s, k):
    s = list(s)
    for i in rng.sample(range(len(s)), k):
        s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
    return "".join(s)


def make_reads(name):
    rng = random.Random("cap " + name)
    prefix, repeat, suffix, mu = LADDERS[name]
    P = len(repeat)
    reads = []
    for units in (2, max(3, 24 // P), max(4, 45 // P)):
        t = prefix + repeat * units + suffix
        for L in (40, 47, 60):
            # substrings across the prefix / repeat boundary, across the repeat / suffix boundary, and (short alleles) both
            starts = {max(0, len(prefix) - L // 2), max(0, len(prefix) + P * units - L // 2), max(0, (len(t) - L) // 2)}
            for s in sorted(starts):
                sub = t[s:s + L]
                if len(sub) < 40:
                    continue
                reads.append(_fill(rng, sub))                       # a real read: the template's N filled in
                reads.append(km.rc(_fill(rng, sub)))                # ... and from the other strand
                reads.append(_mutate(rng, _fill(rng, sub), rng.randint(1, 3)))
                reads.append(km.rc(_mutate(rng, _fill(rng, sub), rng.randint(1, 3))))
                holding = list(_fill(rng, sub))                     # a read that itself holds N
                for i in rng.sample(range(len(holding)), rng.randint(1, 3)):
                    holding[i] = "N"
                reads.append("".join(holding))
    reads += [_fill(rng, (repeat * 60)[k:k + 50]) for k in (0, 1)]   # inside the repeat
    reads += ["".join(rng.choice("ACGT") for _ in range(rng.randint(40, 60))) for _ in range(8)]
    assert all(40 <= len(r) <= 60 for r in reads)
    return reads


def slacks(name, scoring):
    """[(slack, strand)] over every (read, template) of both strands, after checking the bound."""
    lad = LADDERS[name]
    reads = make_reads(name)
    flag, tables = km.ladder_tables(*lad)
    tt = km.strand_templates(*lad)
    refs = tt[0] + tt[1]
    pr = [i for i in range(len(reads)) for _ in refs]
    pt = [k for _ in reads for k in range(len(refs))]
    pairs = po.sw_pairs(reads, refs, pr, pt, scoring=scoring, threads=2)
    out = []
    for (i, k), row in zip(zip(pr, pt), pairs):
        s = 0 if k < len(tt[0]) else 1
        cnt, J, W = km.read_weight(reads[i], tables[s], with_n=flag)
        if not flag:
            assert J == 0 and W == cnt                              # no class table: the plain count
        cap = scoring[0] * (W + 5)
        assert int(row[0]) <= cap, (name, scoring, reads[i], refs[k], int(row[0]), cnt, J, W)
        out.append((cap - int(row[0]), s))
    return out


@pytest.mark.parametrize("scoring", SCORINGS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(LADDERS))
def test_no_alignment_beats_the_cap(name, scoring):
    got = slacks(name, scoring)
    print(name, scoring, "pairs", len(got), "min slack", min(g[0] for g in got))
    assert min(g[0] for g in got) >= 0


@pytest.mark.parametrize("scoring", SCORINGS, ids=lambda s: "-".join(map(str, s)))
def test_the_cap_is_reached(scoring):
    """An exact substring of an N-free template scores match * L = the cap (W = L - 5); on the ladder with an N in its flanks
    only, a read inside the CAG repeat has no N column under any window (J = 0) and scores match * L as well."""
    assert min(g[0] for g in slacks("CAG", scoring)) == 0
    assert min(g[0] for g in slacks("flankN", scoring)) == 0


def test_the_weight_is_lower_than_the_count_where_it_matters():
    """A forward read of the GCN ladder seen from strand 1: every repeat window is present (rc((GCN)n) = (NGC)n) with two N
    columns under it, so W is about two thirds of the count -- the reads the change is about.  The read: 14 prefix bases and
    46 of (GCA)n, 41 windows inside the repeat; no strand-1 window with fewer than two N spells GCAGCA, CAGCAG or AGCAGC (the
    windows over the flank boundaries begin CC.. or end ..CC / ..CA / ..AT)."""
    lad = LADDERS["GCN"]
    flag, tables = km.ladder_tables(*lad)
    read = (lad[0] + lad[1] * 20)[4:64].replace("N", "A")
    cnt, J, W = km.read_weight(read, tables[1])
    assert flag and cnt >= 41 and J >= 2 * 41 and W <= cnt - 14