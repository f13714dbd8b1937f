"""CPU: the SW / classification oracle against the reference's golden vectors (and, in the build
container, against the reference's own ssw.c compiled into oracle/_ref)."""
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as po

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGNUM = {"": 0, "FULL": 1, "PREF": 2, "POST": 3, "REPT": 4, "HANG": 5}


@pytest.fixture(scope="module")
def sw_gold():
    z = np.load(os.path.join(GOLD, "sw_pairs.npz"))
    return ([str(x) for x in z["reads"]], [str(x) for x in z["refs"]], z["pair_read"], z["pair_ref"],
            z["result"].astype(np.int32), tuple(int(x) for x in z["scoring"]))


def test_oracle_matches_reference_golden_pairs(sw_gold):
    reads, refs, pr, pt, want, scoring = sw_gold
    assert len(pr) >= 45000
    got = po.sw_pairs(reads, refs, pr, pt, scoring=scoring, threads=8)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (got[bad[:3]], want[bad[:3]])
    # the set is not trivial: long reads, N reads, both strands, zero-score sentinels
    assert (want[:, 0] == 0).any() and (want[:, 0] > 100).any()


def test_ladder_model_matches_reference_golden_pairs(sw_gold):
    """The kernel's algorithm (shared-prefix ladder + one-pass begin coordinates) on the CPU."""
    reads, refs, pr, pt, want, scoring = sw_gold
    loci = {l["name"]: l for l in json.load(open(os.path.join(GOLD, "..", "..", "tredparse_amd", "data", "treds.json")))["loci"]}
    # recover (read, ladder) groups: templates of one ladder are contiguous in refs, fwd/rc interleaved
    by_read = {}
    for k, (r, t) in enumerate(zip(pr, pt)):
        by_read.setdefault(int(r), []).append(k)
    checked = 0
    for r, ks in list(by_read.items())[::7]:
        tmpl = [refs[pt[k]] for k in ks]
        mu = len(tmpl) // 2
        locus = next(l for l in loci.values()
                     if l["prefix"] + l["repeat"] + l["suffix"] == tmpl[0])
        got = po.ladder_model(reads[r], locus["prefix"], locus["repeat"], locus["suffix"], mu, scoring)
        assert np.array_equal(got, want[ks]), (r, locus["name"])
        checked += len(ks)
    assert checked > 5000


RANDOM_SCORINGS = ((2, 2, 3, 1), (1, 4, 6, 1))        # other scorings the ABI accepts


def random_pairs():
    """Random repeat-locus (read, template) pairs, every read against every template."""
    rng = np.random.default_rng(5)
    reads, refs = [], []
    for _ in range(60):
        L = int(rng.choice([30, 75, 150, 151, 250]))
        base = "".join("ACGT"[i] for i in rng.integers(0, 4, 40))
        rep = "".join("ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(1, 7))))
        ref = base[:18] + rep * int(rng.integers(1, 60)) + base[18:36]
        ref = ref[:400]
        a = int(rng.integers(0, max(1, len(ref) - 20)))
        read = list((ref[a:] + base * 10)[:L])
        for i in rng.integers(0, L, int(rng.integers(0, 8))):
            read[i] = "ACGTN"[int(rng.integers(0, 5))]
        read = "".join(read)
        reads.append(read if rng.random() < 0.5 else po.rc(read))
        refs.append(ref)
    pr = [i for i in range(len(reads)) for _ in range(len(refs))]
    pt = [j for _ in range(len(reads)) for j in range(len(refs))]
    return reads, refs, pr, pt


def random_answers(sw_pairs):
    """{name: (score, ref_begin, ref_end, read_begin, read_end) per pair} of random_pairs() under the default scoring
    and a slice of them under RANDOM_SCORINGS, by sw_pairs (po.sw_pairs or po.ref_sw_pairs).  tools/gen_golden.py
    stores the reference's in tests/golden/sw_random.npz."""
    reads, refs, pr, pt = random_pairs()
    out = {"default": sw_pairs(reads, refs, pr, pt, threads=8)}
    for scoring in RANDOM_SCORINGS:
        out["scoring_" + "_".join(map(str, scoring))] = sw_pairs(reads[:20], refs[:20], pr[:400], [j % 20 for j in pt[:400]],
                                                                  scoring=scoring)
    return out


def test_oracle_matches_compiled_reference_random():
    """The restatement against the compiled reference's answers on random pairs: the stored ones (tests/golden/
    sw_random.npz), and -- where oracle/_ref is built -- the live ones, which must still be the stored ones."""
    want = dict(np.load(os.path.join(GOLD, "sw_random.npz")))
    if po.have_ref():
        live = random_answers(po.ref_sw_pairs)
        assert set(live) == set(want) and all(np.array_equal(live[k], want[k]) for k in want)
    got = random_answers(po.sw_pairs)
    assert set(got) == set(want) and len(want["default"]) == 3600
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# the scorings the long-read kernel's GPU tests run (tools/fuzz_long.py, tests/test_long_sw_shapes_gpu.py) beyond the three
# pinned above; the last three are corners of the range the kernels accept
LONG_SCORINGS = ((1, 1, 2, 1), (3, 5, 7, 2), (1, 0, 1, 1), (1, 9, 12, 3), (8, 16, 16, 16), (8, 0, 1, 1), (1, 16, 16, 1))
LONG_SEED = 20270308
HD = ("GAGTCCCTCAAGTCCTTC", "CAG", "CAACAGCCGCCACCGCCG")      # tredparse_amd/data/treds.json


def long_pairs(k):
    """Eight long (read, template) pairs for LONG_SCORINGS[k]: reads of 513 and 1 025 letters against HD templates of
    600 ... 4 095 columns on either strand.  Suffix, prefix and inside-repeat reads with a few errors, a pure repeat, a
    two-letter read (many cells share the best score), a read with N runs and a random one."""
    rng = np.random.default_rng(LONG_SEED + k)
    pre, rep, suf = HD
    rnd = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    reads, refs = [], []
    cols = [int(c) for c in rng.permutation([600, 700, 1000, 1400, 2047, 2048, 3000, 4095])]
    for j, kind in enumerate(("suffix", "prefix", "inside", "pure", "two", "nruns", "random", "suffix")):
        L = (513, 1025)[j % 2]
        units = (cols[j] - len(pre) - len(suf)) // 3
        t = pre + rep * units + suf
        assert 600 <= len(t) <= 4095
        g = rnd(L) + t + rnd(L)
        if kind in ("suffix", "prefix", "inside", "nruns"):
            a = {"suffix": L + len(t) - L // 3, "prefix": L // 3, "inside": L + len(pre) + 4,
                 "nruns": L + int(rng.integers(0, len(t) - L // 2))}[kind]
            r = list(g[a:a + L])
            for i in rng.integers(0, L, L // 100):
                r[i] = "ACGT"[int(rng.integers(4))]
            if kind == "nruns":
                for i in rng.integers(0, L - 30, 3):
                    r[i:i + 30] = "N" * 30
            r = "".join(r)
        elif kind == "pure":
            r = (rep * L)[1:L + 1]
        elif kind == "two":
            r = "".join("AG"[i] for i in rng.integers(0, 2, L))
        else:
            r = rnd(L)
        assert len(r) == L
        turn = bool(rng.integers(2))
        reads.append(po.rc(r) if turn else r)
        refs.append(po.rc(t) if j % 3 == 2 else t)
    return reads, refs


def long_answers(sw_pairs, scorings=LONG_SCORINGS):
    """{scoring: (score, ref_begin, ref_end, read_begin, read_end) per pair of long_pairs} by sw_pairs (po.sw_pairs or
    po.ref_sw_pairs).  tools/gen_golden.py stores the reference's in tests/golden/sw_long_pairs.npz."""
    out = {}
    for k, scoring in enumerate(LONG_SCORINGS):
        if scoring in scorings:
            reads, refs = long_pairs(k)
            out["scoring_" + "_".join(map(str, scoring))] = sw_pairs(reads, refs, list(range(8)), list(range(8)), scoring=scoring,
                                                                      threads=8)
    return out


def test_oracle_matches_compiled_reference_long_pairs():
    """The restatement against the compiled reference on long pairs at the seven scorings that only the long-read kernel's
    GPU tests use, where those tests lean on the restatement alone: the stored answers (tests/golden/sw_long_pairs.npz),
    and -- where oracle/_ref is built -- the live ones, which must still be the stored ones.  A pair on which the
    reference's CIGAR pass faults (REF_CRASHED) is left out; at most a quarter of a scoring's pairs may be.

    gap_open == gap_extend: the reference's 16-bit pass leaves its lazy-F loop one row early there (ssw.c:472-477: once
    the loop has raised H(i) to F, `F - gap_extend > H(i) - gap_open` is false and it stops, so the vertical gap never
    reaches row i + 1 across a segment boundary), its 8-bit pass tests the next row and does not.  A truncated F only ever
    lowers cells, so at those scorings the reference's score may fall short of the recurrence's, never exceed it: such a
    pair counts as left out as well, within the same quarter (stored: one pair of eight at 8/0/1/1, 2 665 against 2 667;
    none at 1/0/1/1 and 8/16/16/16).  The kernels and this restatement compute the recurrence in full."""
    want = dict(np.load(os.path.join(GOLD, "sw_long_pairs.npz")))
    assert set(want) == {"scoring_" + "_".join(map(str, s)) for s in LONG_SCORINGS}
    if po.have_ref():
        live = long_answers(po.ref_sw_pairs)
        assert set(live) == set(want) and all(np.array_equal(live[k], want[k]) for k in want)
    got = long_answers(po.sw_pairs)
    for scoring in LONG_SCORINGS:
        k = "scoring_" + "_".join(map(str, scoring))
        ok = want[k][:, 0] != po.REF_CRASHED
        if scoring[2] == scoring[3]:
            ok &= want[k][:, 0] >= got[k][:, 0]
        print(k, "left out:", int((~ok).sum()), "of", len(ok))
        assert want[k].shape == (8, 5) and (~ok).sum() <= 2, k
        assert (want[k][ok, 0] >= 255).any(), k        # the reference's 16-bit pass took part
        assert np.array_equal(got[k][ok], want[k][ok]), (k, got[k], want[k])


# tools/fuzz_parity.py seed 20271201, round 334: a 300-base (CTG)n read with a few errors against the DM1 ladder
FAULT_READ = ("TGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCCGCTGCTGCT"
              "GCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTG"
              "CTGCTGCCGGTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTGCTNCTGCTGCTGCTGCTCCTGCTGCTGCTGCGGG")
FAULT_LADDER = ("GCCCGGCCTGGCCACCGC", "CTG", "CGGGGGCCCCGAGCCGCC", 100)
FAULT_OTHER = "GCCCGGCCTGGCCACCGC" + "CTG" * 20 + "CGGGGGCCCCGAGCCGCC"


def fault_answers(classify, sw_pairs):
    """The fault case's answers by classify / sw_pairs (po.ref_classify and po.ref_sw_pairs, or the restatement's):
    {cls: (tag, h, score) of [other, read, other] under scoring 1/3/2/2, pairs: the read against every template and the
    neighbour against one, default: (tag, h, score) of the read under the default scoring}.  tools/gen_golden.py stores
    the reference's in tests/golden/sw_fault.npz."""
    ls = po.LocusSet([FAULT_LADDER])
    zero = np.zeros(3, np.int32)
    return {"cls": classify([FAULT_OTHER, FAULT_READ, FAULT_OTHER], zero, ls, scoring=(1, 3, 2, 2), threads=1),
            "pairs": sw_pairs([FAULT_READ, FAULT_OTHER], ls.templates, [0] * len(ls.templates) + [1],
                              list(range(len(ls.templates))) + [38], scoring=(1, 3, 2, 2), threads=1),
            "default": classify([FAULT_READ], zero[:1], ls, threads=1)}


def test_reference_fault_in_its_cigar_pass_is_reported_not_fatal():
    """tools/fuzz_parity.py seed 20271201, round 334: a 300-base (CTG)n read with a few errors against the DM1 ladder under
    scoring 1/3/2/2 makes the reference's banded_sw (ssw.c:549-633) run off its buffers.  The driver reports the pair
    as REF_CRASHED and the read as tag -1, the neighbours are unaffected, and the restatement -- which has no CIGAR
    pass -- still answers.  The reference's answers are the stored ones (tests/golden/sw_fault.npz) or, where oracle/_ref
    is built, its live ones."""
    ref = fault_answers(po.ref_classify, po.ref_sw_pairs) if po.have_ref() else dict(np.load(os.path.join(GOLD, "sw_fault.npz")))
    mine = fault_answers(po.classify, po.sw_pairs)
    cls = ref["cls"]
    if cls[1, 0] >= 0:
        pytest.skip("this build of the reference survives the input")
    assert cls[1, 0] == -1 and np.array_equal(cls[[0, 2]], mine["cls"][[0, 2]]) and mine["cls"][1, 0] > 0
    pairs = ref["pairs"]
    assert (pairs[:-1, 0] == po.REF_CRASHED).any() and pairs[-1, 0] == 96 and np.array_equal(pairs[-1], mine["pairs"][-1])
    # under the default scoring the same read goes through
    assert ref["default"][0, 0] >= 0 and np.array_equal(ref["default"], mine["default"])


def test_oracle_classification_matches_reference_golden():
    """(tag, h) per read and the FULL/PREF/REPT histograms of bam_parser._parseReadSW + tally_counts."""
    cases = json.load(open(os.path.join(GOLD, "classify.json")))["cases"]
    loci = {l["name"]: l for l in json.load(open(os.path.join(GOLD, "..", "..", "tredparse_amd", "data", "treds.json")))["loci"]}
    for case in cases:
        l = loci[case["locus"]]
        ls = po.LocusSet([(l["prefix"], l["repeat"], l["suffix"], case["max_units"])])
        got = po.classify(case["reads"], np.zeros(len(case["reads"]), np.int32), ls, clip=case["clip"], threads=8)
        want = np.asarray([[TAGNUM[t], h] for t, h in case["expected"]], np.int32)
        assert np.array_equal(got[:, :2], want), case["locus"]
        hist = {"FULL": {}, "PREF": {}, "REPT": {}}
        for t, h, _ in got:
            name = {1: "FULL", 2: "PREF", 3: "PREF", 4: "REPT"}.get(int(t))
            if name:
                hist[name][str(int(h))] = hist[name].get(str(int(h)), 0) + 1
        for name in hist:
            assert hist[name] == case[name], (case["locus"], name)
        assert sum(hist["REPT"].values()) == case["rept"]
