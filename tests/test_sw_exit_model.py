"""The bounded-gain exit of sw_cont_kernel's steady_exit, on the CPU (tests/sw_exit_model.py restates the trunk sweep).

* The bound holds: below every row of every read, no alignment of the rest of the read against any template of the
  strand scores more than G(row) -- the oracle's local alignment of read[row + 1:] (oracle/pyoracle.sw_pairs) is an upper
  bound of what a path through that row can still gain.  For G1 = match * (L - 1 - row), the bound the kernel uses, this
  holds by construction (n letters never score more than match * n): the comparison is kept as a check of the test's own
  indexing.  What it constrains is G2 = match * min(L - 1 - row, 5 + tail windows), the 6-mer tier of the model, which the
  kernel does not hold.
* Exits agree with an unpruned sweep: replaying the kernel's loop with the new test, every read's (tag, units, score) is
  the oracle's classification, which looks at every template -- including reads whose later templates tie the winner's
  score with more units.
"""
import numpy as np
import pytest

from oracle import pyoracle as po

from . import sw_exit_model as xm

SCORING = (1, 5, 7, 2)
LADDERS = {
    "p2": ("GAGTCCCTCAAGTCCTTC", "CA", "TTGACCGGATCCGTAGCA"),
    "p3": ("GAGTCCCTCAAGTCCTTC", "CAG", "CAACAGCCGCCACCGCCG"),
    "p5": ("TGGTTCATCGAGTTTCCA", "ATTCT", "GGCATTAGCCGTTCAAGG"),
    "p12": ("ACCGTTAGCATTCGAGGT", "CGCGGGGCGGGG", "TTAGACCTGAATCGTCAA"),
    "n1": ("CCAGTCTGAGCGGCGATG", "GCN", "GGGGCTGCGGGCGGTCGG"),
    "n2": ("GCCAGGGCTACCGGGGCC", "NGC", "CATCTGGCAGGAGGCATA"),
}


def _junk(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _fill(rng, s):
    return "".join("ACGT"[int(rng.integers(0, 4))] if c == "N" else c for c in s)


def _sub(rng, s, k):
    s = list(s)
    for i in rng.choice(len(s), k, replace=False):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def _indel(rng, s):
    q = int(rng.integers(10, len(s) - 10))
    return (s[:q] + "ACGT"[int(rng.integers(0, 4))] + s[q:-1]) if rng.random() < 0.5 else (s[:q] + s[q + 1:] + "A")


def make_reads(name, L, seed):
    """Reads of every kind for one ladder: PREF, POST, FULL with right flanks of 0, 10, 40 and 100 bases (where the read
    has room), REPT, with substitutions and an indel, one in the other orientation, one random."""
    rng = np.random.default_rng(seed)
    a, rep, b = LADDERS[name]
    p = len(rep)
    out = []
    for flank in (0, 10, 40, 100):
        units = (L - flank - 30) // p
        if units < 2:
            continue
        body = _junk(rng, 200) + _fill(rng, a + rep * units + b) + _junk(rng, 200)
        end = 200 + len(a) + p * units + flank          # the read's right flank: `flank` bases behind the repeat
        out.append(body[end - L:end])
    units = L // p + 3
    hap = _junk(rng, L) + _fill(rng, a + rep * units + b) + _junk(rng, L)
    out.append(hap[L + len(a) - 30:][:L])                 # PREF: runs into the repeat
    out.append(hap[L + len(a) + p * units + len(b) + 12 - L:][:L])   # POST: comes out of it
    out.append(_fill(rng, rep * (L // p + 2))[1:L + 1])   # REPT
    out.append(_sub(rng, out[0], 2))
    out.append(_indel(rng, out[1] if len(out) > 1 else out[0]))
    out.append(po.rc(out[0]))
    out.append(_junk(rng, L))
    return out


CASES = [("p3", 150), ("p2", 100), ("p5", 100), ("p12", 100), ("n1", 100), ("n2", 64)]


@pytest.mark.parametrize("name,L", CASES)
def test_gain_bound_covers_the_oracle(name, L):
    a, rep, b = LADDERS[name]
    mu = -(-L // len(rep))
    reads = make_reads(name, L, 7 + L)
    R = xm.rows_per_lane(L)
    lens = np.asarray([len(r) for r in reads], np.int64)
    codes = np.full((len(reads), 16 * R), 4, np.int64)
    for i, r in enumerate(reads):
        codes[i, :len(r)] = xm.encode(r)
    tables = xm.Tables(a, rep, b, mu)
    slack = [1 << 30, 1 << 30]
    for strand in range(2):
        pa, prep, pb = xm.strand_parts(a, rep, b)[strand]
        tmpl = [pa + prep * u + pb for u in range(1, mu + 1)]
        pres, _ = xm.window_presence(codes, lens, tables, strand)
        g1, g2 = xm.gain_bounds(lens, pres, R, SCORING[0], True)
        assert (g2 <= g1).all()
        tails, owner = [], []
        for i, r in enumerate(reads):
            for row in range(len(r) - 2):
                tails.append(r[row + 1:])
                owner.append((i, row))
        pr = np.repeat(np.arange(len(tails)), mu)
        pt = np.tile(np.arange(mu), len(tails))
        sc = po.sw_pairs(tails, tmpl, pr, pt, scoring=SCORING, threads=4)[:, 0].reshape(len(tails), mu).max(1)
        for (i, row), s in zip(owner, sc):
            assert s <= g2[i, row] <= g1[i, row], (name, strand, i, row, int(s), int(g1[i, row]), int(g2[i, row]), reads[i])
            slack[0] = min(slack[0], int(g1[i, row] - s))
            slack[1] = min(slack[1], int(g2[i, row] - s))
    print(name, L, "reads", len(reads), "smallest slack G1", slack[0], "G2", slack[1])


@pytest.mark.parametrize("name,L", CASES)
def test_exits_agree_with_an_unpruned_sweep(name, L):
    a, rep, b = LADDERS[name]
    lad = (a, rep, b, -(-L // len(rep)))
    reads = make_reads(name, L, 7 + L)
    R = xm.rows_per_lane(L)
    rules = ("none", "old", "tier1", "tier2")
    res = xm.ladder_passes(reads, lad, SCORING, R, rules)
    want = po.classify(reads, np.zeros(len(reads), np.int32), po.LocusSet([lad]), scoring=SCORING, threads=4)
    want = [tuple(int(x) for x in w) for w in want]
    for rule in rules:
        got = [xm.winners(x) for x in res[rule]["best"]]
        assert got == want, (rule, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4])
    cols = {r: res[r]["cols"] for r in rules}
    print(name, L, "trunk columns", cols, "tags", sorted(set(w[0] for w in want)))
    assert cols["tier2"] <= cols["tier1"] <= cols["old"] <= cols["none"]
    assert {xm.TAG_FULL, xm.TAG_PREF} <= set(w[0] for w in want)


def test_a_later_template_with_equal_score_and_more_units_does_not_win():
    """A read that runs from the prefix into the repeat and ends there: every template with at least the read's units
    scores the same; the winner is the first of them under every rule (here the strand exit closes the read: its score is
    its cap), and no rule sweeps more columns than the one before it."""
    a, rep, b = LADDERS["p3"]
    L = 100
    read = ("ACGTTGCA" + a + rep * 40)[:L]                  # 8 junk + 18 prefix + 74 repeat bases: 24 whole units
    lad = (a, rep, b, -(-L // 3))
    st = xm.Strand([read], lad, 0, SCORING, xm.rows_per_lane(L))
    n_rep = (L - 8 - len(a)) // 3
    top = int(st.score[0].max())
    ties = [u for u in range(1, lad[3] + 1) if st.score[0, u] == top]
    assert len(ties) > 3 and ties[0] in (n_rep, n_rep + 1), (ties, n_rep)
    seen = {}
    for rule in ("none", "old", "tier1", "tier2"):
        cols, best, why = xm.replay(st, [0], [-1], rule)
        seen[rule] = (cols, why)
        tag, h, score = xm.winners(best[0])
        assert (h, score) == (ties[0], top) and tag == xm.TAG_PREF, (rule, tag, h, score, ties)
    print(seen)
    assert seen["tier2"][0] <= seen["tier1"][0] <= seen["old"][0] <= seen["none"][0]


TIE_READ = "TATCGGCTACCGCAAAAATAGGAGTCCCTCAAGTCCTTCCAGCAGCAGCAGCCGCAGCAGCAGCAGCAGCAGCAGCAGGAGCAGCAGCAGCAGCAGCAGC"


@pytest.mark.parametrize("strand", (0, 1))
def test_a_tie_that_leaves_through_the_new_test(strand):
    """The same kind of read with two substitutions: its score (67) stays under its cap, so the strand exit does not close it
    and the templates from 20 units on tie.  The wave leaves through the new test (reason 'new'), before the present rule
    would ('steady'), and the winner is the first of the tied templates -- a need() that took bestS where bestS + 1 is due
    would combine the tied templates instead of dropping them, and the new test would never be asked.  strand 1: the reverse
    complement, swept on strand 0 first (nothing to find there), the arg-max word carried over as the device does."""
    a, rep, b = LADDERS["p3"]
    L = 100
    lad = (a, rep, b, -(-L // 3))
    read = TIE_READ if strand == 0 else po.rc(TIE_READ)
    best = [-1]
    if strand == 1:
        st0 = xm.Strand([read], lad, 0, SCORING, xm.rows_per_lane(L))
        _, best, _ = xm.replay(st0, [0], [-1], "tier1")
        assert xm.winners(best[0]) == (0, 0, 0)
    st = xm.Strand([read], lad, strand, SCORING, xm.rows_per_lane(L))
    top = int(st.score[0].max())
    ties = [u for u in range(1, lad[3] + 1) if st.score[0, u] == top]
    assert top == 67 and ties[:3] == [20, 21, 22] and st.cap[0] > top
    seen = {rule: xm.replay(st, [0], list(best), rule) for rule in ("none", "old", "tier1")}
    print({k: (v[0], v[2]) for k, v in seen.items()})
    for rule, (cols, word, why) in seen.items():
        assert xm.winners(word[0])[1:] == (ties[0], top), (rule, xm.winners(word[0]))
    assert seen["tier1"][2] == "new" and seen["old"][2] == "steady" and seen["none"][2] == "end"
    assert seen["tier1"][0] < seen["old"][0] < seen["none"][0]
    # the exit comes after the first tied template was combined and a later one dropped
    assert seen["tier1"][0] >= st.alen + st.period * (ties[0] + 1)
