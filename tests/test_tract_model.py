"""tests/tract_model.py against itself: the lemma that lets the kernels look at a seed's predecessor alone, the perfect scan
as the special case without gaps, and the two tracts the feature exists for."""
import numpy as np

from . import scan_model as sm
from . import tract_model as tm

ALPHABETS = ("AC", "ACG", "ACGT", "ACN")
ALL_ON = (2, 2, 2, 2, 2, 2)


def by_predecessor(letters, min_copies, seed_copies, max_gap):
    """tract_model.tracts_segment with a seed's predecessor in its period's list as its only possible partner: what
    csrc/tract.hip does."""
    s = sm.codes_of(letters).astype(np.int16)
    out = []
    for p, seeds in sorted(tm.seeds_of(letters, min_copies, seed_copies).items()):
        runs = []                          # [first seed, last seed, seeds, mismatches]
        for k, seed in enumerate(seeds):
            if k and tm.linked(s, p, seeds[k - 1], seed, max_gap[p - 1]):
                b1, a0 = seeds[k - 1][0] + seeds[k - 1][1], runs[-1][0][0]
                runs[-1][1] = seed
                runs[-1][2] += 1
                runs[-1][3] += sum(1 for x in range(b1, seed[0]) if s[x] != s[a0 + (x - a0) % p])
            else:
                runs.append([seed, seed, 1, 0])
        for first, last, n, mismatch in runs:
            length = last[0] + last[1] - first[0]
            if length // p >= min_copies[p - 1]:
                out.append((first[0], length, p, n, mismatch))
    return sorted(out, key=lambda r: (r[0], r[2]))


def test_all_pairs_components_equal_predecessor_chains():
    rng = np.random.default_rng(20240611)
    tracts = multi = 0
    for case in range(3000):
        letters = tm.planted(rng, ALPHABETS[case % 4])
        mc, sc, mg = tm.random_params(rng)
        want = tm.tracts_segment(letters, mc, sc, mg)
        assert by_predecessor(letters, mc, sc, mg) == want, (letters, mc, sc, mg)
        tracts += len(want)
        multi += sum(1 for r in want if r[3] >= 2)
    assert tracts >= 3000 and multi >= 300, (tracts, multi)        # (the cases do join seeds)


def test_without_gaps_the_tracts_are_the_scan():
    rng = np.random.default_rng(7)
    for case in range(1000):
        letters = tm.planted(rng, ALPHABETS[case % 4])
        mc = [int(rng.integers(2, 7)) if rng.random() < 0.9 else 0 for _ in range(6)]
        if not any(mc):
            mc[2] = 3
        got = tm.tracts_segment(letters, mc, mc, (0,) * 6)
        assert [r[:3] for r in got] == sm.scan_segment(letters, mc)
        assert all(r[3] == 1 and r[4] == 0 for r in got)


def test_fmr1_shaped_tract():
    """(CGG)9 AGG (CGG)9 AGG (CGG)10 is 90 letters; the perfect scan cuts it into 27 / 29 / 32 (9, 9 and 10 copies).  Where
    the letter behind it is a C -- as in the flank the figures of the design note were taken with -- the last piece and the
    tract are one letter longer: 27 / 29 / 33 (9, 9 and 11 copies) and 91."""
    assert len(tm.FMR1) == 90
    assert [r[1] for r in sm.scan_segment(tm.FMR1, ALL_ON) if r[2] == 3] == [27, 29, 32]
    assert [r for r in tm.tracts_segment(tm.FMR1) if r[2] == 3] == [(0, 90, 3, 3, 2)]
    assert [r[1] for r in sm.scan_segment(tm.FMR1 + "CT", ALL_ON) if r[2] == 3] == [27, 29, 33]
    assert [r[1] // 3 for r in sm.scan_segment(tm.FMR1 + "CT") if r[2] == 3] == [9, 9, 11]
    assert [r for r in tm.tracts_segment(tm.FMR1 + "CT") if r[2] == 3] == [(0, 91, 3, 3, 2)]
    mc = list(sm.MIN_COPIES)
    mc[2] = 10                                                     # one step higher: two of the scan's three pieces vanish
    assert len([r for r in sm.scan_segment(tm.FMR1 + "CT", mc) if r[2] == 3]) == 1
    assert [r for r in tm.tracts_segment(tm.FMR1 + "CT", mc) if r[2] == 3] == [(0, 91, 3, 3, 2)]
    flanked = "ATTGCA" + tm.FMR1.lower() + "TCATGA"               # codes, not bytes
    assert (6, 90, 3, 3, 2) in tm.tracts_segment(flanked)


def test_sca1_shaped_tract():
    """(CAG)12 CAT CAG CAT (CAG)15 is 90 letters: two tracts at the defaults (the gap is 7 letters), one with max_gap 7 and
    seed_copies 4 for period 3.  Between a G and CA -- a flank like the design note's -- the tract is 93 letters."""
    assert len(tm.SCA1) == 90
    got = [r for r in tm.tracts_segment(tm.SCA1) if r[2] == 3]
    assert got == [(0, 38, 3, 1, 0), (45, 45, 3, 1, 0)]
    assert [r[:3] for r in got] == [r for r in sm.scan_segment(tm.SCA1) if r[2] == 3]
    sc, mg = list(tm.SEED_COPIES), list(tm.MAX_GAP)
    sc[2], mg[2] = 4, 7
    assert tm.rule_violation(sm.MIN_COPIES, sc, mg) is None
    assert [r for r in tm.tracts_segment(tm.SCA1, sm.MIN_COPIES, sc, mg) if r[2] == 3] == [(0, 90, 3, 2, 2)]
    assert [r for r in tm.tracts_segment("TG" + tm.SCA1 + "CAT", sm.MIN_COPIES, sc, mg) if r[2] == 3] == [(1, 93, 3, 2, 2)]


def test_lone_unit_is_not_absorbed():
    hd = "CAG" * 12 + "CAACAG" + "CCG" * 8                         # the known limit: the CAG behind CAA is no seed
    got = [r for r in tm.tracts_segment(hd) if r[2] == 3]
    assert got[0] == (0, 38, 3, 1, 0) and got[0][0] + got[0][1] <= 39


def test_every_scan_record_lies_in_one_tract():
    rng = np.random.default_rng(99)
    checked = 0
    for case in range(1000):
        letters = tm.planted(rng, ALPHABETS[case % 4])
        mc, sc, mg = tm.random_params(rng)
        tracts = tm.tracts_segment(letters, mc, sc, mg)
        for a, length, p in sm.scan_segment(letters, mc):
            inside = [t for t in tracts if t[2] == p and t[0] <= a and a + length <= t[0] + t[1]]
            assert len(inside) == 1, (letters, mc, sc, mg, (a, length, p))
            checked += 1
    assert checked >= 500


def test_rules():
    d = (sm.MIN_COPIES, tm.SEED_COPIES, tm.MAX_GAP)
    assert tm.rule_violation(*d) is None
    assert tm.rule_violation((10, 6, 5, 4, 4, 4), (5, 3, 3, 3, 3, 3), (4, 2, 3, 4, 5, 6)) is None      # 5 > 4 + 0
    assert "seed_copies * p" in tm.rule_violation((10, 6, 5, 4, 4, 4), (5, 3, 3, 3, 3, 3), (5, 2, 3, 4, 5, 6))
    assert "seed_copies * p" in tm.rule_violation((0, 0, 5, 0, 0, 0), (0, 0, 3, 0, 0, 0), (0, 0, 5, 0, 0, 0))      # 9 > 5 + 4 fails
    assert tm.rule_violation((0, 0, 5, 0, 0, 0), (9, 9, 3, 9, 9, 9), (-1, 99, 4, 0, 0, 0)) is None    # off periods are ignored
    assert "seed_copies <=" in tm.rule_violation((10, 6, 5, 4, 4, 4), (5, 3, 6, 3, 3, 3), tm.MAX_GAP)
    assert "max_gap" in tm.rule_violation((10, 6, 5, 4, 4, 4), (5, 3, 3, 3, 3, 3), (1, 2, 3, 4, 5, 65))
    assert "max_gap" in tm.rule_violation((10, 6, 5, 4, 4, 4), (5, 3, 3, 3, 3, 3), (-1, 2, 3, 4, 5, 6))
    assert tm.rule_violation((1, 6, 5, 4, 4, 4), tm.SEED_COPIES, tm.MAX_GAP) and tm.rule_violation((0,) * 6, tm.SEED_COPIES, tm.MAX_GAP)
