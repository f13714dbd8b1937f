"""The tandem-repeat scan's definition (tests/scan_model.py, include/tredscan.h) on fixed strings: what the kernel, the
binding and the site builder are checked against is itself checked here, by hand-worked cases."""
import numpy as np

from . import scan_model as sm

ALL2 = (2, 2, 2, 2, 2, 2)


def _flank(seed, n=300):
    """n letters without any record under the defaults (a fixed seed, checked below)."""
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), n))


def test_piezo1_strings():
    """The reference's PIEZO1 site: prefix + tcc x 8 + suffix between random flanks gives exactly two records: the TCC tract
    -- its 24 letters and the T that continues the period -- and the CTG run of the suffix, which begins on the tract's last
    c (the two runs have the letters 341 and 342 in common)."""
    left, right = _flank(1), _flank(2)
    assert sm.scan_segment(left) == [] and sm.scan_segment(right) == []
    s = left + "AGCCCCTCGTCCCTGGAG" + "tcc" * 8 + "TGCTGCTGCTGCTGATGC" + right
    assert sm.scan_segment(s) == [(318, 25, 3), (341, 15, 3)]
    assert s[318:343].upper() == "TCC" * 8 + "T" and s[341:356].upper() == "CTG" * 5


def test_single_letter_run():
    assert sm.scan_segment("A" * 50) == [(0, 50, 1)]        # periods 2 .. 6 see a motif that is not primitive
    assert sm.scan_segment("A" * 50, ALL2) == [(0, 50, 1)]
    assert sm.scan_segment("A" * 9) == [] and sm.scan_segment("A" * 10) == [(0, 10, 1)]


def test_period_two_only():
    assert sm.scan_segment("AC" * 20) == [(0, 40, 2)]
    assert sm.scan_segment("AC" * 20, ALL2) == [(0, 40, 2)]  # ACAC, ACACAC are not primitive; periods 3 and 5 have no run


def test_n_splits_a_run():
    assert sm.scan_segment("A" * 20 + "N" + "A" * 20) == [(0, 20, 1), (21, 20, 1)]
    assert sm.scan_segment("CAG" * 6 + "N" + "CAG" * 6) == [(0, 18, 3), (19, 18, 3)]
    assert sm.scan_segment("N" * 50) == []                  # N never matches, not even N
    assert sm.scan_segment("A" * 20 + "R" + "A" * 20) == [(0, 20, 1), (21, 20, 1)]   # any other byte is N


def test_lower_case_is_upper_case():
    s = _flank(3, 50) + "cAg" * 7 + _flank(4, 50)
    assert sm.scan_segment(s) == sm.scan_segment(s.upper()) == sm.scan_segment(s.lower()) == [(50, 21, 3)]


def test_short_segments():
    for mc in (sm.MIN_COPIES, ALL2):
        assert sm.scan_segment("", mc) == []
        assert sm.scan_segment("A", mc) == []
        for p in range(1, sm.MAX_PERIOD + 1):
            assert [r for r in sm.scan_segment("ACGTAC"[:p], mc) if r[2] == p] == []      # n <= p: e_p is empty
    assert sm.scan_segment("AA", ALL2) == [(0, 2, 1)]
    assert sm.scan_segment("ACAC", ALL2) == [(0, 4, 2)]
    assert sm.scan_segment("ACACA", ALL2) == [(0, 5, 2)]     # the partial last copy counts into the length


def test_run_to_the_last_letter():
    s = _flank(5, 40) + "GATA" * 5
    assert s[39] == "A" and sm.scan_segment(s) == [(39, 21, 4)]      # (the flank's last letter continues the period)
    assert sm.scan_segment("T" + "GATA" * 5 + "GA") == [(1, 22, 4)]
    assert sm.scan_segment("GATA" * 4) == [(0, 16, 4)]


def test_overlapping_periods_are_all_reported():
    # (AAC) x 6 holds six period-1 runs of two letters inside its one period-3 run
    got = sm.scan_segment("AAC" * 6, ALL2)
    assert (0, 18, 3) in got and [r for r in got if r[2] == 1] == [(k, 2, 1) for k in range(0, 18, 3)]
    assert got == sorted(got, key=lambda r: (r[0], r[2]))


def test_segments_and_order():
    letters = "A" * 30 + "CAG" * 10
    assert sm.scan(letters, [0, 60]) == [(0, 0, 30, 1), (0, 30, 30, 3)]
    assert sm.scan(letters, [0, 15, 30, 30, 60]) == [(0, 0, 15, 1), (1, 0, 15, 1), (3, 0, 30, 3)]
    assert sm.scan(letters, [0, 45, 60]) == [(0, 0, 30, 1), (0, 30, 15, 3), (1, 0, 15, 3)]
    seg, start, length, period = sm.arrays(sm.scan(letters, [0, 45, 60]))
    assert seg.dtype == np.int32 and start.dtype == np.int64 and length.dtype == period.dtype == np.int32
    assert sm.arrays([])[0].shape == (0,)


def test_period_switched_off():
    s = "A" * 30 + "CAG" * 10
    assert sm.scan_segment(s, (0, 6, 5, 4, 4, 4)) == [(30, 30, 3)]
    assert sm.scan_segment(s, (10, 0, 0, 0, 0, 0)) == [(0, 30, 1)]


def test_primitive_and_canonical():
    assert sm.primitive(list("CAG")) and not sm.primitive(list("CACA")) and not sm.primitive(list("AAAAAA"))
    assert not sm.primitive(list("CAGCAG")) and sm.primitive(list("CAGCAA")) and sm.primitive(list("A"))
    assert sm.canonical("CAG") == sm.canonical("CTG") == sm.canonical("gca") == "AGC"
    assert sm.canonical("TCC") == "AGG" and sm.canonical("T") == "A" and sm.canonical("GATA") == "AGAT"
