"""CPU: tests/spectrum_model.py -- the yardstick of the spectrum kernel -- against a derivation that never sees a CIGAR (the
three text lines of an alignment) on the reference's own report of t001 / HD and on every item of the three CIGAR fixtures
whose ladder has a tract; every clause of the rule on crafted items; tredparse_amd/spectrum.py on hand-made tables; the
parser."""
import os
import re

import numpy as np
import pytest

from tredparse_amd import tred as tredmod
from tredparse_amd.spectrum import ClassSpectrum, RepeatSpectrum, code_word, word_code
from tredparse_amd.ssw import PyAlignRes

from . import cigar_model as cm
from . import cigar_rowpar_model as rm
from . import pileup_model as pm
from . import spectrum_model as sm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M, I, D = 0, 1, 2


def op(n, code):
    return n << 4 | code


def test_the_report_of_t001_cigar_against_text():
    """Each of the 25 blocks: words and touched units from (stand-in read, fields, the operations of Cigar_string) equal
    those from the block's alignment lines, strand and `Reference begin`."""
    from tredparse_amd.meta import TREDsRepo
    hd = TREDsRepo(ref="hg38")["HD"]
    P, p, S = len(hd.prefix), len(hd.repeat), len(hd.suffix)
    with open(os.path.join(GOLD, "alignments_t001_HD.txt")) as fp:
        blocks = pm.parse_blocks(fp.read())
    assert len(blocks) == 25
    words_seen = 0
    for b in blocks:
        assert len(b["target"]) == P + p * b["units"] + S
        r_line, _, q_line = b["lines"]
        f = b["fields"]
        tail = re.search(r"(\d+)S$", b["cigar_string"])
        read = "G" * f[3] + q_line.replace(" ", "") + "T" * (int(tail.group(1)) if tail else 0)
        by_cigar = sm.item_units(P, p, S, 2 * (b["units"] - 1) + b["strand"], read, f, pm.cigar_ops(b["cigar_string"]))
        by_text = sm.from_lines(P, p, S, b["units"], b["strand"], f[1], r_line, q_line)
        assert by_cigar == by_text, b["id"]
        words_seen += len(by_cigar[0])
        if b["tag"] == "FULL":
            assert by_cigar[1] == b["units"] == 15 and len(by_cigar[0]) >= 13
    assert words_seen > 300


@pytest.mark.parametrize("which", ["sw_cigar", "sw_cigar_scorings", "sw_cigar_long"])
def test_every_fixture_item_cigar_against_text(which):
    g = {"sw_cigar": cm.golden, "sw_cigar_scorings": cm.golden_scorings, "sw_cigar_long": rm.golden_long}[which]()
    seen, n_words, n_items = set(), 0, 0
    for k in range(len(g["reads"])):
        lad, tpl = int(g["ladder"][k]), int(g["template"][k])
        prefix, repeat, suffix, mu = g["ladders"][lad]
        if mu <= 0:
            continue
        ref, read, ops = g["refs"][k], g["reads"][k], g["ops"][k]
        P, p, S = len(prefix), len(repeat), len(suffix)
        assert len(ref) == P + p * (tpl // 2 + 1) + S
        r_line, _, q_line = PyAlignRes(g["fields"][k], read, ref, ops).alignment
        by_cigar = sm.item_units(P, p, S, tpl, read, g["fields"][k], ops)
        by_text = sm.from_lines(P, p, S, tpl // 2 + 1, tpl % 2, g["fields"][k][1], r_line, q_line)
        assert by_cigar == by_text, (which, k)
        assert len(by_cigar[0]) <= by_cigar[1] <= tpl // 2 + 1
        seen |= {(tpl % 2, v & 15) for v in ops}
        n_words += len(by_cigar[0])
        n_items += 1
    assert seen == {(s, o) for s in (0, 1) for o in (0, 1, 2)} and n_items > 50 and n_words > n_items


# ---- crafted items: P = 4, S = 6 (a swapped flank would show), CAG ---------------------------------------------------
P_, S_ = "ACGT", "TTGCAA"


def units(read, tpl, ref_begin, ops, read_begin=0, repeat="CAG"):
    on_ref = sum(v >> 4 for v in ops if v & 15 != I)
    on_read = sum(v >> 4 for v in ops if v & 15 != D)
    f = [0, ref_begin, ref_begin + on_ref - 1, read_begin, read_begin + on_read - 1]
    return sm.item_units(len(P_), len(repeat), len(S_), tpl, read, f, ops)


def test_m_runs_around_a_unit_boundary():
    # template of 4 units: ACGT CAG CAG CAG CAG TTGCAA; the read begins on column 4 (unit 0)
    read = "CAGCAACCGCAG"
    assert units(read, 6, 4, [op(6, M)]) == (["CAG", "CAA"], 2)                 # ends on the boundary
    assert units(read, 6, 4, [op(5, M)]) == (["CAG"], 2)                        # one before: unit 1 touched, not clean
    assert units(read, 6, 4, [op(7, M)]) == (["CAG", "CAA"], 3)                 # one after: unit 2 touched
    assert units(read, 6, 4, [op(12, M)]) == (["CAG", "CAA", "CCG", "CAG"], 4)


def test_insertion_on_a_boundary_and_inside_a_unit():
    read = "CAGTTCAACCG"
    assert units(read, 6, 4, [op(3, M), op(2, I), op(6, M)]) == (["CAG", "CAA", "CCG"], 3)        # on the boundary: both clean
    read = "CAGCTTAACCG"
    assert units(read, 6, 4, [op(4, M), op(2, I), op(5, M)]) == (["CAG", "CCG"], 3)               # inside unit 1


def test_deletion_inside_a_unit():
    read = "CAGCGCCG"
    assert units(read, 6, 4, [op(4, M), op(1, D), op(4, M)]) == (["CAG", "CCG"], 3)
    # a deletion of a whole unit: touched, never clean
    assert units("CAGCCG", 6, 4, [op(3, M), op(3, D), op(3, M)]) == (["CAG", "CCG"], 3)


def test_starts_mid_unit_or_lies_in_a_flank():
    assert units("AGCAACC", 6, 5, [op(7, M)]) == (["CAA"], 3)                   # columns 5..11: unit 0 and 2 cut
    assert units("ACG", 6, 0, [op(3, M)]) == ([], 0)                            # prefix only
    assert units("TGCAA", 6, 17, [op(5, M)]) == ([], 0)                         # suffix only
    assert units("GTC", 6, 2, [op(3, M)]) == ([], 1)                            # one tract column
    assert units("xxCAGCAG", 6, 4, [op(6, M)], read_begin=2) == (["CAG", "CAG"], 2)     # a soft clip counts nowhere


def test_n_in_a_word_and_lower_case():
    assert units("CAGCNGcag", 6, 4, [op(9, M)]) == (["CAG", "CNG", "CAG"], 3)
    lad = [(P_, "CAG", S_, 4)]
    spec, items, status = sm.spectrum(lad, ["CAGCNGCAA"], [0], [6], [[0, 4, 12, 0, 8]], [[op(9, M)]], [1], [0], 1, [0], 1)
    assert not status.any() and list(items[0]) == [2, 1, 3]
    assert list(spec[0, sm.BINS:]) == [3, 1, 3, 1] and spec[0, word_code("CAG")] == 1 and spec[0, word_code("CAA")] == 1
    assert spec[0, :sm.BINS].sum() == 2


def test_both_strands_with_different_flanks():
    """The reverse-complement template of 3 units: TTGCAA CTG CTG CTG ACGT (rc(S) first).  A read CTGCGGTTG on its columns
    6..14 shows, forward, CAA CCG CAG on units 0..2."""
    assert pm.revcomp(P_ + "CAG" * 3 + S_) == "TTGCAA" + "CTG" * 3 + "ACGT"
    assert units("CTGCGGTTG", 5, 6, [op(9, M)]) == (["CAA", "CCG", "CAG"], 3)
    # two columns earlier -- where the tract would begin if rc(P), 4 letters, came first -- the read is out of frame: own
    # columns 4..12 are forward 14..6, units 1 and 2 whole, and their words are the complements of TTG and GCG backwards
    assert units("CTGCGGTTG", 5, 4, [op(9, M)]) == (["AAC", "CGC"], 3)
    # own columns 3..8: forward 10..15 = the last tract column... rc(S) has 6 letters, so own 6 is forward column 12
    assert units("CAACTG", 5, 3, [op(6, M)]) == (["CAG"], 1)
    # an insertion before own column 9 is on the forward boundary of units 1 | 2
    assert units("CTGAACTGCTG", 5, 6, [op(3, M), op(2, I), op(6, M)]) == (["CAG", "CAG", "CAG"], 3)
    # N stays N on the reverse strand
    assert units("CTGCNG", 5, 6, [op(6, M)]) == (["CNG", "CAG"], 2)


@pytest.mark.parametrize("period", [1, 2, 3, 4, 5, 6])
def test_periods_one_to_six(period):
    repeat = "CAGTTA"[:period]
    read = repeat * 2 + "G" * period + repeat
    want = [repeat, repeat, "G" * period, repeat]
    assert units(read, 6, 4, [op(4 * period, M)], repeat=repeat) == (want, 4)
    rc = pm.revcomp(read)
    assert units(rc, 7, len(S_), [op(4 * period, M)], repeat=repeat) == (want, 4)
    lad = [(P_, repeat, S_, 4)]
    spec, items, status = sm.spectrum(lad, [read], [0], [6], [[0, 4, 4 + 4 * period - 1, 0, 4 * period - 1]],
                                      [[op(4 * period, M)]], [1], [0], 1, [0], 1)
    assert not status.any() and list(items[0]) == [4, 3, 4] and spec[0, word_code(repeat)] == 3
    assert spec[0, 4 ** period:sm.BINS].sum() == 0 and spec[0, :sm.BINS].sum() == 4


def test_refusals_of_the_model():
    lad = [(P_, "CAG", S_, 4), (P_, "CAGCAGCAGCAA", S_, 2), ("ACGTACGT", "A", "", 0)]
    ok = dict(ladders=lad, n_groups=3, group_ladder=[0, 1, 2], cap=2, read_len=6, lad=0, tpl=2, fields=[0, 4, 9, 0, 5],
              ops=[op(6, M)], n_ops=1, group=0)
    assert sm.status_of(**ok) == sm.OK
    assert sm.status_of(**dict(ok, group=1)) == sm.BAD_ITEM                     # another ladder than the group's
    assert sm.status_of(**dict(ok, lad=2, tpl=0, group=2, fields=[0, 0, 5, 0, 5])) == sm.BAD_ITEM       # no tract
    assert sm.status_of(**dict(ok, lad=1, group=1)) == sm.PERIOD                # period 12
    assert sm.status_of(**dict(ok, lad=1, group=0)) == sm.BAD_ITEM              # the ladder check comes first
    assert sm.status_of(**dict(ok, read_len=2049)) == sm.TOO_LONG
    assert sm.status_of(**dict(ok, lad=1, group=1, n_ops=0)) == sm.BAD_ITEM     # what validate refuses comes first


# ---- tredparse_amd/spectrum.py ------------------------------------------------------------------------------------------
def test_codes_and_words():
    assert word_code("A") == 0 and word_code("CAG") == 1 * 16 + 0 * 4 + 2 and word_code("TTTTTT") == 4095
    assert word_code("CNG") is None and word_code("cag") == word_code("CAG")
    assert all(word_code(code_word(c, 4)) == c for c in (0, 1, 77, 255))


def _row(words, with_n=0, touched=0, reads=0):
    row = np.zeros(sm.STRIDE, np.int32)
    for w, n in words.items():
        row[word_code(w)] = n
    row[sm.BINS:] = [sum(words.values()) + with_n, with_n, touched, reads]
    return row


def test_class_spectrum_on_hand_made_tables():
    c = ClassSpectrum("CAG", _row({"CAG": 90, "CCG": 6, "CAA": 6, "TTT": 1}, with_n=2, touched=120, reads=5),
                      [[20, 20, 24], [20, 18, 24], [23, 23, 24], [20, 13, 24], [20, 16, 24]])
    assert (c.reads, c.units, c.with_n, c.touched) == (5, 103, 2, 120)
    assert c.purity == 90 / 103 and c.interrupted_reads == 3
    assert list(c.words.items()) == [("CAG", 90), ("CAA", 6), ("CCG", 6), ("TTT", 1)]       # falling count, then the word
    assert c.to_dict() == {"interrupted_reads": 3, "purity": 90 / 103, "reads": 5, "touched": 120, "units": 103, "with_n": 2,
                           "words": {"CAG": 90, "CAA": 6, "CCG": 6, "TTT": 1}}
    assert list(c.to_dict()) == sorted(c.to_dict())
    empty = ClassSpectrum("CAG", _row({}, with_n=1, touched=3, reads=2), np.zeros((2, 3), np.int32))
    assert empty.purity is None and empty.units == 0 and empty.words == {} and empty.interrupted_reads == 0
    pure = ClassSpectrum("CAG", _row({"CAG": 7}, reads=1, touched=8), [[7, 7, 8]])
    assert pure.purity == 1.0 and pure.interrupted_reads == 0 and pure.words == {"CAG": 7}
    none = ClassSpectrum("CAG", _row({"CAA": 7}, reads=1, touched=8), [[7, 0, 8]])
    assert none.purity == 0.0 and none.interrupted_reads == 1


def test_repeat_spectrum_to_dict():
    tables = {"rept": (_row({"CAG": 3}, reads=1, touched=3), [[3, 3, 3]]), "full:15": (_row({}), []),
              "partial": (_row({"CAG": 1, "CAA": 1}, reads=1, touched=2), [[2, 1, 2]])}
    r = RepeatSpectrum("CAG", tables)
    d = r.to_dict()
    assert (d["motif"], d["period"]) == ("CAG", 3) and list(d["classes"]) == ["full:15", "partial", "rept"]
    assert d["classes"]["partial"]["interrupted_reads"] == 1 and d["classes"]["full:15"]["purity"] is None
    assert "unsupported" not in d and r.unsupported is False
    u = RepeatSpectrum("CAGCAGCAGCAA")
    assert u.to_dict() == {"motif": "CAGCAGCAGCAA", "period": 12, "unsupported": True} and u.classes == {}
    import json
    assert json.loads(json.dumps(d, sort_keys=True)) == d


def test_the_parser_sets_nothing_else():
    p_ = tredmod.set_argparse()
    base = ["x.bam", "--tred", "HD"]
    a, plain = p_.parse_args(base + ["--spectrum"]), p_.parse_args(base)
    assert a.spectrum is True and plain.spectrum is False
    assert {k: v for k, v in vars(a).items() if k != "spectrum"} == {k: v for k, v in vars(plain).items() if k != "spectrum"}
    from tredparse_amd.runtime import _options
    arg = ("k", "x.bam", None, ["HD"], 300, False, False, True, True, "INFO")
    o = _options(arg + (False, False, False, True))
    assert o["spectrum"] is True and not (o["alignments"] or o["consensus"] or o["consensus_partial"])
    assert _options(arg)["spectrum"] is False and _options(arg + (True, True, True))["spectrum"] is False
