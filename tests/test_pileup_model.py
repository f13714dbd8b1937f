"""CPU: tests/pileup_model.py -- the yardstick of the pileup kernel -- against a derivation that never sees a CIGAR (the
three text lines of an alignment), on the reference's own report of t001 / HD and on every item of the three CIGAR
fixtures; and the consensus, tie and interruption rules (the model's and tredparse_amd/consensus.py's) on crafted tables."""
import os
import re

import numpy as np
import pytest

from tredparse_amd.consensus import AlleleConsensus
from tredparse_amd.ssw import PyAlignRes

from . import cigar_model as cm
from . import cigar_rowpar_model as rm
from . import pileup_model as pm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _blocks():
    with open(os.path.join(GOLD, "alignments_t001_HD.txt")) as fp:
        return pm.parse_blocks(fp.read())


def test_the_report_of_t001_cigar_against_text():
    """Each of the 25 blocks: the table from (stand-in read, fields, the operations of Cigar_string) equals the table from
    the block's alignment lines, strand and `Reference begin`."""
    blocks = _blocks()
    assert len(blocks) == 25        # (all on the + strand: the fixtures below have both)
    assert sum(b["tag"] == "FULL" for b in blocks) == 4 and all(b["h"] == 15 for b in blocks if b["tag"] == "FULL")
    for b in blocks:
        L = len(b["target"])
        r_line, _, q_line = b["lines"]
        f = b["fields"]
        # the read: only its aligned letters are in the block; the clipped ends count nowhere, so any letters stand for them
        tail = re.search(r"(\d+)S$", b["cigar_string"])
        clip_end = int(tail.group(1)) if tail else 0
        read = "G" * f[3] + q_line.replace(" ", "") + "T" * clip_end
        assert len(read) - 1 - clip_end == f[4]
        by_cigar, by_text = pm.table(L), pm.table(L)
        pm.add_item(by_cigar, L, b["strand"], read, f, pm.cigar_ops(b["cigar_string"]))
        pm.from_lines(by_text, L, b["strand"], f[1], r_line, q_line)
        assert by_cigar == by_text, b["id"]
        assert sum(sum(row[:5]) for row in by_cigar) == len(q_line.replace(" ", "")) - sum(row[7] for row in by_cigar)
        # the match line's bars are the reads' letters that equal the forward template's
        fwd = pm.revcomp(b["target"]) if b["strand"] else b["target"]
        n_match = b["lines"][1].count("|")
        assert sum(row[pm.channel(fwd[c])] for c, row in enumerate(by_cigar[:L]) if fwd[c] in "ACGT") == n_match


@pytest.mark.parametrize("which", ["sw_cigar", "sw_cigar_scorings", "sw_cigar_long"])
def test_every_fixture_item_cigar_against_text(which):
    g = {"sw_cigar": cm.golden, "sw_cigar_scorings": cm.golden_scorings, "sw_cigar_long": rm.golden_long}[which]()
    n = len(g["reads"])
    seen = set()
    for k in range(n):
        lad, tpl = int(g["ladder"][k]), int(g["template"][k])
        ref, read, ops = g["refs"][k], g["reads"][k], g["ops"][k]
        strand = tpl % 2 if g["ladders"][lad][3] > 0 else 0
        L = len(ref)
        assert L == pm.template_len(g["ladders"][lad], tpl)
        r_line, _, q_line = PyAlignRes(g["fields"][k], read, ref, ops).alignment
        by_cigar, by_text = pm.table(L), pm.table(L)
        pm.add_item(by_cigar, L, strand, read, g["fields"][k], ops)
        pm.from_lines(by_text, L, strand, g["fields"][k][1], r_line, q_line)
        assert by_cigar == by_text, (which, k)
        seen |= {(strand, v & 15) for v in ops}
    assert seen == {(s, op) for s in (0, 1) for op in (0, 1, 2)}, seen


def test_the_fixtures_hold_1116_items():
    assert len(cm.golden()["reads"]) + len(cm.golden_scorings()["reads"]) + len(rm.golden_long()["reads"]) == 1116


def test_strand_mapping_by_hand():
    """ACGTA forward; the read CGT on the reverse-complement template TACGT, columns 1-3, with an insertion of 2 before
    its column 2 and a deletion of its column 3."""
    L = 5
    t = pm.table(L)
    # rc template TACGT; read A + GG + C laid as 1M 2I 1M 1D: columns 1 (A), insertion before 2, column 2 (C), column 3 deleted
    pm.add_item(t, L, 1, "AGGC", [0, 1, 3, 0, 3], [1 << 4, 2 << 4 | 1, 1 << 4, 1 << 4 | 2])
    want = pm.table(L)
    want[3][3] += 1          # rc column 1 -> forward 3, A -> T
    want[3][6] += 1          # insertion before rc column 2 -> before forward 5 - 2
    want[3][7] += 2
    want[2][2] += 1          # rc column 2 -> forward 2, C -> G
    want[1][5] += 1          # rc column 3 -> forward 1, deleted
    assert t == want
    # N stays N, and an insertion behind the last rc column is before forward column 0; on the forward strand it is slot L
    t = pm.table(L)
    pm.add_item(t, L, 1, "NA", [0, 4, 4, 0, 1], [1 << 4, 1 << 4 | 1])
    assert t[0][4] == 1 and t[0][6:] == [1, 1] and sum(map(sum, t)) == 3
    t = pm.table(L)
    pm.add_item(t, L, 0, "NA", [0, 4, 4, 0, 1], [1 << 4, 1 << 4 | 1])
    assert t[4][4] == 1 and t[5][6:] == [1, 1] and sum(map(sum, t)) == 3


def _both(counts, T, plen, period, a):
    counts = np.asarray(counts, np.int32)
    m = pm.consensus_of(counts, T, plen, period, a)
    x = AlleleConsensus(a, 0, counts, T, plen, period)
    assert (x.consensus, [int(v) for v in x.depth], x.interruptions, x.insertions) == (m["consensus"], m["depth"], m["interruptions"],
                                                                                    m["insertions"])
    return m


def test_consensus_rules_on_crafted_tables():
    T, plen, period, a = "GT" + "CAG" * 3 + "AC", 2, 3, 3          # columns 2..10 are the tract
    c = np.zeros((len(T) + 1, 8), np.int32)
    m = _both(c, T, plen, period, a)
    assert m["consensus"] == T.lower() and not any(m["depth"]) and m["interruptions"] == [] and m["insertions"] == []
    c[0, 2] = 3                   # the template's letter
    c[1, 0] = 2                   # a mismatch outside the tract: consensus only
    c[2, 1], c[2, 3] = 2, 2       # tie with the template's channel among the tied -> C
    c[3, 2], c[3, 3] = 2, 2       # tie without it (ref A) -> the lowest channel, G; half the depth: not reported
    c[4, 0] = 1                   # depth 1: never reported
    c[5, 0], c[5, 1] = 3, 2       # unit 2 offset 0: C -> A with 3 of 5
    c[6, 5], c[6, 0] = 4, 1       # a deletion can be the consensus: A -> -
    c[7, 4], c[7, 2] = 5, 4       # N
    c[8, 0], c[8, 3], c[8, 1] = 2, 2, 1   # a tie among other letters than the template's C -> the lowest, A; 2 of 5
    c[10, 0], c[10, 2] = 3, 3     # the tract's last column, tie with the template's G
    c[11, 3] = 9                  # beyond the tract: A -> T, consensus only
    c[11, 6], c[11, 7] = 2, 5
    c[len(T), 6], c[len(T), 7] = 1, 4
    m = _both(c, T, plen, period, a)
    assert m["consensus"] == "GACGAA-NAaGTc"
    assert m["depth"] == [3, 2, 4, 4, 1, 5, 5, 9, 5, 0, 6, 9, 0]
    assert m["interruptions"] == [
        {"unit": 2, "offset": 0, "ref": "C", "alt": "A", "support": 3, "depth": 5},
        {"unit": 2, "offset": 1, "ref": "A", "alt": "-", "support": 4, "depth": 5},
        {"unit": 2, "offset": 2, "ref": "G", "alt": "N", "support": 5, "depth": 9}]
    assert m["insertions"] == [{"before": 11, "reads": 2, "bases": 5}, {"before": len(T), "reads": 1, "bases": 4}]
    # exactly half is not more than half; one more is
    c[:] = 0
    c[5, 0], c[5, 1] = 2, 2
    assert _both(c, T, plen, period, a)["interruptions"] == [] and _both(c, T, plen, period, a)["consensus"][5] == "C"
    c[5, 0] = 3
    assert _both(c, T, plen, period, a)["interruptions"] == [{"unit": 2, "offset": 0, "ref": "C", "alt": "A", "support": 3, "depth": 5}]
    # depth 2 with both reads on the other letter is the smallest reported case; the first and last tract columns count
    c[:] = 0
    c[2, 3], c[10, 0], c[1, 0], c[11, 0] = 2, 2, 2, 2
    assert [(i["unit"], i["offset"]) for i in _both(c, T, plen, period, a)["interruptions"]] == [(1, 0), (3, 2)]


def test_consensus_rules_on_random_tables():
    rng = np.random.default_rng(3)
    T = "ACGTN" * 2 + "CAG" * 6 + "TTGCA"
    for _ in range(40):
        c = rng.integers(0, 4, (len(T) + 1, 8)).astype(np.int32) * (rng.random((len(T) + 1, 8)) < .5)
        _both(c, T, 10, 3, 6)


def test_statuses_of_the_model():
    lad = [("ACGTAC", "CAG", "TTG", 4), ("ACGTACGT", "A", "", 0)]
    ok = dict(ladders=lad, n_groups=2, cap=4, read_len=5, lad=0, tpl=2, fields=[5, 1, 5, 0, 4], ops=[5 << 4], n_ops=1, group=1)
    assert pm.status_of(**ok) == pm.OK
    for change in (dict(group=2), dict(group=-1), dict(lad=2), dict(tpl=8), dict(tpl=-1), dict(lad=1, tpl=1),
                   dict(fields=[5, 1, 15, 0, 4]), dict(fields=[5, 1, 5, 0, 5]), dict(fields=[5, -1, 3, 0, 4]),
                   dict(n_ops=0), dict(n_ops=5), dict(ops=[5 << 4 | 3]), dict(ops=[5 << 4, 0], n_ops=2),
                   dict(ops=[4 << 4]), dict(ops=[5 << 4, 1 << 4 | 1], n_ops=2), dict(ops=[5 << 4, 1 << 4 | 2], n_ops=2)):
        assert pm.status_of(**dict(ok, **change)) == pm.BAD_ITEM, change
    assert pm.status_of(**dict(ok, read_len=2049)) == pm.TOO_LONG
    long_lad = [("A" * 4000, "CAG", "T" * 90, 4)]
    assert pm.status_of(**dict(ok, ladders=long_lad, tpl=0)) == pm.OK
    assert pm.status_of(**dict(ok, ladders=long_lad, tpl=2)) == pm.TOO_LONG
