"""CPU: tests/pileup_anchored_model.py -- the yardstick of tredpileup_pileup_anchored -- against tests/pileup_model.py on
whole items, against the text of the reference's own report (tests/golden/alignments_t001_HD.txt) on the partial reads of
t001 / HD, and rule by rule on hand-made items; AlleleConsensus' three new counts and the parser's new flag."""
import os

import numpy as np

from tredparse_amd import tred as tredmod
from tredparse_amd.consensus import AlleleConsensus

from . import pileup_anchored_model as am
from . import pileup_model as pm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PREFIX, SUFFIX = "GAGTCCCTCAAGTCCTTC", "CAACAGCCGCCACCGCCG"
P, p, S = 18, 3, 18
M, I, D = 0, 1, 2


def op(n, code):
    return n << 4 | code


# ---- whole items: the existing model ----------------------------------------------------------------------------------
def _random_call(rng):
    ladders = [("ACGTTGCA" * 2, "CAG", "TTGACC", 6), ("GATTACA", "AT", "CCGGA", 9), ("ACGTACGTAC" * 3, "A", "", 0)]
    groups = [(0, 3), (1, 5), (0, 6), (1, 1)]
    items = dict(reads=[], lad=[], tpl=[], fields=[], ops=[], n_ops=[], group=[])
    for _ in range(40):
        g = int(rng.integers(0, len(groups)))
        lad, a = groups[g]
        T = pm.template_len(ladders[lad], 2 * a - 2)
        rb = int(rng.integers(0, T - 1))
        room, ops, on_ref, on_read = int(rng.integers(1, T - rb + 1)), [], 0, 0
        while on_ref < room:
            code = M if not ops or ops[-1] & 15 != M else int(rng.choice([I, D]))
            n = int(rng.integers(1, 6))
            if code != I:
                n = min(n, room - on_ref)
                on_ref += n
            if code != D:
                on_read += n
            ops.append(op(n, code))
        qb = int(rng.integers(0, 3))
        items["reads"].append("".join(rng.choice(list("ACGTN"), qb + on_read + 2)))
        items["lad"].append(lad)
        items["tpl"].append(2 * a - 2 + int(rng.integers(0, 2)))
        items["fields"].append([0, rb, rb + on_ref - 1, qb, qb + on_read - 1])
        items["ops"].append(ops)
        items["n_ops"].append(len(ops))
        items["group"].append(g)
    # what an item is refused for on its own: both models say so alike
    items["fields"][3][2] += 1
    items["n_ops"][7] = 0
    items["group"][11] = 9
    items["lad"][13] = 5
    return ladders, groups, items


def test_whole_items_equal_the_existing_model():
    rng = np.random.default_rng(20)
    for _ in range(8):
        ladders, groups, x = _random_call(rng)
        stride = 64
        want, want_status = pm.pileup(ladders, x["reads"], x["lad"], x["tpl"], x["fields"], x["ops"], x["n_ops"], x["group"],
                                      len(groups), stride, 12)
        got, status = am.pileup_anchored(ladders, x["reads"], x["lad"], x["tpl"], x["fields"], x["ops"], x["n_ops"], x["group"],
                                         [am.WHOLE] * len(x["reads"]), len(groups), [g[0] for g in groups],
                                         [g[1] for g in groups], stride, 12)
        assert list(status) == list(want_status) and (status != 0).sum() >= 4 and np.array_equal(got, want) and got.any()


# ---- t001 / HD: the report's text against its CIGARs ------------------------------------------------------------------
def t001_partial_table(alleles=(15, 41)):
    """(table of the longest allele from the text of the PREF / POST blocks placed on it, the same from their CIGARs, the
    numbers placed / ambiguous / beyond) -- shared with the GPU tests."""
    with open(os.path.join(GOLD, "alignments_t001_HD.txt")) as fp:
        blocks = pm.parse_blocks(fp.read())
    a = max(alleles)
    T = P + p * a + S
    text, cigar, n = pm.table(T), pm.table(T), {"partial": 0, "ambiguous": 0, "beyond": 0}
    for b in blocks:
        kind, where = am.place(b["tag"], b["h"], alleles)
        if b["tag"] == "FULL" or kind is None:
            continue
        n[kind] += 1
        if kind != "partial":
            continue
        assert where == a
        Th = PREFIX + "CAG" * b["h"] + SUFFIX
        assert (pm.revcomp(b["target"]) if b["strand"] else b["target"]) == Th
        am.from_lines_anchored(text, P, p, S, b["h"], a, b["strand"], b["tag"], b["fields"][1], b["lines"][0], b["lines"][2])
        read = "N" * b["fields"][3] + b["lines"][2].replace(" ", "")
        am.add_item_anchored(cigar, P, p, S, b["h"], a, b["strand"], am.ANCHOR_OF_TAG[b["tag"]], read, b["fields"],
                             pm.cigar_ops(b["cigar_string"]))
    return text, cigar, n


def test_t001_hd_partial_reads_cover_allele_41():
    text, cigar, n = t001_partial_table()
    assert text == cigar
    assert n == {"partial": 7, "ambiguous": 14, "beyond": 0}
    T41 = PREFIX + "CAG" * 41 + SUFFIX
    got = pm.consensus_of(text, T41, P, p, 41)
    assert got["consensus"] == T41 and (min(got["depth"]), max(got["depth"])) == (3, 6)
    assert got["interruptions"] == [] and got["insertions"] == []


# ---- rule by rule -----------------------------------------------------------------------------------------------------
A, H = 12, 5                     # the group's units and the item's: T_a = 72, T_h = 51, the tract of the item ends before 33
TH = P + p * H + S


def _one(strand, anchor, ref_begin, ops, read=None, h=H, a=A):
    """The table (as {column: row}) of one item on a group of a units."""
    on_read = sum(v >> 4 for v in ops if v & 15 != D)
    on_ref = sum(v >> 4 for v in ops if v & 15 != I)
    read = read or ("ACGT" * 40)[:on_read]
    t = pm.table(P + p * a + S)
    am.add_item_anchored(t, P, p, S, h, a, strand, anchor, read, [0, ref_begin, ref_begin + on_ref - 1, 0, on_read - 1], ops)
    return {c: row for c, row in enumerate(t) if any(row)}


def _cols(t):
    return sorted(c for c, row in t.items() if any(row[:6]))


def test_left_is_cut_exactly_at_the_end_of_its_tract():
    t = _one(0, am.BEGIN, 20, [op(25, M)])                         # columns 20..44 of T_h: the tract ends before 33
    assert _cols(t) == list(range(20, 33))
    assert _cols(_one(0, am.BEGIN, 33, [op(5, M)])) == [] and _cols(_one(0, am.BEGIN, 32, [op(5, M)])) == [32]


def test_right_is_cut_exactly_at_the_prefix_and_shifted():
    t = _one(0, am.END, 10, [op(30, M)])                           # columns 10..39 of T_h: kept from P = 18, moved by 21
    assert _cols(t) == [c + (A - H) * p for c in range(18, 40)]
    assert _cols(_one(0, am.END, 10, [op(8, M)])) == [] and _cols(_one(0, am.END, 10, [op(9, M)])) == [18 + 21]
    # the letters go with their columns: the read's base 8 is the first kept
    assert _one(0, am.END, 10, [op(9, M)], read="AAAAAAAAG")[39][:5] == [0, 0, 1, 0, 0]


def test_an_insertion_at_the_cut_is_dropped_and_its_neighbours_are_kept():
    cut = P + p * H
    for slot, kept in ((cut - 1, True), (cut, False), (cut + 1, False)):
        t = _one(0, am.BEGIN, slot - 4, [op(4, M), op(2, I), op(3, M)])
        assert ((t.get(slot) or [0] * 8)[6:] == [1, 2]) == kept, slot
    for slot, kept in ((P - 1, False), (P, False), (P + 1, True)):
        t = _one(0, am.END, slot - 4, [op(4, M), op(2, I), op(3, M)])
        assert ((t.get(slot + 21) or [0] * 8)[6:] == [1, 2]) == kept, slot
        assert sum(row[6] for row in t.values()) == int(kept)


def test_slot_0_on_the_left_and_the_last_slot_on_the_right():
    t = _one(0, am.BEGIN, 0, [op(2, I), op(6, M)])
    assert t[0][6:] == [1, 2] and _cols(t) == list(range(6))
    t = _one(0, am.END, TH - 6, [op(6, M), op(3, I)])
    Ta = P + p * A + S
    assert t[Ta][6:] == [1, 3] and _cols(t) == list(range(Ta - 6, Ta)) and not any(t[Ta][:6])


def test_a_deletion_and_a_match_run_across_the_cut_count_on_the_kept_side():
    cut = P + p * H
    t = _one(0, am.BEGIN, cut - 6, [op(3, M), op(6, D), op(4, M)])
    assert [t[c][5] for c in range(cut - 3, cut)] == [1, 1, 1] and _cols(t) == list(range(cut - 6, cut))
    t = _one(0, am.END, P - 5, [op(2, M), op(6, D), op(4, M)], read="ACGTAC")
    assert _cols(t) == [c + 21 for c in range(P, P + 7)] and [t[c + 21][5] for c in range(P, P + 3)] == [1, 1, 1]
    assert [t[c + 21][:4] for c in range(P + 3, P + 7)] == [[0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0]]


def test_both_strands_times_both_anchors_land_on_the_stated_side():
    whole = [op(TH, M)]
    left, right = list(range(0, P + p * H)), [c + 21 for c in range(P, TH)]
    assert _cols(_one(0, am.BEGIN, 0, whole)) == left          # PREF on the forward template
    assert _cols(_one(1, am.BEGIN, 0, whole)) == right         # PREF on the reverse complement: the suffix end
    assert _cols(_one(0, am.END, 0, whole)) == right           # POST on the forward template
    assert _cols(_one(1, am.END, 0, whole)) == left            # POST on the reverse complement
    # a reverse-complement item's letters are complemented, and its own column c is forward column T_h - 1 - c
    t = _one(1, am.END, TH - 3, [op(3, M)], read="AAC")
    assert (t[0][:4], t[1][:4], t[2][:4]) == ([0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 1])


def test_an_item_of_the_groups_units_counts_whole_whatever_its_anchor():
    ops = [op(20, M), op(2, I), op(3, D), op(30, M)]
    for strand in (0, 1):
        want = pm.table(P + p * A + S)
        pm.add_item(want, len(want) - 1, strand, ("ACGT" * 40)[:52], [0, 7, 59, 0, 51], ops)
        for anchor in (am.WHOLE, am.BEGIN, am.END):
            assert _one(strand, anchor, 7, ops, h=A) == {c: row for c, row in enumerate(want) if any(row)}


def test_the_refusals_of_an_item_against_its_group():
    ladders = [(PREFIX, "CAG", SUFFIX, 20), (PREFIX, "CAG", SUFFIX + "A", 20), ("ACGT" * 20, "A", "", 0)]
    args = dict(n_groups=3, cap=4, read_len=10, fields=[0, 0, 9, 0, 9], ops=[op(10, M)], n_ops=1, group_ladder=[0, 1, 2],
                group_units=[12, 12, 1])
    st = lambda **kw: am.status_of_anchored(ladders, **dict(dict(args, lad=0, tpl=8, group=0, anchor=am.BEGIN), **kw))
    assert st() == pm.OK and st(anchor=am.END) == pm.OK and st(tpl=22, anchor=am.WHOLE) == pm.OK and st(tpl=23) == pm.OK
    assert st(lad=1) == pm.BAD_ITEM and st(group=1) == pm.BAD_ITEM               # another ladder than the group's
    assert st(lad=2, tpl=0, group=2) == pm.BAD_ITEM                              # a plain reference
    assert st(anchor=3) == pm.BAD_ITEM and st(anchor=-1) == pm.BAD_ITEM
    assert st(tpl=24) == pm.BAD_ITEM                                             # h = 13 > a
    assert st(anchor=am.WHOLE) == pm.BAD_ITEM                                    # WHOLE with h != a
    assert st(fields=[0, 0, 10, 0, 9]) == pm.BAD_ITEM and st(read_len=3000) == pm.TOO_LONG


def test_place():
    assert am.place("FULL", 15, [15, 41]) == ("whole", 15) and am.place("FULL", 16, [15, 41]) == (None, None)
    assert am.place("PREF", 16, [15, 41]) == ("partial", 41) and am.place("POST", 41, [41, 15]) == ("partial", 41)
    assert am.place("PREF", 15, [15, 41]) == ("ambiguous", 41) and am.place("POST", 42, [15, 41]) == ("beyond", 41)
    assert am.place("PREF", 1, [41, 41]) == ("partial", 41) and am.place("PREF", 3, [0, -1]) == (None, None)
    assert am.place("REPT", 20, [15, 41]) == (None, None) and am.place("HANG", 20, [15, 41]) == (None, None)


# ---- AlleleConsensus and the parser ------------------------------------------------------------------------------------
def test_allele_consensus_with_and_without_partial():
    text, _, n = t001_partial_table()
    T41 = PREFIX + "CAG" * 41 + SUFFIX
    table = np.asarray(text, np.int32)
    x = AlleleConsensus(41, 0, table, T41, P, p, partial=n["partial"], ambiguous=n["ambiguous"], beyond=n["beyond"])
    want = pm.consensus_of(text, T41, P, p, 41)
    plain = dict(want, h=41, reads=0)
    assert x.to_dict() == plain and list(x.to_dict()) == ["h", "reads", "consensus", "depth", "interruptions", "insertions"]
    assert x.to_dict(partial=True) == dict(plain, partial=7, ambiguous=14, beyond=0)
    y = AlleleConsensus(41, 0, table, T41, P, p)
    assert (y.partial, y.ambiguous, y.beyond) == (0, 0, 0) and y.to_dict() == plain


def test_the_parser_sets_both_options():
    p_ = tredmod.set_argparse()
    base = ["x.bam", "--tred", "HD"]
    a = p_.parse_args(base + ["--consensus-partial"])
    assert a.consensus is True and a.consensus_partial is True
    a = p_.parse_args(base + ["--consensus"])
    assert a.consensus is True and a.consensus_partial is False
    a = p_.parse_args(base)
    assert a.consensus is False and a.consensus_partial is False
    from tredparse_amd.runtime import _options
    arg = ("k", "x.bam", None, ["HD"], 300, False, False, True, True, "INFO")
    assert _options(arg + (False, True, True))["consensus_partial"] is True
    assert _options(arg + (False, True))["consensus_partial"] is False and _options(arg)["consensus_partial"] is False
