"""GPU: the anchored pileup (tredpileup_pileup_anchored, tredparse_amd/csrc/pileup.hip through Context.pileup_anchored)
equals tests/pileup_anchored_model.py exactly -- tables, written whole, and statuses: the four strand x anchor
combinations with operations across the cut, the cut and the shift on a tile's edge, several groups of one ladder, every
refusal of an item and of a call, and whole items against the existing entry."""
import numpy as np
import pytest

from tredparse_amd import _lib, synth

from . import pileup_anchored_model as am
from . import pileup_model as pm
from .test_pileup_gpu import _random_items, item, op
from .test_pileup_gpu import run as run_plain

pytestmark = pytest.mark.gpu
M, I, D = 0, 1, 2
PREFIX, SUFFIX = "GAGTCCCTCAAGTCCTTC", "CAACAGCCGCCACCGCCG"
HD = (PREFIX, "CAG", SUFFIX, 50)
P, p, S = 18, 3, 18


def T_of(ladder, units):
    return len(ladder[0]) + len(ladder[1]) * units + len(ladder[2])


def anchored(x, anchor):
    return dict(x, anchor=anchor)


def run(ctx, ladders, items, groups, stride=None, cap=None, fill=7):
    """(counts, status) of the kernel; groups: [(ladder, units)].  The outputs are pre-filled: every cell must be written."""
    n = len(items)
    stride = max(T_of(ladders[l], a) for l, a in groups) + 1 if stride is None else stride
    cap = max([len(x["ops"]) for x in items] + [1]) if cap is None else cap
    packed, woff, rlen = _lib.pack_reads([x["read"] for x in items]) if n else (np.zeros(1, np.uint32), np.zeros(1, np.int64),
                                                                                np.zeros(0, np.int32))
    ops = np.zeros((n, cap), np.uint32)
    for k, x in enumerate(items):
        ops[k, :min(len(x["ops"]), cap)] = x["ops"][:cap]
    arr = lambda key, dt: np.ascontiguousarray([x[key] for x in items], dt)
    counts, status = np.full((len(groups), stride, 8), fill, np.int32), np.full(n, -1, np.int32)
    ctx.pileup_anchored(packed, woff, rlen, n, arr("lad", np.int32), arr("tpl", np.int32),
                        arr("fields", np.int16).reshape(n, 5), ops, cap, arr("n_ops", np.int32), arr("group", np.int32),
                        arr("anchor", np.int32), len(groups), np.ascontiguousarray([g[0] for g in groups], np.int32),
                        np.ascontiguousarray([g[1] for g in groups], np.int32), stride, counts, status, ladders=ladders)
    return counts, status


def model(ladders, items, groups, stride=None, cap=None):
    stride = max(T_of(ladders[l], a) for l, a in groups) + 1 if stride is None else stride
    cap = max([len(x["ops"]) for x in items] + [1]) if cap is None else cap
    col = lambda key: [x[key] for x in items]
    return am.pileup_anchored(ladders, col("read"), col("lad"), col("tpl"), col("fields"), [x["ops"][:cap] for x in items],
                              col("n_ops"), col("group"), col("anchor"), len(groups), [g[0] for g in groups],
                              [g[1] for g in groups], stride, cap)


def check(ctx, ladders, items, groups, stride=None, cap=None, all_ok=True):
    counts, status = run(ctx, ladders, items, groups, stride, cap)
    want, want_status = model(ladders, items, groups, stride, cap)
    assert list(status) == list(want_status)
    assert not all_ok or not status.any()
    bad = np.argwhere(counts != want)
    assert len(bad) == 0, (bad[:5].tolist(), counts[tuple(bad[0])], want[tuple(bad[0])])
    return counts, status


def at_forward(ladder, h, strand, lo, ops, group, anchor, lad=0):
    """An item whose operations begin at FORWARD column lo of its own template of h units when read left to right on the
    forward strand: on the reverse-complement template the same columns, the operations in reverse order."""
    on_ref = sum(v >> 4 for v in ops if v & 15 != I)
    on_read = sum(v >> 4 for v in ops if v & 15 != D)
    read = ("ACGTTGCANACGGTCA" * 130)[:on_read + 3]
    if strand:
        return anchored(item(read, lad, 2 * h - 1, T_of(ladder, h) - lo - on_ref, list(reversed(ops)), group, read_begin=2), anchor)
    return anchored(item(read, lad, 2 * h - 2, lo, list(ops), group, read_begin=2), anchor)


# ---- (a) strand x anchor --------------------------------------------------------------------------------------------------
def test_the_four_strand_and_anchor_combinations(ctx):
    rng = np.random.default_rng(31)
    a, items = 12, []
    for h in (1, 5, 11, 12):
        Th, cut = T_of(HD, h), P + p * h
        for strand in (0, 1):
            for anchor in (am.BEGIN, am.END) + ((am.WHOLE,) if h == a else ()):
                items.append(at_forward(HD, h, strand, 0, [op(Th, M)], 0, anchor))                         # M across both cuts
                items.append(at_forward(HD, h, strand, 3, [op(10, M), op(Th - 20, D), op(5, M)], 0, anchor))  # D across both
                for slot in (P - 1, P, P + 1, cut - 1, cut, cut + 1):                                      # I at and next to the cuts
                    items.append(at_forward(HD, h, strand, slot - 4, [op(4, M), op(2, I), op(3, M)], 0, anchor))
                items.append(at_forward(HD, h, strand, 0, [op(1, I), op(6, M)], 0, anchor))                # slot 0
                items.append(at_forward(HD, h, strand, Th - 6, [op(6, M), op(3, I)], 0, anchor))           # slot T_h
                for x in _random_items(rng, Th, 0, h, 0, 4, max_read=120):
                    items.append(anchored(x, anchor))
    counts, _ = check(ctx, [HD], items, [(0, a)])
    Ta = T_of(HD, a)
    assert counts[0, :Ta, :6].sum(axis=1).all() and counts[0, 0, 6] and counts[0, Ta, 6] and not counts[0, Ta, :6].any()
    # one item per combination, h = 5: the side it lands on
    left, right = (0, P + p * 5), (P + 21, T_of(HD, 5) + 21)
    for strand, anchor, (lo, hi) in ((0, am.BEGIN, left), (1, am.BEGIN, right), (0, am.END, right), (1, am.END, left)):
        one, _ = check(ctx, [HD], [at_forward(HD, 5, strand, 0, [op(T_of(HD, 5), M)], 0, anchor)], [(0, a)])
        assert np.nonzero(one[0, :, :6].sum(axis=1))[0].tolist() == list(range(lo, hi)), (strand, anchor)


# ---- (b) tile edges -------------------------------------------------------------------------------------------------------
def test_right_items_on_the_edge_of_the_second_tile(ctx):
    a, h = 170, 40
    assert T_of(HD, a) == 546
    shift, Th = (a - h) * p, T_of(HD, h)
    own = lambda col: col - shift                            # the own forward column that lands on a group's column
    assert shift == 390 and P < own(480) and own(545) == Th - 1
    items = []
    for strand in (0, 1):
        for anchor in ((am.END, am.BEGIN)[strand],):         # RIGHT on either strand
            items.append(at_forward(HD, h, strand, own(490), [op(22, M)], 0, anchor))                      # ends at 511
            items.append(at_forward(HD, h, strand, own(512), [op(20, M)], 0, anchor))                      # starts at 512
            items.append(at_forward(HD, h, strand, own(500), [op(8, M), op(8, D), op(9, M)], 0, anchor))   # D over 511 / 512
            items.append(at_forward(HD, h, strand, own(505), [op(20, M)], 0, anchor))                      # M over 511 / 512
            items.append(at_forward(HD, h, strand, own(508), [op(4, M), op(3, I), op(6, M)], 0, anchor))   # a slot at 512
            items.append(at_forward(HD, h, strand, own(507), [op(4, M), op(2, I), op(6, M)], 0, anchor))   # ... and at 511
            items.append(at_forward(HD, h, strand, 2, [op(Th - 2, M)], 0, anchor))                         # cut at P, both tiles
            items.append(at_forward(HD, h, strand, Th - 5, [op(5, M), op(1, I)], 0, anchor))               # slot 546
    counts, _ = check(ctx, [HD], items, [(0, a)])
    assert counts.shape == (1, 547, 8) and (counts[0, 512, 6], counts[0, 511, 6], counts[0, 546, 6]) == (2, 2, 2)
    assert counts[0, 511, :6].sum() == 12 and counts[0, 512, :6].sum() == 12 and counts[0, 508:516, 5].tolist() == [2] * 8
    assert not counts[0, :P + shift].any() and counts[0, P + shift, :6].sum() == 2


def _ladder_cut_at(target):
    """(ladder, h) with P + p * h == target: a locus of the table if one fits, else a crafted ladder."""
    for l in synth.load_loci():
        Pl, pl = len(l["prefix"]), len(l["repeat"])
        if (target - Pl) % pl == 0 and (target - Pl) // pl >= 1:
            h = (target - Pl) // pl
            return (l["prefix"], l["repeat"], l["suffix"], h + 4), h, l["name"]
    rng = np.random.default_rng(target)
    Pl = target - 4 * 120
    return ("".join(rng.choice(list("ACGT"), Pl)), "ACGT", "TTGACCA", 124), 120, None


@pytest.mark.parametrize("target", [511, 512, 513])
def test_a_left_cut_on_the_tile_edge(ctx, target):
    lad, h, name = _ladder_cut_at(target)
    assert len(lad[0]) + len(lad[1]) * h == target and (name is not None) == (target == 513)   # the table has one for 513 only
    a = h + 3
    Th, items = T_of(lad, h), []
    for strand in (0, 1):
        anchor = (am.BEGIN, am.END)[strand]                  # LEFT on either strand
        items.append(at_forward(lad, h, strand, target - 30, [op(min(40, Th - target + 30), M)], 0, anchor))   # M across the cut
        items.append(at_forward(lad, h, strand, target - 9, [op(5, M), op(7, D), op(2, M)], 0, anchor))        # D across it
        for slot in (target - 1, target, target + 1):
            items.append(at_forward(lad, h, strand, slot - 4, [op(4, M), op(2, I), op(2, M)], 0, anchor))
        items.append(at_forward(lad, h, strand, 0, [op(Th, M)], 0, anchor))
        items.append(at_forward(lad, a, strand, 0, [op(T_of(lad, a), M)], 0, anchor))                        # h == a: whole
    counts, _ = check(ctx, [lad], items, [(0, a)])
    depth = counts[0, :, :6].sum(axis=1)
    assert depth[target - 1] == 2 * 7 and depth[target] == 2 and counts[0, target - 1, 6] == 2 and counts[0, target, 6] == 0


def test_groups_of_one_ladder_an_empty_group_and_no_items(ctx):
    rng = np.random.default_rng(33)
    groups = [(0, 170), (0, 30), (0, 7), (0, 170)]
    items = []
    for g, (_, a) in enumerate(groups[:2]):
        for h in (3, 7, 30):
            for x in _random_items(rng, T_of(HD, h), 0, h, g, 12, max_read=140):
                items.append(anchored(x, int(rng.integers(1, 3))))
    counts, _ = check(ctx, [HD], items, groups)
    assert counts[0].any() and counts[1].any() and not counts[2].any() and not counts[3].any()
    assert counts[0, 512:].any() and not counts[1, T_of(HD, 30) + 1:].any()
    order = rng.permutation(len(items))
    again, _ = check(ctx, [HD], [items[k] for k in order], groups)
    assert np.array_equal(again, counts)
    none, status = run(ctx, [HD], [], groups)
    assert none.shape == (4, 547, 8) and not none.any() and len(status) == 0


# ---- (c) refusals ---------------------------------------------------------------------------------------------------------
LADDERS = [HD, (PREFIX, "CAG", SUFFIX + "A", 50), ("ACGTACGTAC" * 4, "A", "", 0)]
GROUPS = [(0, 12), (1, 12), (2, 1)]
GOOD = dict(read="ACGTACGTACGT", lad=0, tpl=8, ref_begin=20, ops=[op(5, M), op(2, I), op(3, D), op(5, M)], group=0)
CAUSES = {
    "another ladder than the group's": dict(lad=1),
    "a group of another ladder": dict(group=1),
    "a plain reference": dict(lad=2, tpl=0, group=2),
    "anchor below range": dict(anchor=-1),
    "anchor beyond range": dict(anchor=3),
    "more units than the group": dict(tpl=24),
    "whole with other units than the group's": dict(anchor=am.WHOLE),
    "ladder beyond range": dict(lad=3),
    "template beyond range": dict(tpl=100),
    "group beyond range": dict(group=3),
    "group below range": dict(group=-1),
    "ref_end beyond the template": dict(fields=[0, 40, 51, 0, 11]),
    "no operations": dict(n_ops=0),
    "more operations than cap": dict(n_ops=9),
    "an operation code other than M I D": dict(ops=[op(5, M), op(2, 3), op(3, D), op(5, M)]),
    "M + D lengths off": dict(ops=[op(5, M), op(2, I), op(4, D), op(5, M)], fields=[0, 20, 32, 0, 11]),
}


def _good(rng):
    out = []
    for h, anchor in ((5, am.BEGIN), (9, am.END), (12, am.WHOLE)):
        out += [anchored(x, anchor) for x in _random_items(rng, T_of(HD, h), 0, h, 0, 3, max_read=60)]
    out += [anchored(x, am.END) for x in _random_items(rng, T_of(LADDERS[1], 4), 1, 4, 1, 3, max_read=60)]
    return out


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_bad_item(ctx, cause):
    rng = np.random.default_rng(34)
    good = _good(rng)
    over = dict(CAUSES[cause])
    spec, anchor = dict(GOOD), over.pop("anchor", am.BEGIN)
    for k in ("lad", "tpl", "group", "ops"):
        if k in over:
            spec[k] = over.pop(k)
    bad = anchored(item(**spec, **over), anchor)
    at = 4
    counts, status = check(ctx, LADDERS, good[:at] + [bad] + good[at:], GROUPS, cap=8, all_ok=False)
    assert status[at] == _lib.PILEUP_BAD_ITEM and not np.delete(status, at).any(), cause
    without, _ = model(LADDERS, good, GROUPS, cap=8)
    assert np.array_equal(counts, without)
    ok = anchored(item(**GOOD), am.BEGIN)                       # the same item unspoilt is accepted and counts
    counts, status = check(ctx, LADDERS, good[:at] + [ok] + good[at:], GROUPS, cap=8)
    assert not np.array_equal(counts, without)


def test_too_long_read_and_template(ctx):
    rng = np.random.default_rng(35)
    lad = [("".join(rng.choice(list("ACGT"), 4079)), "CAG", "TTGACCATGG", 3)]       # 4 092, 4 095 and 4 098 columns
    groups = [(0, 2), (0, 4)]
    good = [anchored(x, am.BEGIN) for x in _random_items(rng, 4092, 0, 1, 0, 6, max_read=2048)]
    long_read = anchored(item("A" * 2049, 0, 0, 7, [op(100, M)], 0, read_begin=3), am.BEGIN)
    long_template = anchored(item("ACGTACGT", 0, 4, 7, [op(8, M)], 1), am.BEGIN)
    edge = anchored(item("C" * 2048, 0, 3, 0, [op(2048, M)], 0), am.END)             # both limits themselves are served
    beyond = anchored(item("ACGTACGT", 0, 2, 4085, [op(8, M)], 1), am.END)           # the GROUP's template may be longer
    items = good[:3] + [long_read, long_template, edge, beyond] + good[3:]
    counts, status = check(ctx, lad, items, groups, all_ok=False)
    assert list(status[3:7]) == [_lib.PILEUP_TOO_LONG, _lib.PILEUP_TOO_LONG, _lib.PILEUP_OK, _lib.PILEUP_OK]
    assert counts.shape[1] == 4102 and counts[1, 4085 + 6:4085 + 6 + 8, :6].sum() == 8


def test_refused_calls_write_nothing(ctx):
    rng = np.random.default_rng(36)
    good = _good(rng)
    n = len(good)
    packed, woff, rlen = _lib.pack_reads([x["read"] for x in good])
    arr = lambda key, dt: np.ascontiguousarray([x[key] for x in good], dt)
    ops = np.zeros((n, 8), np.uint32)
    for k, x in enumerate(good):
        ops[k, :len(x["ops"])] = x["ops"]
    base = dict(item_anchor=arr("anchor", np.int32), group_ladder=np.array([0, 1, 2], np.int32),
                group_units=np.array([12, 12, 1], np.int32), stride=T_of(LADDERS[1], 12) + 1)
    cases = {
        "units below 1": dict(group_units=np.array([12, 0, 1], np.int32)),
        "negative units": dict(group_units=np.array([-4, 12, 1], np.int32)),
        "group ladder below range": dict(group_ladder=np.array([0, -1, 2], np.int32)),
        "group ladder beyond range": dict(group_ladder=np.array([0, 1, 3], np.int32)),
        "stride below the largest group template + 1": dict(stride=T_of(LADDERS[1], 12)),
        "stride of a longer group": dict(group_units=np.array([12, 13, 1], np.int32)),
        "stride beyond the cap": dict(stride=65537),
        "no anchors": dict(item_anchor=None),
        "no group ladders": dict(group_ladder=None),
        "no group units": dict(group_units=None),
    }
    for cause, over in sorted(cases.items()):
        kw = dict(base, **over)
        counts, status = np.full((3, kw["stride"], 8), 7, np.int32), np.full(n, -1, np.int32)
        with pytest.raises(_lib.TredGpuError, match=r"tredpileup_pileup_anchored failed \(-2\)"):
            ctx.pileup_anchored(packed, woff, rlen, n, arr("lad", np.int32), arr("tpl", np.int32), arr("fields", np.int16), ops, 8,
                                arr("n_ops", np.int32), arr("group", np.int32), kw["item_anchor"], 3, kw["group_ladder"],
                                kw["group_units"], kw["stride"], counts, status, ladders=LADDERS)
        assert (counts == 7).all() and (status == -1).all(), cause
    check(ctx, LADDERS, good, GROUPS, stride=base["stride"])               # the smallest stride that holds the last slot
    # the ladders' own templates (168 columns and more) do not bound the stride
    check(ctx, LADDERS, [x for x in good if x["group"] == 0], [(0, 12)], stride=T_of(HD, 12) + 1)


# ---- (d) the existing entry -----------------------------------------------------------------------------------------------
def test_whole_items_equal_the_existing_entry_and_timing_counts_both(ctx):
    rng = np.random.default_rng(37)
    lad = [HD, (PREFIX[:11], "CCG", SUFFIX[:7], 180)]
    groups = [(0, 12), (1, 170), (0, 3)]
    items = []
    for g, (l, a) in enumerate(groups):
        items += [anchored(x, am.WHOLE) for x in _random_items(rng, T_of(lad[l], a), l, a, g, 25, max_read=300)]
    ctx.reset_timing()
    counts, status = check(ctx, lad, items, groups, stride=700)
    assert ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
    plain, plain_status = run_plain(ctx, lad, items, len(groups), stride=700)
    n, ms = ctx.get_timing(_lib.KERNEL_PILEUP)
    assert n == 2 and ms > 0
    assert np.array_equal(counts, plain) and np.array_equal(status, plain_status) and counts[1, 512:].any()
    assert pm.OK == _lib.PILEUP_OK and (am.WHOLE, am.BEGIN, am.END) == (_lib.PILEUP_ANCHOR_WHOLE, _lib.PILEUP_ANCHOR_BEGIN,
                                                                        _lib.PILEUP_ANCHOR_END)
