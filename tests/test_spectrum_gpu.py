"""GPU: the spectrum kernel (tredpileup_unit_spectrum, tredparse_amd/csrc/pileup.hip through Context.unit_spectrum) equals
tests/spectrum_model.py exactly -- out_spectrum written whole, out_item and the statuses -- on the three CIGAR fixtures as
they are, on the crafted items of tests/test_spectrum_model.py, on periods 1-6, at the limits of read and template, on
counts beyond 16 bits with every lane on one bin and with every lane on its own, on empty, shuffled and many groups, and on every refusal."""
import numpy as np
import pytest

from tredparse_amd import _lib

from . import cigar_model as cm
from . import cigar_rowpar_model as rm
from . import pileup_model as pm
from . import spectrum_model as sm
from .test_pileup_gpu import D, I, M, item, op
from .test_spectrum_model import P_, S_

pytestmark = pytest.mark.gpu
BINS = sm.BINS


def run(ctx, ladders, items, n_groups, group_ladder, cap=None):
    """(spectrum, per item, status) of the kernel, the outputs pre-filled so that every cell must be written."""
    n = len(items)
    cap = max([len(x["ops"]) for x in items] + [1]) if cap is None else cap
    packed, woff, rlen = _lib.pack_reads([x["read"] for x in items])
    ops = np.zeros((n, cap), np.uint32)
    for k, x in enumerate(items):
        ops[k, :min(len(x["ops"]), cap)] = x["ops"][:cap]
    arr = lambda key, dt: np.ascontiguousarray([x[key] for x in items], dt)
    spec, per_item, status = np.full((n_groups, sm.STRIDE), 7, np.int32), np.full((n, 3), 7, np.int32), np.full(n, -1, np.int32)
    ctx.unit_spectrum(packed, woff, rlen, n, arr("lad", np.int32), arr("tpl", np.int32), arr("fields", np.int16), ops,
                      cap, arr("n_ops", np.int32), arr("group", np.int32), n_groups, np.ascontiguousarray(group_ladder, np.int32),
                      spec, per_item, status, ladders=ladders)
    return spec, per_item, status


def model(ladders, items, n_groups, group_ladder, cap=None):
    cap = max([len(x["ops"]) for x in items] + [1]) if cap is None else cap
    col = lambda key: [x[key] for x in items]
    return sm.spectrum(ladders, col("read"), col("lad"), col("tpl"), col("fields"), [x["ops"][:cap] for x in items], col("n_ops"),
                       col("group"), n_groups, list(group_ladder), cap)


def check(ctx, ladders, items, n_groups, group_ladder, cap=None, all_ok=True):
    spec, per_item, status = run(ctx, ladders, items, n_groups, group_ladder, cap)
    want, want_item, want_status = model(ladders, items, n_groups, group_ladder, cap)
    assert list(status) == list(want_status)
    assert not all_ok or not status.any()
    bad = np.argwhere(spec != want)
    assert len(bad) == 0, (bad[:5].tolist(), spec[tuple(bad[0])], want[tuple(bad[0])])
    bad = np.argwhere(per_item != want_item)
    assert len(bad) == 0, (bad[:5].tolist(), per_item[bad[0][0]], want_item[bad[0][0]])
    return spec, per_item, status


def own_template(ladder, tpl):
    prefix, repeat, suffix, _ = ladder
    fwd = prefix + repeat * (tpl // 2 + 1) + suffix
    return pm.revcomp(fwd) if tpl % 2 else fwd


def tract_items(rng, ladders, lad, group, n, max_read=150, noise=.04, max_ops=32):
    """n consistent items that read like the ladder's templates: random units and strand, a random span, M / I / D runs,
    the template's letters under M with a few changed (N among them) -- most words are the motif, some are not."""
    out = []
    mu = ladders[lad][3]
    for _ in range(n):
        tpl = 2 * int(rng.integers(0, mu)) + int(rng.integers(0, 2))
        t = own_template(ladders[lad], tpl)
        T = len(t)
        room = int(rng.integers(1, min(T, max_read) + 1))
        rb = int(rng.integers(0, T - room + 1))
        ops, letters, on_ref, on_read = [], [], 0, 0
        while on_ref < room and on_read < max_read - 8 and len(ops) < max_ops:
            code = int(rng.choice([M, M, M, I, D])) if ops else M
            if ops and ops[-1] & 15 == code:
                code = M if code != M else D
            ln = int(rng.integers(1, 5)) if code != M else int(rng.integers(1, 60))
            if code != I:
                ln = min(ln, room - on_ref)
            if code != D:
                ln = min(ln, max_read - 8 - on_read)
            if ln == 0:
                break
            ops.append(op(ln, code))
            if code == M:
                letters += list(t[rb + on_ref:rb + on_ref + ln])
            elif code == I:
                letters += list(rng.choice(list("ACGT"), ln))
            on_ref += ln if code != I else 0
            on_read += ln if code != D else 0
        for k in np.nonzero(rng.random(len(letters)) < noise)[0]:
            letters[k] = str(rng.choice(list("ACGTN")))
        qb, tail = int(rng.integers(0, 5)), int(rng.integers(0, 4))
        read = "".join(rng.choice(list("ACGT"), qb)) + "".join(letters) + "".join(rng.choice(list("ACGT"), tail))
        out.append(item(read, lad, tpl, rb, ops, group, read_begin=qb))
    return out


# ---- the fixtures, fed as they are ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sw_cigar", "sw_cigar_scorings", "sw_cigar_long"])
def test_fixture_items_one_group_per_ladder(ctx, which):
    g = {"sw_cigar": cm.golden, "sw_cigar_scorings": cm.golden_scorings, "sw_cigar_long": rm.golden_long}[which]()
    ladders = g["ladders"]
    items = [dict(read=g["reads"][k], lad=int(g["ladder"][k]), tpl=int(g["template"][k]), fields=[int(v) for v in g["fields"][k][:5]],
                  ops=g["ops"][k], n_ops=len(g["ops"][k]), group=int(g["ladder"][k])) for k in range(len(g["reads"]))]
    spec, per_item, status = check(ctx, ladders, items, len(ladders), range(len(ladders)), all_ok=False)
    ok = status == 0
    assert ok.sum() >= .4 * len(items) and spec[:, :BINS].sum() > ok.sum() and spec[:, BINS + 3].sum() == ok.sum()
    assert (per_item[~ok] == 0).all() and (per_item[ok, 0] > per_item[ok, 1]).any()


# ---- crafted items ----------------------------------------------------------------------------------------------------
CRAFTED = [(P_, "CAG", S_, 4)]


def test_the_crafted_items_of_the_model_tests(ctx):
    items = [
        item("CAGCAACCGCAG", 0, 6, 4, [op(6, M)], 0), item("CAGCAACCGCAG", 0, 6, 4, [op(5, M)], 0),
        item("CAGCAACCGCAG", 0, 6, 4, [op(7, M)], 0), item("CAGCAACCGCAG", 0, 6, 4, [op(12, M)], 0),
        item("CAGTTCAACCG", 0, 6, 4, [op(3, M), op(2, I), op(6, M)], 1), item("CAGCTTAACCG", 0, 6, 4, [op(4, M), op(2, I), op(5, M)], 1),
        item("CAGCGCCG", 0, 6, 4, [op(4, M), op(1, D), op(4, M)], 2), item("CAGCCG", 0, 6, 4, [op(3, M), op(3, D), op(3, M)], 2),
        item("AGCAACC", 0, 6, 5, [op(7, M)], 3), item("ACG", 0, 6, 0, [op(3, M)], 3), item("TGCAA", 0, 6, 17, [op(5, M)], 3),
        item("GTC", 0, 6, 2, [op(3, M)], 3), item("xxCAGCAG", 0, 6, 4, [op(6, M)], 3, read_begin=2),
        item("CAGCNGcag", 0, 6, 4, [op(9, M)], 4),
        item("CTGCGGTTG", 0, 5, 6, [op(9, M)], 5), item("CTGCGGTTG", 0, 5, 4, [op(9, M)], 5), item("CAACTG", 0, 5, 3, [op(6, M)], 5),
        item("CTGAACTGCTG", 0, 5, 6, [op(3, M), op(2, I), op(6, M)], 5), item("CTGCNG", 0, 5, 6, [op(6, M)], 5),
    ]
    spec, per_item, _ = check(ctx, CRAFTED, items, 7, [0] * 7)
    code = lambda w: sm.code_of(w)
    assert per_item.tolist()[:4] == [[2, 1, 2], [1, 1, 2], [2, 1, 3], [4, 2, 4]]
    assert spec[0, code("CAG")] == 5 and spec[0, code("CAA")] == 3 and spec[0, code("CCG")] == 1 and list(spec[0, BINS:]) == [9, 0, 11, 4]
    assert per_item.tolist()[4:8] == [[3, 1, 3], [2, 1, 3], [2, 1, 3], [2, 1, 3]]
    assert per_item.tolist()[8:13] == [[1, 0, 3], [0, 0, 0], [0, 0, 0], [0, 0, 1], [2, 2, 2]] and spec[3, BINS + 3] == 5
    assert per_item.tolist()[13] == [2, 2, 3] and list(spec[4, BINS:]) == [3, 1, 3, 1]
    assert per_item.tolist()[14:] == [[3, 1, 3], [2, 0, 3], [1, 1, 1], [3, 3, 3], [1, 1, 2]]
    assert spec[5, code("AAC")] == 1 and spec[5, code("CGC")] == 1 and spec[5, BINS + 1] == 1
    assert not spec[6].any()


@pytest.mark.parametrize("period", [1, 2, 3, 4, 5, 6])
def test_periods_one_to_six(ctx, period):
    rng = np.random.default_rng(period)
    repeat = "CAGTTA"[:period]
    lad = [("ACGTTGCATG", repeat, "TTGCAA", 40), ("GGAT", "T" * period, "CCGATAGG", 9)]
    items = tract_items(rng, lad, 0, 0, 120) + tract_items(rng, lad, 1, 1, 60, max_read=60)
    # a run of the motif longer than a wavefront has lanes (period 1 and 2), on both strands
    for tpl in (78, 79):
        items.append(item(own_template(lad[0], tpl)[3:], 0, tpl, 3, [op(len(own_template(lad[0], tpl)) - 3, M)], 0))
    spec, per_item, _ = check(ctx, lad, items, 2, [0, 1])
    assert spec[0, sm.code_of(repeat)] > spec[0, :BINS].sum() // 2 and np.count_nonzero(spec[0, :BINS]) > 1
    assert not spec[:, 4 ** period:BINS].any() and spec[:, BINS + 1].sum() > 0
    assert per_item[-1].tolist() == [40, 40, 40] and (per_item[:, 0] > per_item[:, 1]).any()


def test_a_2048_bp_item_on_a_4095_column_template(ctx):
    rng = np.random.default_rng(11)
    letters = lambda n: "".join(rng.choice(list("ACGT"), n))
    lad = [(letters(1000), "CAG", letters(95), 1000)]
    assert pm.template_len(lad[0], 1998) == 4095
    items = []
    for tpl in (1998, 1999):
        t = own_template(lad[0], tpl)
        for rb in (0, 900, 4095 - 2048):
            items.append(item(t[rb:rb + 2048], 0, tpl, rb, [op(2048, M)], 0))
        read = t[700:1500] + "TT" + t[1500:1900] + t[1907:2753]
        items.append(item(read, 0, tpl, 700, [op(800, M), op(2, I), op(400, M), op(7, D), op(846, M)], 0))
        assert len(read) == 2048
    items += tract_items(rng, lad, 0, 0, 30, max_read=2048)
    spec, per_item, _ = check(ctx, lad, items, 1, [0])
    assert per_item[1].tolist() == [(2948 - 1000) // 3, (2948 - 1000) // 3, (2948 - 1000 + 2) // 3]      # columns 900..2947
    assert spec[0, BINS + 3] == len(items)


def test_counts_beyond_16_bits_with_every_lane_on_the_motif(ctx):
    lad = [("ACGTTGCATG", "CAG", "TTGCAA", 80)]
    t = own_template(lad[0], 2 * 69)
    one = item(t[10:10 + 210], 0, 2 * 69, 10, [op(210, M)], 0)                # 70 units: more than a wavefront's lanes
    want, want_item, _ = model(lad, [one], 1, [0])
    assert want[0, sm.code_of("CAG")] == 70 and want_item[0].tolist() == [70, 70, 70]
    n = 70000
    spec, per_item, status = run(ctx, lad, [one] * n, 1, [0])
    assert not status.any() and np.array_equal(spec, want * n) and (per_item == want_item[0]).all()
    assert spec[0, BINS + 3] == n > 65535 and spec[0, sm.code_of("CAG")] == 70 * n


def test_a_group_whose_words_are_all_different(ctx):
    rng = np.random.default_rng(12)
    lad = [("ACGTTGCATG", "CAGTTA", "TTGCAA", 200)]
    codes = rng.permutation(4096)[:200]
    codes = codes[codes != sm.code_of("CAGTTA")][:150]
    words = ["".join("ACGT"[(c >> (2 * (5 - i))) & 3] for i in range(6)) for c in codes]
    read = "".join(words)
    items = [item(read, 0, 2 * 149, 10, [op(900, M)], 0), item(pm.revcomp(read), 0, 2 * 149 + 1, 6, [op(900, M)], 0)]
    spec, per_item, _ = check(ctx, lad, items, 1, [0])
    assert per_item.tolist() == [[150, 0, 150]] * 2 and (spec[0, codes] == 2).all() and spec[0, :BINS].sum() == 300


def test_empty_groups_no_items_and_shuffled_order(ctx):
    rng = np.random.default_rng(13)
    lad = [("ACGTTGCATG", "CAG", "TTGCAA", 50), ("GGAT", "CCTG", "CCGATAGG", 30)]
    items = tract_items(rng, lad, 0, 0, 80) + tract_items(rng, lad, 1, 2, 80) + tract_items(rng, lad, 0, 3, 5)
    spec, per_item, _ = check(ctx, lad, items, 5, [0, 1, 1, 0, 1])
    assert not spec[1].any() and not spec[4].any() and spec[0].any() and spec[2].any() and spec[3].any()
    order = rng.permutation(len(items))
    again, again_item, _ = check(ctx, lad, [items[k] for k in order], 5, [0, 1, 1, 0, 1])
    assert np.array_equal(again, spec) and np.array_equal(again_item, per_item[order])
    # no items at all: the rows are written, zero
    spec, per_item, status = run(ctx, lad, [], 3, [0, 1, 0])
    assert spec.shape == (3, sm.STRIDE) and not spec.any() and len(status) == 0
    # items and no group: every item's group is out of range
    spec, per_item, status = run(ctx, lad, items[:3], 0, [])
    assert list(status) == [_lib.PILEUP_BAD_ITEM] * 3 and not per_item.any()


def test_more_groups_than_workgroups(ctx):
    rng = np.random.default_rng(14)
    lad = [("ACGTTGCATG", "CAG", "TTGCAA", 20)]
    n = 4200                                                   # the launch has 4 096 workgroups at the most
    items = tract_items(rng, lad, 0, 0, n, max_read=60, noise=.1)
    for g, x in enumerate(items):
        x["group"] = g
    spec, _, _ = check(ctx, lad, items, n, [0] * n)
    assert all(spec[g, BINS + 3] == 1 for g in (0, 4095, 4096, n - 1))
    assert len({spec[g].tobytes() for g in range(n)}) > n // 4


# ---- refusals ---------------------------------------------------------------------------------------------------------
LADDERS = [("ACGTTGCATGACGTTGCATG", "CAG", "TTGCAATTGC", 30), ("GGATGGAT", "CCTG", "CCGATAGG", 20), ("ACGTACGTAC" * 5, "A", "", 0),
           ("ACGTTGCATG", "CAGCAGCAGCAA", "TTGCAA", 6)]
GROUP_LADDER = [0, 1, 2, 3]


def _good(rng):
    return tract_items(rng, LADDERS, 0, 0, 6, max_read=100, max_ops=8) + tract_items(rng, LADDERS, 1, 1, 6, max_read=80, max_ops=8)


GOOD = dict(read="CAGCAGTTCAACAG", lad=0, tpl=8, ref_begin=20, ops=[op(6, M), op(2, I), op(3, D), op(6, M)], group=0)
CAUSES = {
    "ladder below range": (dict(lad=-1), 5),
    "ladder beyond range": (dict(lad=4), 5),
    "template below range": (dict(tpl=-(2 ** 31)), 5),
    "template beyond range": (dict(tpl=60), 5),
    "group below range": (dict(group=-1), 5),
    "group beyond range": (dict(group=4), 5),
    "group far beyond range": (dict(group=2 ** 31 - 1), 5),
    "ref_begin negative": (dict(fields=[0, -1, 13, 0, 13]), 5),
    "ref_end before ref_begin": (dict(fields=[0, 20, 19, 0, 13]), 5),
    "ref_end beyond the template": (dict(fields=[0, 31, 45, 0, 13]), 5),
    "read_begin negative": (dict(fields=[0, 20, 34, -1, 12]), 5),
    "read_end before read_begin": (dict(fields=[0, 20, 34, 5, 4]), 5),
    "read_end beyond the read": (dict(fields=[0, 20, 34, 1, 14]), 5),
    "no operations": (dict(n_ops=0), 5),
    "more operations than cap": (dict(n_ops=9), 5),
    "an operation code other than M I D": (dict(ops=[op(6, M), op(2, 3), op(3, D), op(6, M)]), 5),
    "an operation of length 0": (dict(ops=[op(6, M), op(0, I), op(3, D), op(6, M)]), 5),
    "M + D lengths off": (dict(ops=[op(6, M), op(2, I), op(4, D), op(6, M)], fields=[0, 20, 34, 0, 13]), 5),
    "M + I lengths off": (dict(ops=[op(6, M), op(3, I), op(3, D), op(6, M)], fields=[0, 20, 34, 0, 13]), 5),
    "another ladder than the group's": (dict(lad=1), 5),
    "a ladder without a tract": (dict(lad=2, tpl=0, group=2), 5),
    "a period of 12": (dict(lad=3, group=3), 6),
    "a period of 12 in another ladder's group": (dict(lad=3, group=0), 5),
    "a read of 2 049 letters": (dict(read="CAGCAGTTCAACAG" + "A" * 2035), 4),
}


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_refused_item(ctx, cause):
    rng = np.random.default_rng(6)
    good = _good(rng)
    over, want_status = CAUSES[cause]
    over, spec_of = dict(over), dict(GOOD)
    for k in ("read", "lad", "tpl", "group", "ops"):
        if k in over:
            spec_of[k] = over.pop(k)
    bad = item(**spec_of, **over)
    at = 4
    items = good[:at] + [bad] + good[at:]
    spec, per_item, status = check(ctx, LADDERS, items, 4, GROUP_LADDER, cap=8, all_ok=False)
    assert status[at] == want_status and not np.delete(status, at).any(), cause
    assert want_status in (_lib.PILEUP_TOO_LONG, _lib.PILEUP_BAD_ITEM, _lib.PILEUP_PERIOD)
    without, without_item, _ = model(LADDERS, good, 4, GROUP_LADDER, cap=8)
    assert np.array_equal(spec, without) and not per_item[at].any() and np.array_equal(np.delete(per_item, at, axis=0), without_item)
    # the same item unspoilt is accepted and counts
    spec, _, _ = check(ctx, LADDERS, good[:at] + [item(**GOOD)] + good[at:], 4, GROUP_LADDER, cap=8)
    assert not np.array_equal(spec, without)


def test_too_long_template(ctx):
    rng = np.random.default_rng(7)
    letters = lambda n: "".join(rng.choice(list("ACGT"), n))
    lad = [(letters(4000), "CAG", letters(89), 3)]             # templates of 4 092, 4 095 and 4 098 columns
    ok = item("CAGCAG", 0, 2, 4000, [op(6, M)], 0)
    items = [ok, item("CAGCAG", 0, 4, 4000, [op(6, M)], 0), dict(ok, tpl=3, fields=[0, 89, 94, 0, 5])]
    spec, per_item, status = check(ctx, lad, items, 1, [0], all_ok=False)
    assert list(status) == [0, _lib.PILEUP_TOO_LONG, 0] and per_item.tolist() == [[2, 2, 2], [0, 0, 0], [2, 0, 2]]


def _raw_args(items, ladders, n_groups, group_ladder, cap=8):
    n = len(items)
    packed, woff, rlen = _lib.pack_reads([x["read"] for x in items])
    ops = np.zeros((n, cap), np.uint32)
    for k, x in enumerate(items):
        ops[k, :len(x["ops"])] = x["ops"]
    arr = lambda key, dt: np.ascontiguousarray([x[key] for x in items], dt)
    return dict(packed=packed, read_off=woff, read_len=rlen, n_items=n, item_ladder=arr("lad", np.int32),
                item_template=arr("tpl", np.int32), fields=arr("fields", np.int16), ops=ops, cap=cap, n_ops=arr("n_ops", np.int32),
                item_group=arr("group", np.int32), n_groups=n_groups, group_ladder=np.ascontiguousarray(group_ladder, np.int32),
                out_spectrum=np.full((max(n_groups, 1), sm.STRIDE), 7, np.int32), out_item=np.full((n, 3), 7, np.int32),
                out_status=np.full(n, -1, np.int32), ladders=ladders)


BAD_CALLS = [(k, None) for k in ("packed", "read_off", "read_len", "item_ladder", "item_template", "fields", "ops", "n_ops",
                                   "item_group", "group_ladder", "out_spectrum", "out_item", "out_status")] + \
            [("group_ladder", np.array([0, 4, 2, 3], np.int32)), ("group_ladder", np.array([0, 1, -1, 3], np.int32)),
             ("n_groups", -1), ("cap", 0), ("n_items", -1)]


@pytest.mark.parametrize("key,value", BAD_CALLS, ids=["{}={}".format(k, "NULL" if v is None else "bad") + str(i)
                                                        for i, (k, v) in enumerate(BAD_CALLS)])
def test_a_refused_call_writes_nothing(ctx, key, value):
    rng = np.random.default_rng(8)
    a = _raw_args(_good(rng), LADDERS, 4, GROUP_LADDER)
    outs = {k: a[k] for k in ("out_spectrum", "out_item", "out_status")}
    a[key] = value
    with pytest.raises(_lib.TredGpuError, match=r"tredpileup_unit_spectrum failed \(-2\)"):
        ctx.unit_spectrum(**a)
    assert (outs["out_spectrum"] == 7).all() and (outs["out_item"] == 7).all() and (outs["out_status"] == -1).all()


def test_timing_counts_one_call_per_call(ctx):
    rng = np.random.default_rng(9)
    good = _good(rng)
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_PILEUP) == (0, 0.0)
    run(ctx, LADDERS, good, 4, GROUP_LADDER)
    assert ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
    run(ctx, LADDERS, good, 4, GROUP_LADDER)
    n, ms = ctx.get_timing(_lib.KERNEL_PILEUP)
    assert n == 2 and ms > 0
    assert ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0 and ctx.get_timing(_lib.KERNEL_SW)[0] == 0
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 0
