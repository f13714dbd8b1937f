"""GPU: the pileup kernel (include/tredpileup.h, tredparse_amd/csrc/pileup.hip through Context.pileup) equals
tests/pileup_model.py exactly -- tables and statuses -- on the three CIGAR fixtures as they are, on crafted shapes (tile
edges, slot L, one-letter reads, counts beyond 16 bits, more groups than workgroups) and on every refusal."""
import numpy as np
import pytest

from tredparse_amd import _lib

from . import cigar_model as cm
from . import cigar_rowpar_model as rm
from . import pileup_model as pm

pytestmark = pytest.mark.gpu
M, I, D = 0, 1, 2


def op(n, code):
    return n << 4 | code


def item(read, lad, tpl, ref_begin, ops, group, read_begin=0, score=0, **over):
    """An item whose fields follow from where it begins and what its operations consume; over: fields / n_ops replaced."""
    on_ref = sum(v >> 4 for v in ops if v & 15 != I)
    on_read = sum(v >> 4 for v in ops if v & 15 != D)
    d = dict(read=read, lad=lad, tpl=tpl, group=group, ops=list(ops), n_ops=len(ops),
             fields=[score, ref_begin, ref_begin + on_ref - 1, read_begin, read_begin + on_read - 1])
    d.update(over)
    return d


def longest(ladders):
    return max(min(pm.template_len(l, 2 * l[3] - 2) if l[3] > 0 else len(l[0]), pm.MAX_TEMPLATE) for l in ladders)


def run(ctx, ladders, items, n_groups, stride=None, cap=None):
    """(counts, status) of the kernel for the items, the outputs pre-filled so that every cell must be written."""
    n = len(items)
    stride = longest(ladders) + 1 if stride is None else stride
    cap = max(max(len(x["ops"]) for x in items), 1) if cap is None else cap
    packed, woff, rlen = _lib.pack_reads([x["read"] for x in items])
    ops = np.zeros((n, cap), np.uint32)
    for k, x in enumerate(items):
        ops[k, :min(len(x["ops"]), cap)] = x["ops"][:cap]
    arr = lambda key, dt: np.ascontiguousarray([x[key] for x in items], dt)
    counts, status = np.full((n_groups, stride, 8), 7, np.int32), np.full(n, -1, np.int32)
    ctx.pileup(packed, woff, rlen, n, arr("lad", np.int32), arr("tpl", np.int32), arr("fields", np.int16), ops, cap,
               arr("n_ops", np.int32), arr("group", np.int32), n_groups, stride, counts, status, ladders=ladders)
    return counts, status


def model(ladders, items, n_groups, stride=None, cap=None):
    stride = longest(ladders) + 1 if stride is None else stride
    cap = max(max(len(x["ops"]) for x in items), 1) if cap is None else cap
    col = lambda key: [x[key] for x in items]
    return pm.pileup(ladders, col("read"), col("lad"), col("tpl"), col("fields"), [x["ops"][:cap] for x in items], col("n_ops"),
                     col("group"), n_groups, stride, cap)


def check(ctx, ladders, items, n_groups, stride=None, cap=None, all_ok=True):
    counts, status = run(ctx, ladders, items, n_groups, stride, cap)
    want, want_status = model(ladders, items, n_groups, stride, cap)
    assert list(status) == list(want_status)
    assert not all_ok or not status.any()
    bad = np.argwhere(counts != want)
    assert len(bad) == 0, (bad[:5].tolist(), counts[tuple(bad[0])], want[tuple(bad[0])])
    return counts, status


# ---- the fixtures, fed as they are ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sw_cigar", "sw_cigar_scorings", "sw_cigar_long"])
def test_fixture_items_one_group_per_ladder_and_units(ctx, which):
    g = {"sw_cigar": cm.golden, "sw_cigar_scorings": cm.golden_scorings, "sw_cigar_long": rm.golden_long}[which]()
    keys = sorted({(int(l), int(t) // 2) for l, t in zip(g["ladder"], g["template"])})
    group = {k: i for i, k in enumerate(keys)}
    items = [dict(read=g["reads"][k], lad=int(g["ladder"][k]), tpl=int(g["template"][k]), fields=[int(v) for v in g["fields"][k][:5]],
                  ops=g["ops"][k], n_ops=len(g["ops"][k]), group=group[(int(g["ladder"][k]), int(g["template"][k]) // 2)])
             for k in range(len(g["reads"]))]
    counts, status = check(ctx, g["ladders"], items, len(keys), all_ok=False)
    assert (status == 0).sum() >= .9 * len(items) and counts[:, :, 6].any() and counts[:, :, 5].any()
    if which == "sw_cigar_long":
        assert counts[:, 512:].any()              # more than one tile


# ---- crafted shapes ---------------------------------------------------------------------------------------------------
def _ladder(rng, T, units=2, period=3):
    """A ladder whose template of `units` units has T columns (random flanks: the pileup never reads them)."""
    suffix = 10
    letters = lambda n: "".join(rng.choice(list("ACGT"), n))
    return (letters(T - suffix - period * units), "CAG"[:period], letters(suffix), units + 1)


def _random_items(rng, T, lad, units, group, n, max_read=300, n_rate=.05):
    """n consistent items on the two templates of `units` units (T columns): random begin, random M / I / D runs."""
    out = []
    for _ in range(n):
        ops, on_ref, on_read = [], 0, 0
        room = int(rng.integers(1, min(T, max_read) + 1))
        rb = int(rng.integers(0, T - room + 1))
        while on_ref < room and on_read < max_read - 8:
            code = int(rng.choice([M, M, I, D])) if ops else M
            if ops and ops[-1] & 15 == code:
                code = M if code != M else D
            ln = int(rng.integers(1, 9)) if code != M else int(rng.integers(1, 80))
            if code != I:
                ln = min(ln, room - on_ref)
            if code != D:
                ln = min(ln, max_read - 8 - on_read)
            if ln == 0:
                break
            ops.append(op(ln, code))
            on_ref += ln if code != I else 0
            on_read += ln if code != D else 0
        qb, tail = int(rng.integers(0, 5)), int(rng.integers(0, 4))
        read = "".join(rng.choice(list("ACGTN"), qb + on_read + tail, p=[(1 - n_rate) / 4] * 4 + [n_rate]))
        out.append(item(read, lad, 2 * (units - 1) + int(rng.integers(0, 2)), rb, ops, group, read_begin=qb))
    return out


@pytest.mark.parametrize("T", [511, 512, 513, 4095])
def test_template_lengths_around_the_tile(ctx, T):
    rng = np.random.default_rng(T)
    lad = [_ladder(rng, T)]
    assert pm.template_len(lad[0], 2) == T
    items = _random_items(rng, T, 0, 2, 0, 60, max_read=2048 if T > 600 else 300)
    # both ends on both strands, and the slot behind the last column from both
    for tpl in (2, 3):
        items.append(item("ACGTNACGT", 0, tpl, 0, [op(2, I), op(7, M)], 0))                  # an insertion first, at column 0
        items.append(item("ACGTNACGT", 0, tpl, T - 6, [op(6, M), op(3, I)], 0))              # an insertion last, behind column T - 1
        items.append(item("G" * min(T, 2048), 0, tpl, 0, [op(min(T, 2048), M)], 0))
        items.append(item("T" * min(T, 2048), 0, tpl, T - min(T, 2048), [op(min(T, 2048), M)], 0))
    counts, _ = check(ctx, lad, items, 1)
    assert counts[0, T, 6] == 2 and counts[0, 0, 6] == 2 and counts[0, 0, :6].sum() > 0 and counts[0, T - 1, :6].sum() > 0
    assert not counts[0, T, :6].any()


def test_a_one_letter_read(ctx):
    rng = np.random.default_rng(1)
    lad = [_ladder(rng, 60)]
    items = [item("A", 0, 2, 17, [op(1, M)], 0), item("A", 0, 3, 17, [op(1, M)], 0), item("N", 0, 2, 59, [op(1, M)], 0)]
    counts, _ = check(ctx, lad, items, 1)
    assert counts[0, 17, 0] == 1 and counts[0, 60 - 1 - 17, 3] == 1 and counts[0, 59, 4] == 1 and counts.sum() == 3


def test_runs_across_a_tile_edge(ctx):
    rng = np.random.default_rng(2)
    T = 1100
    lad = [_ladder(rng, T)]
    read = "".join(rng.choice(list("ACGTN"), 400))
    items = []
    for tpl in (2, 3):
        items.append(item(read, 0, tpl, 300, [op(400, M)], 0))                               # M over 512 (and over T - 512 - 1)
        items.append(item(read, 0, tpl, 480, [op(20, M), op(30, D), op(7, I), op(40, M)], 0))  # D over 512 on the forward strand
        items.append(item(read, 0, tpl, T - 540, [op(20, M), op(30, D), op(40, M)], 0))      # ... and on the reverse strand
        items.append(item(read, 0, tpl, 1000, [op(20, M), op(10, D), op(4, I), op(30, M)], 0))  # D over 1024
        items.append(item(read, 0, tpl, 512, [op(3, I), op(10, M)], 0))                      # a slot on a tile's first column
        items.append(item(read, 0, tpl, 502, [op(10, M), op(3, I)], 0))
    counts, _ = check(ctx, lad, items, 1)
    assert counts[0, 505:520, 5].all() and counts[0, 512, 6] >= 2


def test_an_empty_group_between_two_filled_ones_and_shuffled_order(ctx):
    rng = np.random.default_rng(3)
    lad = [_ladder(rng, 300, units=2), _ladder(rng, 700, units=4)]
    items = _random_items(rng, 300, 0, 2, 0, 40) + _random_items(rng, 700, 1, 4, 2, 40) + _random_items(rng, 300 + 3, 0, 3, 3, 20)
    counts, _ = check(ctx, lad, items, 4)
    assert not counts[1].any() and counts[0].any() and counts[2].any() and counts[3].any()
    order = rng.permutation(len(items))
    again, _ = check(ctx, lad, [items[k] for k in order], 4)
    assert np.array_equal(again, counts)                      # the table does not depend on the order of the items


def test_counts_beyond_16_bits(ctx):
    rng = np.random.default_rng(4)
    lad = [_ladder(rng, 60)]
    one = item("ACGTNACGTACGTTGCAACG", 0, 2, 11, [op(6, M), op(2, I), op(3, D), op(12, M)], 0)
    want, _ = model(lad, [one], 1)
    n = 70000
    counts, status = run(ctx, lad, [one] * n, 1)
    assert not status.any() and np.array_equal(counts, want * n) and counts[0, :, :7].max() == n > 65535


def test_more_groups_than_workgroups(ctx):
    rng = np.random.default_rng(5)
    lad = [_ladder(rng, 60)]
    n = 4200                                                   # the launch has 4 096 workgroups at the most
    items = [x for g in range(n) for x in _random_items(rng, 60, 0, 2, g, 1, max_read=40)]
    counts, _ = check(ctx, lad, items, n)
    assert all(counts[g].any() for g in (0, 4095, 4096, n - 1))
    assert len({counts[g].tobytes() for g in range(n)}) > n // 2


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _base(rng):
    lad = [_ladder(rng, 120, units=3), _ladder(rng, 90, units=2), ("ACGTACGTAC" * 5, "A", "", 0)]
    good = (_random_items(rng, 120, 0, 3, 0, 6, max_read=100) + _random_items(rng, 90, 1, 2, 1, 6, max_read=80) +
            [item("ACGTAC", 2, 0, 4, [op(6, M)], 2)])
    return lad, good


GOOD = dict(read="ACGTACGTACGT", lad=0, tpl=4, ref_begin=20, ops=[op(5, M), op(2, I), op(3, D), op(5, M)], group=0)
CAUSES = {
    "ladder below range": dict(lad=-1),
    "ladder beyond range": dict(lad=3),
    "ladder far beyond range": dict(lad=2 ** 31 - 1),
    "template below range": dict(tpl=-(2 ** 31)),
    "template beyond range": dict(tpl=8),
    "template of a plain reference": dict(lad=2, tpl=1, group=2),
    "group below range": dict(group=-1),
    "group beyond range": dict(group=3),
    "group far beyond range": dict(group=2 ** 31 - 1),
    "ref_begin negative": dict(fields=[0, -1, 11, 0, 11]),
    "ref_end before ref_begin": dict(fields=[0, 20, 19, 0, 11]),
    "ref_end beyond the template": dict(fields=[0, 108, 120, 0, 11]),
    "read_begin negative": dict(fields=[0, 20, 32, -1, 10]),
    "read_end before read_begin": dict(fields=[0, 20, 32, 5, 4]),
    "read_end beyond the read": dict(fields=[0, 20, 32, 1, 12]),
    "no operations": dict(n_ops=0),
    "negative operation count": dict(n_ops=-3),
    "more operations than cap": dict(n_ops=9),
    "an operation code other than M I D": dict(ops=[op(5, M), op(2, 3), op(3, D), op(5, M)]),
    "an operation of length 0": dict(ops=[op(5, M), op(0, I), op(3, D), op(5, M)]),
    "M + D lengths off": dict(ops=[op(5, M), op(2, I), op(4, D), op(5, M)], fields=[0, 20, 32, 0, 11]),
    "M + I lengths off": dict(ops=[op(5, M), op(3, I), op(3, D), op(5, M)], fields=[0, 20, 32, 0, 11]),
    "other units than the group's": dict(tpl=2),
    "another ladder than the group's": dict(lad=1, tpl=2),
}


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_bad_item(ctx, cause):
    rng = np.random.default_rng(6)
    lad, good = _base(rng)
    over = dict(CAUSES[cause])
    spec = dict(GOOD)
    for k in ("lad", "tpl", "group", "ops"):
        if k in over:
            spec[k] = over.pop(k)
    bad = item(**spec, **over)
    at = 4
    items = good[:at] + [bad] + good[at:]
    counts, status = check(ctx, lad, items, 3, cap=8, all_ok=False)
    assert status[at] == _lib.PILEUP_BAD_ITEM and not np.delete(status, at).any(), cause
    without, _ = model(lad, good, 3, cap=8)
    assert np.array_equal(counts, without)
    # the same item unspoilt is accepted and counts
    ok = item(**GOOD)
    counts, status = check(ctx, lad, good[:at] + [ok] + good[at:], 3, cap=8)
    assert not np.array_equal(counts, without)


def test_too_long_read_and_template(ctx):
    rng = np.random.default_rng(7)
    T = 4095
    lad = [_ladder(rng, T, units=2), ("ACGTACGTAC" * 5, "A", "", 0)]               # the ladder's third template has 4 098 columns
    good = _random_items(rng, T, 0, 2, 0, 10, max_read=2048)
    long_read = item("A" * 2049, 0, 2, 7, [op(100, M)], 0, read_begin=3)
    long_template = item("ACGTACGT", 0, 4, 7, [op(8, M)], 1)
    edge = item("C" * 2048, 0, 3, 0, [op(2048, M)], 0)                              # both limits themselves are served
    items = good[:5] + [long_read, long_template, edge] + good[5:]
    counts, status = check(ctx, lad, items, 2, stride=4096, all_ok=False)
    assert list(status[5:8]) == [_lib.PILEUP_TOO_LONG, _lib.PILEUP_TOO_LONG, _lib.PILEUP_OK] and not counts[1].any()
    assert np.array_equal(counts, model(lad, good + [edge], 2, stride=4096)[0])


def test_stride_too_small_is_refused_and_nothing_is_written(ctx):
    rng = np.random.default_rng(8)
    lad, good = _base(rng)
    assert longest(lad) == 123               # the first ladder's fourth template
    with pytest.raises(_lib.TredGpuError, match=r"tredpileup_pileup failed \(-2\).*stride"):
        run(ctx, lad, good, 3, stride=123)
    n = len(good)
    packed, woff, rlen = _lib.pack_reads([x["read"] for x in good])
    ops = np.zeros((n, 8), np.uint32)
    counts, status = np.full((3, 123, 8), 7, np.int32), np.full(n, -1, np.int32)
    z = np.zeros(n, np.int32)
    with pytest.raises(_lib.TredGpuError):
        ctx.pileup(packed, woff, rlen, n, z, z, np.zeros((n, 5), np.int16), ops, 8, z, z, 3, 123, counts, status, ladders=lad)
    assert (counts == 7).all() and (status == -1).all()
    check(ctx, lad, good, 3, stride=124)                       # the smallest stride that holds slot L
    check(ctx, lad, good, 3, stride=700)                       # a second, partly used tile


def test_timing_counts_one_call_per_call(ctx):
    rng = np.random.default_rng(9)
    lad, good = _base(rng)
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_PILEUP) == (0, 0.0)
    run(ctx, lad, good, 3)
    assert ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
    run(ctx, lad, good, 3)
    n, ms = ctx.get_timing(_lib.KERNEL_PILEUP)
    assert n == 2 and ms > 0
    assert ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0 and ctx.get_timing(_lib.KERNEL_SW)[0] == 0
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 0
