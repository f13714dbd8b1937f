"""GPU: the CIGAR kernel (tredparse_amd/csrc/sw_cigar.hip) where one scoring, one tier and one item per lane do not
reach: the reference's goldens at eight more scorings (tests/golden/sw_cigar_scorings.npz), items on either side of the
two limits between the narrow and the wide kernel, lanes that take a second and a third item with the previous item's
cells still in their arrays, and what a context keeps between calls (ladder table, staging buffers, release).

Everything goes through the C ABI (_lib.Context.sw_cigar); expected operations are tests/cigar_model.py's -- pinned to
the compiled reference by the goldens -- and are compared exactly.  The tier an item ends in is PREDICTED: cm.bands_of
gives the bands the model ran, cm.is_wide applies the kernel's own NARROW_ROW / NARROW_PLANE to them, and every group
asserts that it holds the tiers it is named for.

Wide items by that prediction: boundaries 8 of 18 at 1/5/7/2 and 10 of 20 at 2/2/3/1 and 3/5/7/2 (which add the 40-base
pair), the full-cover rectangle, wide statuses 40 of 80, the mixed call 200 of 320 (host and device), the large call
120 of 33 000.  Scorings: the 8 of the fixture, 1/5/7/2, 2/2/2/2 in the large call and 8/16/16/1 for full cover.
"""
import collections
import random

import numpy as np
import pytest

from tredparse_amd import _lib, ssw

from . import cigar_model as cm

pytestmark = pytest.mark.gpu
CAP = 32
DEFAULT = (1, 5, 7, 2)
CHEAP_GAPS = (2, 2, 3, 1)             # a gap of 40 bases costs what 21 matches give: short reads carry a wide band's path
Item = collections.namedtuple("Item", "ladder template read fields")      # ladder: (prefix, repeat, suffix, max_units)
_expected = {}


def _params(scoring):
    return _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], 9, 0, 0, 0)


def _expect(item, scoring):
    """(status, ops, bands, wide) of the model for the item, computed once per (item, scoring)."""
    key = (item, scoring)
    if key not in _expected:
        st, ops, passes = cm.passes_of(cm.template(item.ladder, item.template), item.read, item.fields, *scoring)
        bands = [b for b, _ in passes]
        _expected[key] = (st, ops, bands, cm.is_wide(bands, item.fields[4] - item.fields[3] + 1))
    return _expected[key]


def _want_arrays(want, cap):
    """What the call must write for [(status, ops)]: an OK item longer than cap is an OVERFLOW with its true count."""
    ops, n_ops, status = np.zeros((len(want), cap), np.uint32), np.zeros(len(want), np.int32), np.zeros(len(want), np.int32)
    for i, (st, w) in enumerate(want):
        status[i] = st
        if st == cm.OK:
            n_ops[i] = len(w)
            if len(w) > cap:
                status[i] = cm.OVERFLOW
            else:
                ops[i, :len(w)] = w
    return ops, n_ops, status


class Call(object):
    """The arguments of one sw_cigar call over items[src[k]]: every distinct read is packed once and every distinct
    expectation computed once, however often src names it."""

    def __init__(self, items, src=None):
        self.items = list(items)
        self.src = np.arange(len(self.items)) if src is None else np.asarray(src)
        self.ladders = list(collections.OrderedDict((it.ladder, 0) for it in self.items))
        lid = {l: i for i, l in enumerate(self.ladders)}
        self.packed, woff, rlen = _lib.pack_reads([it.read for it in self.items])
        self.n = len(self.src)
        self.read_off = np.ascontiguousarray(np.append(woff[:-1][self.src], woff[-1]), np.int64)
        self.read_len = np.ascontiguousarray(rlen[self.src], np.int32)
        self.ladder = np.array([lid[it.ladder] for it in self.items], np.int32)[self.src]
        self.template = np.array([it.template for it in self.items], np.int32)[self.src]
        self.fields = np.array([it.fields for it in self.items], np.int16).reshape(-1, 5)[self.src]

    def run(self, ctx, scoring, cap=CAP, device=False, ladders=None, ladder=None, template=None):
        n = self.n
        ladders = self.ladders if ladders is None else ladders
        ladder = self.ladder if ladder is None else ladder
        template = self.template if template is None else template
        args = [self.packed, self.read_off, self.read_len, np.ascontiguousarray(ladder), np.ascontiguousarray(template),
                np.ascontiguousarray(self.fields)]
        if not device:
            ops, n_ops, status = np.full((n, cap), 7, np.uint32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
            ctx.sw_cigar(_lib.MEM_HOST, args[0], args[1], args[2], n, args[3], args[4], args[5], _params(scoring), cap, ops,
                         n_ops, status, ladders=ladders)
            return ops, n_ops, status
        import torch
        args[0] = args[0].view(np.int32)
        d = [torch.from_numpy(a).cuda() for a in args]
        ops = torch.full((n, cap), 7, dtype=torch.int32, device="cuda")
        n_ops = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.sw_cigar(_lib.MEM_DEVICE, d[0], d[1], d[2], n, d[3], d[4], d[5], _params(scoring), cap, ops, n_ops, status,
                     ladders=ladders)
        ctx.sync()
        return ops.cpu().numpy().view(np.uint32), n_ops.cpu().numpy(), status.cpu().numpy()

    def want(self, scoring, cap=CAP):
        ops, n_ops, status = _want_arrays([_expect(it, scoring)[:2] for it in self.items], cap)
        return ops[self.src], n_ops[self.src], status[self.src]

    def wide(self, scoring):
        return np.array([_expect(it, scoring)[3] for it in self.items])[self.src]

    def check(self, ctx, scoring, cap=CAP, device=False):
        got = self.run(ctx, scoring, cap, device)
        _same(got, self.want(scoring, cap), self)
        return got


def _same(got, want, call=None):
    for name, g, w in zip(("status", "n_ops", "ops"), (got[2], got[1], got[0]), (want[2], want[1], want[0])):
        if not np.array_equal(g, w):
            k = int(np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][0])
            it = call.items[call.src[k]] if call is not None else None
            raise AssertionError("{} of item {} ({} differ): got {}, want {}; fields {}, read of {}".format(
                name, k, int((g != w).reshape(len(g), -1).any(axis=1).sum()), g[k].tolist(), w[k].tolist(),
                it and it.fields, it and len(it.read)))


# ---- items ----------------------------------------------------------------------------------------------------------------
def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _rect(rng, ref_len, read_len, score, pad=2):
    """A ref_len x read_len rectangle on a plain reference, cut around a single gap of |ref_len - read_len| bases in the
    middle of an exact copy, `pad` bases of the read and of the reference outside it: the first band, |ref_len -
    read_len| + 1, holds that path, so a modest score is reached there."""
    ref = _seq(rng, pad + ref_len + pad)
    body = ref[pad:pad + ref_len]
    half = min(ref_len, read_len) // 2
    if ref_len >= read_len:
        read = body[:half] + body[half + ref_len - read_len:]
    else:
        read = body[:half] + _seq(rng, read_len - ref_len) + body[half:]
    assert len(read) == read_len
    read = _seq(rng, pad) + read + _seq(rng, pad)
    return Item((ref, "A", "", 0), 0, read, (score, pad, pad + ref_len - 1, pad, pad + read_len - 1))


def _compensating(rng, n, g, scoring):
    """Equal lengths: an insertion of g bases at 70 and a deletion of g bases at 160 of an n-base copy, with the score of
    exactly that path -- no band below g reaches it."""
    ref = _seq(rng, n + 20)
    body = ref[10:10 + n]
    read = body[:70] + _seq(rng, g) + body[70:160] + body[160 + g:]
    assert len(read) == n
    m, _, o, e = scoring
    score = (n - g) * m - 2 * (o + (g - 1) * e)
    return Item((ref, "A", "", 0), 0, read, (score, 10, 10 + n - 1, 0, n - 1))


def _full_cover(rng, score):
    """480 x 511: the read's first 90 bases lie on the diagonal 300 columns to the right, 269 inserted bases bring it back
    to the last cell's diagonal: only the last band (510, the whole rectangle) holds that path."""
    x, a, b = _seq(rng, 300), _seq(rng, 90), _seq(rng, 121)
    return Item((x + a + b, "A", "", 0), 0, a + _seq(rng, 269) + b, (score, 0, 510, 0, 479))


def _wide_base(rng, scoring, n=16):
    """Cheap wide items: reads of 60-90 bp with a deletion of 36-44 bases (band 37-45 from the first pass)."""
    out = []
    for k in range(n):
        L, g = rng.randint(60, 90), rng.randint(36, 44)
        it = _rect(rng, L + g, L, 10 * scoring[0], pad=rng.randint(0, 4))
        if k % 4 == 3:                                              # and two short indels, for more than three operations
            f = it.fields
            read = it.read[:f[3] + 8] + "TT" + it.read[f[3] + 8:f[4] - 9] + it.read[f[4] - 6:]
            it = Item(it.ladder, 0, read, (f[0], f[1], f[2], f[3], f[4] - 1))
        out.append(it)
    return out


VARIANTS = ((0, 0, 0, 0, -2), (0, 0, -3, 0, 0), (0, 0, 0, 3, 0), (0, 1, 0, 0, 0), (0, 3, 0, 0, 0))      # as test_cigar_crafted_gpu


def _moved(items, scoring, far=False):
    """Every item with its fields cut or moved off the path (OFF_EDGE, zero-length M) and, for `far`, with a score out of
    reach (NO_PATH)."""
    out = []
    for it in items:
        for d in VARIANTS:
            f = tuple(int(a + b) for a, b in zip(it.fields, d))
            if f[1] <= f[2] and f[3] <= f[4]:
                out.append(Item(it.ladder, it.template, it.read, (10 * scoring[0],) + f[1:]))
        if far:
            out.append(Item(it.ladder, it.template, it.read, (it.fields[0] + 4000,) + it.fields[1:]))
    return out


def _golden_items(g, ks, score=None):
    return [Item(g["ladders"][g["ladder"][k]], int(g["template"][k]), g["reads"][k],
                 tuple(int(v) for v in g["fields"][k]) if score is None else (score,) + tuple(int(v) for v in g["fields"][k][1:]))
            for k in ks]


# ---- 1. goldens at other scorings -----------------------------------------------------------------------------------------
def _scoring_call(g, s):
    ks = [k for k, v in enumerate(g["scoring"]) if v == s]
    return ks, Call(_golden_items(g, ks))


@pytest.mark.parametrize("scoring", sorted(set(cm.golden_scorings()["scoring"])), ids=lambda s: "/".join(map(str, s)))
def test_kernel_reproduces_the_goldens_of_every_scoring(ctx, scoring):
    g = cm.golden_scorings()
    ks, call = _scoring_call(g, scoring)
    assert len(ks) >= 55 and max(len(g["ops"][k]) for k in ks) <= CAP
    _same(call.run(ctx, scoring), _want_arrays([(cm.OK, g["ops"][k]) for k in ks], CAP), call)


@pytest.mark.parametrize("args", [(), (3, 5, 7, 2)], ids=["default", "3/5/7/2"])
def test_aligner_gives_the_references_text_at_its_default_and_at_another_scoring(ctx, args):
    """Aligner(ref, report_cigar=True) without scoring arguments is 2/2/3/1, as the reference's."""
    g = cm.golden_scorings()
    scoring = args or (2, 2, 3, 1)
    ks = [k for k, v in enumerate(g["scoring"]) if v == scoring]
    by_ref = {}
    for k in ks:
        by_ref.setdefault(g["refs"][k], []).append(k)
    assert len(ks) >= 55
    for ref, sub in by_ref.items():
        al = ssw.Aligner(ref, *args, report_cigar=True, ctx=ctx).align_many([g["reads"][k] for k in sub])
        for k, a in zip(sub, al):
            assert [a.score, a.ref_begin, a.ref_end, a.query_begin, a.query_end] == list(g["fields"][k]), k
            assert a.cigar_string == a.cigar == g["cigar_string"][k], (k, a.cigar_string, g["cigar_string"][k])


# ---- 2. tier boundaries ---------------------------------------------------------------------------------------------------
_boundaries = {}


def _boundary_items(scoring):
    """[(name, item, wide?)] around the two limits of the narrow kernel."""
    if scoring in _boundaries:
        return _boundaries[scoring]
    rng = random.Random("boundaries {}".format(scoring))
    s = 10 * scoring[0]
    out = []
    for L in (252, 40):
        out += [("del 31 / band 32 x {}".format(L), _rect(rng, L + 31, L, s), False),
                ("del 32 / band 33 x {}".format(L), _rect(rng, L + 32, L, s), True)]
    out += [("ins 31 / band 32 x 252", _rect(rng, 221, 252, s), False),
            ("ins 31 / band 32 x 253", _rect(rng, 222, 253, s), True),
            ("ins 32 / band 33 x 252", _rect(rng, 220, 252, s), True),
            ("ins 32 / band 33 x 200", _rect(rng, 168, 200, s), True),
            ("band 17 x 468, del", _rect(rng, 484, 468, s), False), ("band 17 x 469, del", _rect(rng, 485, 469, s), True),
            ("band 17 x 468, ins", _rect(rng, 452, 468, s, pad=1), False),
            ("band 17 x 469, ins", _rect(rng, 453, 469, s, pad=1), True),
            ("band 16 x 480, del", _rect(rng, 495, 480, s, pad=0), False),
            ("band 16 x 480, ins", _rect(rng, 465, 480, s, pad=0), False),
            ("band 1 x 480", _rect(rng, 480, 480, s, pad=0), False),
            ("compensating 20", _compensating(rng, 250, 20, scoring), False),
            ("compensating 20 x 252", _compensating(rng, 252, 20, scoring), False),
            ("compensating 20 x 253", _compensating(rng, 253, 20, scoring), True)]
    if scoring != DEFAULT:                       # at 1/5/7/2 two gaps of 40 bases cost more than 250 matches give
        out += [("compensating 40", _compensating(rng, 250, 40, scoring), True),
                ("compensating 40 x 200", _compensating(rng, 200, 40, scoring), True)]
    _boundaries[scoring] = out
    return out


@pytest.mark.parametrize("scoring", [DEFAULT, (2, 2, 3, 1), (3, 5, 7, 2)], ids=lambda s: "/".join(map(str, s)))
def test_items_on_either_side_of_the_narrow_limits(ctx, scoring):
    cases = _boundary_items(scoring)
    for name, it, wide in cases:                                      # the case did not drift
        st, ops, bands, w = _expect(it, scoring)
        assert w == wide and st == cm.OK, (name, bands, st)
        if name.startswith("compensating 20"):
            assert bands == [1, 2, 4, 8, 16, 32], (name, bands)
        elif name.startswith("compensating 40"):
            assert bands == [1, 2, 4, 8, 16, 32, 64], (name, bands)       # six narrow passes, then wide
        else:
            assert len(bands) == 1 and "band {} ".format(bands[0]) in name, (name, bands)
    assert sum(1 for c in cases if c[2]) >= 8 and sum(1 for c in cases if not c[2]) >= 10
    assert any(len(_expect(it, scoring)[1]) >= 3 for _, it, _ in cases)
    call = Call([it for _, it, _ in cases])
    call.check(ctx, scoring)
    order = np.arange(call.n)[::-1]                                   # and in the opposite order, through device memory
    Call(call.items, order).check(ctx, scoring, device=True)


FULL_COVER = (8, 16, 16, 1)
FULL_COVER_SCORE = 8 * (90 + 121) - (16 + 268)          # 90 M, 269 I, 121 M


def test_the_480_x_511_rectangle_at_full_cover(ctx):
    """Opening a gap is dear and extending it cheap, so that the path with 269 inserted bases is the best of the rectangle
    and chance finds little else: the bands assert that no pass before the last reaches FULL_COVER_SCORE."""
    it = _full_cover(random.Random("full cover"), FULL_COVER_SCORE)
    st, ops, bands, wide = _expect(it, FULL_COVER)
    assert st == cm.OK and bands == [32, 64, 128, 256, 510] and wide
    assert ops == [90 << 4, 269 << 4 | 1, 121 << 4]
    call = Call([it])
    call.check(ctx, FULL_COVER)
    call.check(ctx, FULL_COVER, device=True)


_wide_sets = {}


def _wide_status_items(scoring=CHEAP_GAPS):
    """Wide items of every status, and narrow ones between them."""
    if scoring not in _wide_sets:
        rng = random.Random("wide statuses {}".format(scoring))
        base = _wide_base(rng, scoring, 8)
        wide = base + _moved(base, scoring, far=True)[:32]
        g = cm.golden()
        narrow = _golden_items(g, [k for k, c in enumerate(g["cls"]) if c in "bce" and len(g["reads"][k]) <= 250 and
                                   len(g["ops"][k]) <= 3][:16])
        _wide_sets[scoring] = (wide, narrow)
    return _wide_sets[scoring]


def test_overflow_no_path_and_off_edge_on_wide_items(ctx):
    wide, narrow = _wide_status_items()
    items = [x for pair in zip(wide, (narrow * 3)[:len(wide)]) for x in pair]          # wide, narrow, wide, narrow ...
    call = Call(items)
    w = call.wide(CHEAP_GAPS)
    assert w[0::2].all() and not w[1::2].any() and w.sum() == 40
    sts = [_expect(it, CHEAP_GAPS)[0] for it in wide]
    long_ = [k for k, it in enumerate(wide) if _expect(it, CHEAP_GAPS)[0] == cm.OK and len(_expect(it, CHEAP_GAPS)[1]) >= 5]
    assert sts.count(cm.NO_PATH) >= 4 and sts.count(cm.OFF_EDGE) >= 4 and sts.count(cm.OK) >= 12 and len(long_) >= 2
    call.check(ctx, CHEAP_GAPS)
    # room for four operations: the wide items with five or more overflow, the neighbours stay intact
    got = call.check(ctx, CHEAP_GAPS, cap=4)
    for k in long_:
        assert got[2][2 * k] == _lib.CIGAR_OVERFLOW and got[1][2 * k] == len(_expect(wide[k], CHEAP_GAPS)[1]) and not got[0][2 * k].any()
    assert (got[2][1::2] == _lib.CIGAR_OK).sum() >= 0.9 * len(wide)


_mixed = {}


def _mixed_call():
    """200 wide items -- every one of the 64 wide lanes takes at least three -- among 120 narrow ones, shuffled."""
    if not _mixed:
        wide, narrow = _wide_status_items()
        g = cm.golden()
        narrow = narrow + _golden_items(g, [k for k, c in enumerate(g["cls"]) if len(g["reads"][k]) <= 250][::3][:104])
        items = wide + narrow
        src = np.array(list(range(len(wide))) * 5 + list(range(len(wide), len(items))))
        np.random.RandomState(20261018).shuffle(src)
        _mixed["call"] = Call(items, src)
    return _mixed["call"]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_wide_lane_takes_three_items(ctx, device):
    call = _mixed_call()
    w = call.wide(CHEAP_GAPS)
    assert w.sum() == 200 >= 3 * 64 and (~w).sum() == 120
    assert w[:40].any() and (~w[:40]).any()                               # mixed, not sorted by tier
    call.check(ctx, CHEAP_GAPS, device=device)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_calls_of_one_wavefront_and_one_item_more(ctx, n):
    call = _mixed_call()
    part = Call(call.items, call.src[:n] if n > 1 else call.src[np.nonzero(call.wide(CHEAP_GAPS))[0][:1]])
    w = part.wide(CHEAP_GAPS)
    assert part.n == n and w.any() and (n == 1 or (~w).any())
    part.check(ctx, CHEAP_GAPS)


# ---- 3. lanes that take a second and a third item ---------------------------------------------------------------------------
N_LARGE = 2 * 16384 + 232
_large = {}


def _large_call():
    """About 500 distinct items tiled to N_LARGE in a fixed shuffled order: items k, k + 16 384 and k + 32 768 share a
    lane of the narrow grid (256 blocks of 64 lanes, grid-stride)."""
    if _large:
        return _large["call"]
    rng = random.Random("large")
    g, gs = cm.golden(), cm.golden_scorings()
    short = [k for k in range(len(g["reads"])) if len(g["reads"][k]) <= 250]
    items = _golden_items(g, ([k for k in short if g["cls"][k] in "cdef"] + [k for k in short if g["cls"][k] in "ab"])[:260])
    items += _golden_items(gs, range(0, len(gs["reads"]), 4), score=10)           # every scoring's shapes, any band reaches 10
    for diff in (0, 1, 2, 3, 5, 7, 11, 15, 16, 20, 24, 28, 30, 31):                # crafted: bands 1 to 32
        for sign in (1, -1):
            L = rng.choice([36, 50, 75, 100, 150]) if diff < 30 else rng.choice([36, 250])
            items.append(_rect(rng, L + diff, L, 10) if sign > 0 else _rect(rng, max(L - diff, 20), max(L - diff, 20) + diff, 10))
    for L in (36, 75, 100, 150, 200, 250):                                         # band 32 on reads of 36 to 250 bp
        items.append(_rect(rng, L + 31, L, 10))
    base = _golden_items(g, [k for k, c in enumerate(g["cls"]) if c in "cde" and len(g["reads"][k]) <= 250][:12])
    items += _moved(base, DEFAULT)                                                 # OFF_EDGE and zero-length M
    for k in range(12):                                                            # NO_PATH inside the narrow tier
        n = rng.randint(15, 33)
        it = _rect(rng, n, n - rng.randint(0, 3), 10)
        items.append(Item(it.ladder, 0, it.read, (4000,) + it.fields[1:]))
    n_narrow = len(items)
    wide = _wide_base(rng, DEFAULT, 12)
    wide += _moved(wide, DEFAULT, far=True)[:12]
    items += wide
    reps = -(-(N_LARGE - 5 * len(wide)) // n_narrow)
    src = np.concatenate([np.tile(np.arange(n_narrow), reps)[:N_LARGE - 5 * len(wide)],
                          np.tile(np.arange(n_narrow, len(items)), 5)])
    np.random.RandomState(20261019).shuffle(src)
    _large["call"] = Call(items, src)
    _large["n_narrow"] = n_narrow
    return _large["call"]


@pytest.mark.parametrize("scoring", [DEFAULT, (2, 2, 2, 2)], ids=lambda s: "/".join(map(str, s)))
def test_lanes_take_a_second_and_a_third_item(ctx, scoring):
    call = _large_call()
    assert call.n == N_LARGE >= 2 * 16384 + 100 and len(call.items) >= 450
    exp = [_expect(it, scoring) for it in call.items]
    wide = np.array([e[3] for e in exp])
    assert not wide[:_large["n_narrow"]].any() and wide[_large["n_narrow"]:].all() and call.wide(scoring).sum() == 120
    first = np.array([e[2][0] for e in exp])[call.src]
    last = np.array([e[2][-1] for e in exp])[call.src]
    st = np.array([e[0] for e in exp])[call.src]
    w = wide[call.src]
    a, b = slice(0, N_LARGE - 16384), slice(16384, N_LARGE)                    # an item and the lane's next one
    assert ((last[a] == 32) & (first[b] == 1) & ~w[a] & ~w[b]).sum() >= 10       # a 32-band item, then a 1-band one
    assert ((st[a] == cm.OFF_EDGE) & (st[b] == cm.OK) & ~w[b]).sum() >= 10
    assert ((st[a] == cm.NO_PATH) & (st[b] == cm.OK) & ~w[a] & ~w[b]).sum() >= 10
    assert (np.array([len(e[2]) for e in exp])[call.src] >= 3).sum() >= 500      # bands that doubled twice or more
    assert len({len(it.read) for it in call.items}) >= 20
    call.check(ctx, scoring)


# ---- 4. what a context keeps between calls ----------------------------------------------------------------------------------
def _table_items(rng, refs, scoring):
    """One read per reference: a copy with a 3-base deletion, placed by its own path's score."""
    out = []
    for ref in refs:
        a, n = rng.randint(0, 10), rng.randint(100, 150)
        p = rng.randint(30, n - 30)
        read = ref[a:a + p] + ref[a + p + 3:a + n]
        out.append(Item((ref, "A", "", 0), 0, read, ((n - 3) * scoring[0] - scoring[2] - 2 * scoring[3], a, a + n - 1, 0, n - 4)))
    return out


def test_ladder_table_follows_the_call(ctx):
    """Tables A, B, A -- B has A's count and A's lengths, other letters -- and then a table of another count."""
    rng = random.Random("tables")
    refs_a = [_seq(rng, 200) for _ in range(8)]
    refs_b = refs_a[1:] + refs_a[:1]
    a, b = Call(_table_items(rng, refs_a, DEFAULT)), Call(_table_items(rng, refs_b, DEFAULT))
    assert [len(l[0]) for l in a.ladders] == [len(l[0]) for l in b.ladders] and len(a.ladders) == len(b.ladders) == 8
    assert all(x != y for x, y in zip(a.ladders, b.ladders))
    assert all(_expect(it, DEFAULT)[0] == cm.OK and len(_expect(it, DEFAULT)[1]) == 3 for it in a.items + b.items)
    # b's reads against a's table are another result: a table left over from the call before would show
    stale = [cm.cigar_of(ra, it.read, it.fields) for ra, it in zip(refs_a, b.items)]
    assert all(s != _expect(it, DEFAULT)[:2] for s, it in zip(stale, b.items))
    a.check(ctx, DEFAULT)
    b.check(ctx, DEFAULT)
    a.check(ctx, DEFAULT)
    g = cm.golden()
    c = Call(b.items + _golden_items(g, [k for k in range(0, len(g["reads"]), 9) if len(g["reads"][k]) <= 250]) + a.items)
    assert len(c.ladders) > 16 and any(l[3] > 0 for l in c.ladders)
    c.check(ctx, DEFAULT)
    b.check(ctx, DEFAULT)


def test_a_small_call_after_a_large_one_and_a_larger_cap(ctx):
    large, small = _large_call(), _mixed_call()
    large.check(ctx, DEFAULT)
    Call(small.items, small.src[:3]).check(ctx, CHEAP_GAPS)
    small.check(ctx, CHEAP_GAPS, cap=97)                                     # more room per item than any call before
    large.check(ctx, DEFAULT, cap=3)


def test_release_and_a_call_that_works_again(ctx):
    call = _mixed_call()
    call.check(ctx, CHEAP_GAPS)
    ctx.lib.tredcigar_release(ctx.h)
    ctx.lib.tredcigar_release(ctx.h)                                      # nothing left to free
    call.check(ctx, CHEAP_GAPS)
    assert ctx.get_timing(_lib.KERNEL_CIGAR)[0] >= 1


def test_statuses_of_items_that_name_no_pair(ctx):
    rng = random.Random("statuses")
    g = cm.golden()
    periodic = next(k for k, l in enumerate(g["ladder"]) if g["ladders"][l][3] > 0)
    lad = g["ladders"][g["ladder"][periodic]]
    good = _golden_items(g, [periodic])[0]
    plain = _rect(rng, 100, 100, 10)
    long_read = _rect(rng, 481, 481, 10, pad=0)                           # TOO_LONG: a read of 481 bp
    ref512 = _seq(rng, 512)
    long_ref = Item((ref512, "A", "", 0), 0, ref512[5:105], (10, 5, 104, 0, 99))         # TOO_LONG: 512 columns
    ref511 = ref512[:511]
    fits = Item((ref511, "A", "", 0), 0, ref511[5:105], (10, 5, 104, 0, 99))
    items = [good, good, good, good, plain, plain, plain, long_read, long_ref, fits, good, plain]
    call = Call(items)
    n_l = len(call.ladders)
    ladder, template = call.ladder.copy(), call.template.copy()
    ladder[0], ladder[1] = -1, n_l
    template[2], template[3] = -1, 2 * lad[3]
    template[5], template[6] = -1, 1
    ops, n_ops, status = call.run(ctx, DEFAULT, ladder=ladder, template=template)
    B, T = _lib.CIGAR_BAD_ITEM, _lib.CIGAR_TOO_LONG
    assert list(status) == [B, B, B, B, 0, B, B, T, T, 0, 0, 0]
    want = call.want(DEFAULT)
    bad = status != 0
    assert not ops[bad].any() and not n_ops[bad].any()
    _same((ops[~bad], n_ops[~bad], status[~bad]), tuple(w[~bad] for w in want))
    # the last template of the ladder is still an item
    template[3] = 2 * lad[3] - 1
    assert call.run(ctx, DEFAULT, ladder=call.ladder, template=template)[2][3] != B


@pytest.mark.parametrize("scoring", [(0, 5, 7, 2), (9, 5, 7, 2), (1, -1, 7, 2), (1, 17, 7, 2), (1, 5, 0, 0), (1, 5, 17, 2),
                                     (1, 5, 7, 0), (1, 5, 7, 8)], ids=lambda s: "/".join(map(str, s)))
def test_scoring_just_outside_the_range_is_refused(ctx, scoring):
    call = Call(_mixed_call().items[:3])
    with pytest.raises(_lib.TredGpuError, match=r"\(-2\)"):
        call.run(ctx, scoring)
    call.check(ctx, DEFAULT)


def test_the_edges_of_the_scoring_range_are_accepted_and_no_room_is_refused(ctx):
    call = Call(_mixed_call().items[:3])
    with pytest.raises(_lib.TredGpuError, match=r"\(-2\)"):
        call.run(ctx, DEFAULT, cap=0)
    for scoring in ((8, 16, 16, 16), (1, 0, 1, 1)):
        call.check(ctx, scoring)


def test_aligner_takes_a_second_pass_for_more_than_32_operations(ctx):
    """480 bp with one base deleted every 25: 39 operations at 2/2/3/1, more than the 32 the first call has room for."""
    rng = random.Random("second pass")
    ref = _seq(rng, 499)
    read = "".join(ref[26 * k:26 * k + 25] for k in range(20))[:480]
    assert len(read) == 480
    ctx.reset_timing()
    al = ssw.Aligner(ref, report_cigar=True, ctx=ctx).align(read)
    assert ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 2
    fields = (al.score, al.ref_begin, al.ref_end, al.query_begin, al.query_end)
    st, ops = cm.cigar_of(ref, read, fields, 2, 2, 3, 1)
    assert st == cm.OK and len(ops) > 32 and sum(1 for v in ops if v & 15 == 2) >= 16
    assert al.cigar_string == ssw.PyAlignRes(fields, read, ref, ops).cigar_string
    assert [(n, op) for n, op in al.iter_cigar] == [(v >> 4, "MID"[v & 15]) for v in ops]
