"""GPU: the CIGAR of long alignments (tredparse_amd/csrc/sw_cigar_long.hip through Context.sw_cigar with the long-read path
on): the reference's long goldens (tests/golden/sw_cigar_long.npz), the routing between tredlong_sw_cigar and
tredcigar_sw_cigar, rectangles on either side of the 64-lane chunks and at the limits, every status, wavefront slots that
take a second and a third item, and what a context keeps between calls.

Expected operations of crafted items are tests/cigar_rowpar_model.py's -- equal to the serial model on small rectangles and
pinned to the compiled reference by the goldens (tests/test_cigar_long_model.py) -- and are compared exactly.
"""
import random

import numpy as np
import pytest

from tredparse_amd import _lib, ssw

from . import cigar_model as cm
from . import cigar_rowpar_model as rp
from .test_cigar_shapes_gpu import Call, Item, _golden_items, _moved, _rect, _same, _seq, _want_arrays

pytestmark = pytest.mark.gpu
CAP = 32
DEFAULT, CHEAP, DEAR = (1, 5, 7, 2), (2, 2, 3, 1), (8, 16, 16, 1)
SLOTS = _lib.LONG_CIGAR_SLOTS
_expected = {}


@pytest.fixture(scope="module")
def lctx(ctx):
    """A context of its own, so that the switch never reaches the other test modules' session context (`ctx` first:
    torch's HIP runtime is loaded before the library's, conftest.py)."""
    c = _lib.Context(0)
    c.set_long_reads(True)
    yield c
    c.close()


def _expect(item, scoring):
    """(status, ops, bands) of the row-parallel model for the item, computed once per (item, scoring)."""
    key = (item, scoring)
    if key not in _expected:
        st, ops, passes = rp.passes_of(cm.template(item.ladder, item.template), item.read, item.fields, *scoring)
        _expected[key] = (st, ops, [b for b, _ in passes])
    return _expected[key]


def _want(call, scoring, cap=CAP):
    ops, n_ops, status = _want_arrays([_expect(it, scoring)[:2] for it in call.items], cap)
    return ops[call.src], n_ops[call.src], status[call.src]


def _check(call, ctx, scoring, cap=CAP):
    got = call.run(ctx, scoring, cap)
    _same(got, _want(call, scoring, cap), call)
    return got


def _is_long(item):
    l = item.ladder
    return len(item.read) > _lib.MAX_READ_LEN or (len(l[0]) + len(l[2]) + len(l[1]) * l[3] if l[3] else len(l[0])) > _lib.MAX_TEMPLATE_LEN


def _on_long_ref(rng, it):
    """The item on a reference lengthened to at least 520 columns (behind the rectangle): a long item whatever its read."""
    ref = it.ladder[0] + _seq(rng, max(0, 520 - len(it.ladder[0])))
    return Item((ref, "A", "", 0), 0, it.read, it.fields)


def _width(item, scoring):
    """Band cells of the widest row the kernel runs for the item (0: refused before a pass)."""
    ref_len = item.fields[2] - item.fields[1] + 1
    return max([min(2 * b + 1, ref_len) for b in _expect(item, scoring)[2]] + [0])


# ---- 1. the reference's goldens -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", [DEFAULT, CHEAP, DEAR], ids=lambda s: "/".join(map(str, s)))
def test_kernel_reproduces_the_long_goldens(lctx, scoring):
    g = rp.golden_long()
    ks = [k for k, v in enumerate(g["scoring"]) if v == scoring]
    call = Call(_golden_items(g, ks))
    assert len(ks) >= 8 and all(_is_long(it) for it in call.items) and max(len(g["ops"][k]) for k in ks) <= CAP
    lctx.reset_timing()
    _same(call.run(lctx, scoring), _want_arrays([(cm.OK, g["ops"][k]) for k in ks], CAP), call)
    assert lctx.get_timing(_lib.KERNEL_CIGAR_LONG)[0] == 1 and lctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0


# ---- 2. routing -----------------------------------------------------------------------------------------------------------------
def _routing_items():
    g, gl = cm.golden(), rp.golden_long()
    short = _golden_items(g, list(range(0, len(g["reads"]), 7))[:40])
    long_ks = [k for k, v in enumerate(gl["scoring"]) if v == DEFAULT and gl["cls"][k] in ("La", "Lb", "Ld")][:30]
    return short, _golden_items(gl, long_ks), [gl["ops"][k] for k in long_ks]


def test_a_shuffled_call_is_one_launch_of_each_kernel(ctx, lctx):
    short, long_, long_ops = _routing_items()
    assert len(short) >= 30 and len(long_) >= 20 and not any(_is_long(it) for it in short) and all(_is_long(it) for it in long_)
    src = np.arange(len(short) + len(long_))
    np.random.RandomState(20261019).shuffle(src)
    is_long = src >= len(short)
    assert is_long[:10].any() and (~is_long[:10]).any()
    off = Call(short).run(ctx, DEFAULT)                                   # the short items alone, the path off
    assert (off[2] == cm.OK).all()
    call = Call(short + long_, src)
    lctx.reset_timing()
    got = call.run(lctx, DEFAULT)
    assert lctx.get_timing(_lib.KERNEL_CIGAR_LONG)[0] == 1 and lctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1
    for a, b in zip(got, off):
        assert np.array_equal(a[~is_long][np.argsort(src[~is_long])], b)
    want = _want_arrays([(cm.OK, o) for o in long_ops], CAP)
    _same(tuple(a[is_long][np.argsort(src[is_long])] for a in got), want)
    # a call of short items only stays one launch of the short kernel
    lctx.reset_timing()
    assert all(np.array_equal(a, b) for a, b in zip(Call(short).run(lctx, DEFAULT), off))
    assert lctx.get_timing(_lib.KERNEL_CIGAR_LONG)[0] == 0 and lctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1


def test_long_items_with_the_path_off_are_too_long(ctx):
    _, long_, _ = _routing_items()
    ops, n_ops, status = Call(long_).run(ctx, DEFAULT)
    assert (status == _lib.CIGAR_TOO_LONG).all() and not ops.any() and not n_ops.any()


def test_a_device_memory_call_with_a_long_item_is_refused(lctx):
    short, long_, _ = _routing_items()
    with pytest.raises(_lib.TredGpuError, match="host-memory calls"):
        Call(short[:3] + long_[:1]).run(lctx, DEFAULT, device=True)
    rng = random.Random("device")
    ref = _seq(rng, 600)                                                  # a read of 100 bp on a ladder of 600 columns
    with pytest.raises(_lib.TredGpuError, match="host-memory calls"):
        Call([Item((ref, "A", "", 0), 0, ref[50:150], (10, 50, 149, 0, 99))]).run(lctx, DEFAULT, device=True)
    got = Call(short[:5]).run(lctx, DEFAULT, device=True)                 # short items go on as before
    assert (got[2] == cm.OK).all()


# ---- 3. chunk and size boundaries ---------------------------------------------------------------------------------------------
def _boundary_items():
    """[(name, item, scoring, cells of the widest row)]: where the gap is long, at a scoring that makes it worth taking."""
    rng = random.Random("long boundaries")
    out = []
    for cells in (3, 63, 65, 127, 129):                                   # 2 * band + 1, a deletion and an insertion
        d = (cells - 1) // 2 - 1
        out += [("del, {} cells".format(cells), _rect(rng, 500 + d, 500, 20), CHEAP, cells),
                ("ins, {} cells".format(cells), _rect(rng, 500 - d, 500, 20, pad=1), CHEAP, cells)]
    out += [("64 columns x 150", _on_long_ref(rng, _rect(rng, 64, 150, 20)), DEAR, 64),      # the whole reference side in every row
            ("128 columns x 500", _rect(rng, 128, 500, 20), DEAR, 128)]
    ref = _seq(rng, 700)
    out += [("readLen 1", Item((ref, "A", "", 0), 0, ref[340], (2, 0, 699, 0, 0)), CHEAP, 700),
            ("the band never moves", _rect(rng, 1300, 600, 20), DEAR, 1300),          # band 701 > every row
            ("the band moves from row 102", _rect(rng, 700, 600, 20), CHEAP, 203)]
    return out


def test_rows_on_either_side_of_the_chunks(lctx):
    cases = _boundary_items()
    for name, it, scoring, cells in cases:
        st, ops, bands = _expect(it, scoring)
        assert st == cm.OK and len(ops) <= 3 and len(bands) == 1 and _width(it, scoring) == cells and _is_long(it), (name, bands, st)
    assert _expect(cases[-2][1], DEAR)[2][0] >= 600 and _expect(cases[-1][1], CHEAP)[2][0] == 101
    for scoring in (CHEAP, DEAR):
        call = Call([it for _, it, s, _ in cases if s == scoring])
        _check(call, lctx, scoring)
        _check(Call(call.items, np.arange(call.n)[::-1]), lctx, DEFAULT)     # (other paths, whatever their status)


def test_a_single_column_under_700_rows(lctx):
    """refLen == 1 on a long template: the traceback walks up the one column, or off it."""
    rng = random.Random("one column")
    ref = _seq(rng, 600)
    items = [Item((ref, "A", "", 0), 0, _seq(rng, k) + ref[5] + _seq(rng, 699 - k), (2, 5, 5, 0, 699)) for k in (0, 300, 699)]
    assert all(_width(it, CHEAP) == 1 and _expect(it, CHEAP)[2] == [700] for it in items)
    assert {_expect(it, CHEAP)[0] for it in items} <= {cm.OK, cm.OFF_EDGE}
    _check(Call(items), lctx, CHEAP)


FULL_600 = 8 * 250 - (16 + 349)            # 100 M, 350 I, 150 M


def test_a_600_x_700_rectangle_whose_earlier_bands_fail(lctx):
    """The read's first 100 bases lie on the diagonal 450 columns to the right: only the band that covers the rectangle
    holds the path, and 150 matches (1 200) stay below its score."""
    rng = random.Random("full cover 600")
    x, a, b = _seq(rng, 450), _seq(rng, 100), _seq(rng, 150)
    it = Item((x + a + b, "A", "", 0), 0, a + _seq(rng, 350) + b, (FULL_600, 0, 699, 0, 599))
    st, ops, bands = _expect(it, DEAR)
    assert st == cm.OK and bands == [101, 202, 404, 699] and ops == [100 << 4, 350 << 4 | 1, 150 << 4]
    _check(Call([it]), lctx, DEAR)


FULL_2048 = 8 * 1095 - (16 + 952)          # 500 M, 953 I, 595 M


def _largest_item():
    rng = random.Random("full cover 2048")
    x, a, b = _seq(rng, 3000), _seq(rng, 500), _seq(rng, 595)
    return Item((x + a + b, "A", "", 0), 0, a + _seq(rng, 953) + b, (FULL_2048, 0, 4094, 0, 2047))


def test_the_2048_x_4095_rectangle_at_full_cover(lctx):
    it = _largest_item()
    st, ops, bands = _expect(it, DEAR)
    assert st == cm.OK and bands == [2048, 4094] and ops == [500 << 4, 953 << 4 | 1, 595 << 4]
    lctx.reset_timing()
    _check(Call([it]), lctx, DEAR)
    print("2048 x 4095 at full cover: {:.1f} ms".format(lctx.get_timing(_lib.KERNEL_CIGAR_LONG)[1]))


# ---- 4. statuses ----------------------------------------------------------------------------------------------------------------
def _status_items():
    rng = random.Random("long statuses")
    base = [_rect(rng, 520 + d, 500, 20, pad=rng.randint(1, 4)) for d in (0, 3, 40, 70, 100)]
    base += [_rect(rng, 500, 500 + d, 20, pad=rng.randint(1, 4)) for d in (5, 66)]
    many = _rect(rng, 640, 600, 20)                                        # and two short indels: five operations
    f = many.fields
    read = many.read[:f[3] + 50] + "TT" + many.read[f[3] + 50:f[4] - 60] + many.read[f[4] - 57:]
    many = Item(many.ladder, 0, read, (f[0], f[1], f[2], f[3], f[4] - 1))
    return base, many


def test_no_path_off_edge_and_overflow(lctx):
    base, many = _status_items()
    items = base + _moved(base, CHEAP, far=True)
    items = [x for it in items for x in (it, many)]                        # every other item has five operations
    sts = [_expect(it, CHEAP)[0] for it in items[0::2]]
    assert sts.count(cm.NO_PATH) >= 5 and sts.count(cm.OFF_EDGE) >= 5 and sts.count(cm.OK) >= 10
    assert _expect(many, CHEAP)[0] == cm.OK and len(_expect(many, CHEAP)[1]) >= 5
    call = Call(items)
    got = _check(call, lctx, CHEAP)
    bad = np.isin(got[2], (cm.NO_PATH, cm.OFF_EDGE))
    assert not got[0][bad].any() and not got[1][bad].any()
    got = _check(call, lctx, CHEAP, cap=4)                                 # room for four operations
    n = len(_expect(many, CHEAP)[1])
    assert (got[2][1::2] == _lib.CIGAR_OVERFLOW).all() and (got[1][1::2] == n).all() and not got[0][1::2].any()
    keep = np.array([_expect(it, CHEAP)[0] == cm.OK and len(_expect(it, CHEAP)[1]) <= 4 for it in items])
    assert keep.sum() >= 10 and (got[2][keep] == cm.OK).all() and got[0][keep].any(axis=1).all()      # neighbours intact


def test_statuses_of_items_that_name_no_pair(lctx):
    rng = random.Random("long bad items")
    g = rp.golden_long()
    periodic = next(k for k, l in enumerate(g["ladder"]) if g["ladders"][l][3] > 0 and g["scoring"][k] == DEFAULT)
    lad = g["ladders"][g["ladder"][periodic]]
    good = _golden_items(g, [periodic])[0]
    plain = _rect(rng, 600, 600, 10)
    too_long = _rect(rng, 2049, 2049, 10, pad=0)                           # TOO_LONG: a read of 2 049 bp
    fits = _rect(rng, 2048, 2048, 10, pad=0)
    items = [good, good, good, good, plain, plain, plain, too_long, fits, good, plain, plain, plain]
    call = Call(items)
    ladder, template, fields = call.ladder.copy(), call.template.copy(), call.fields.copy()
    ladder[0], ladder[1] = -1, len(call.ladders)
    template[2], template[3] = -1, 2 * lad[3]
    template[5], template[6] = -1, 1
    fields[10] = (10, 0, len(plain.ladder[0]), 0, 599)                     # ref_end == the template's length
    fields[11] = (10, 5, 4, 0, 599)                                        # end < begin
    call.fields = fields
    ops, n_ops, status = call.run(lctx, DEFAULT, ladder=ladder, template=template)
    B, T = _lib.CIGAR_BAD_ITEM, _lib.CIGAR_TOO_LONG
    assert list(status) == [B, B, B, B, 0, B, B, T, 0, 0, B, B, 0]
    bad = status != 0
    assert not ops[bad].any() and not n_ops[bad].any()
    want = _want(Call(items), DEFAULT)
    _same((ops[~bad], n_ops[~bad], status[~bad]), tuple(w[~bad] for w in want))


def test_a_ladder_of_4096_columns_is_refused(lctx):
    rng = random.Random("4096")
    ref = _seq(rng, 4096)
    with pytest.raises(_lib.TredGpuError, match=r"tredlong_sw_cigar failed \(-2\).*4096 exceeds TREDGPU_MAX_LONG_TEMPLATE_LEN"):
        Call([Item((ref, "A", "", 0), 0, ref[5:605], (10, 5, 604, 0, 599))]).run(lctx, DEFAULT)
    it = Item((ref[:4095], "A", "", 0), 0, ref[3495:4095], (10, 3495, 4094, 0, 599))
    assert _check(Call([it]), lctx, DEFAULT)[2][0] == cm.OK               # 4 095 columns, read to the last one
    with pytest.raises(_lib.TredGpuError, match=r"\(-2\)"):
        Call([it]).run(lctx, (1, 5, 7, 8))                                 # gap_extend > gap_open: the scan relies on the order
    with pytest.raises(_lib.TredGpuError, match=r"tredlong_sw_cigar failed \(-2\)"):
        Call([it]).run(lctx, DEFAULT, cap=0)


# ---- 5. slots that take a second and a third item --------------------------------------------------------------------------
_reuse = {}


def _reuse_call():
    """3 * SLOTS + 1 items from about 40 distinct ones, all on references of 520-900 columns: slot s takes items s,
    s + SLOTS, s + 2 * SLOTS, each narrower than the one before, among them items that end OFF_EDGE and NO_PATH."""
    if _reuse:
        return _reuse["call"]
    rng = random.Random("slots")

    def on_long_ref(it):
        return _on_long_ref(rng, it)

    def group(diffs, n):
        ok = [on_long_ref(_rect(rng, n + d, n, 20, pad=rng.randint(0, 3)) if k % 2 else
                          _rect(rng, n, n + d, 20, pad=rng.randint(0, 3))) for k, d in enumerate(diffs)]
        off = [it for it in _moved(ok[:4], CHEAP) if _expect(it, CHEAP)[0] == cm.OFF_EDGE][:3]
        return ok, off

    wide, wide_off = group((120, 130, 150, 170, 190, 210, 230, 250), 300)         # rows of 241 cells and more
    none = [Item(it.ladder, 0, it.read, (30000,) + it.fields[1:]) for it in wide[:3]]      # NO_PATH: the whole rectangle
    mid, mid_off = group((34, 40, 47, 55, 63, 64, 70, 80), 200)                   # 71 to 163 cells
    small = [on_long_ref(_rect(rng, 40, 40 - rng.randint(0, 3), 10)) for _ in range(3)]
    mid_none = [Item(it.ladder, 0, it.read, (30000,) + it.fields[1:]) for it in small]      # NO_PATH on 40 columns
    narrow, _ = group((16, 1, 2, 3, 5, 8, 12, 0), 150)                            # 3 to 35 cells
    narrow.append(on_long_ref(_rect(rng, 30, 30, 10)))
    turns = [wide + wide_off + none, mid + mid_off + mid_none, narrow]
    items, src = [], []
    for t in turns:
        first = len(items)
        items += t
        src += [first + (k * 5) % len(t) for k in range(SLOTS)]
    src.append(len(items) - 1)
    _reuse["call"] = Call(items, src)
    return _reuse["call"]


def test_every_slot_takes_a_second_and_a_third_item(lctx):
    call = _reuse_call()
    assert call.n == 3 * SLOTS + 1 and 35 <= len(call.items) <= 50 and all(_is_long(it) for it in call.items)
    width = np.array([_width(it, CHEAP) for it in call.items])[call.src]
    st = np.array([_expect(it, CHEAP)[0] for it in call.items])[call.src]
    a, b = slice(0, call.n - SLOTS), slice(SLOTS, call.n)                     # an item and its slot's next one
    assert (width[a] > width[b]).all()                                        # every slot, twice, after a wider item
    assert ((st[a] == cm.OFF_EDGE) & (st[b] == cm.OK)).sum() >= 10
    assert ((st[a] == cm.NO_PATH) & (st[b] == cm.OK)).sum() >= 10
    assert ((st[a] == cm.OK) & (st[b] == cm.OK)).sum() >= 100
    lctx.reset_timing()
    _check(call, lctx, CHEAP)
    print("slot reuse, {} items: {:.1f} ms".format(call.n, lctx.get_timing(_lib.KERNEL_CIGAR_LONG)[1]))


# ---- 6. what a context keeps between calls ------------------------------------------------------------------------------------
def test_a_small_call_after_the_largest_one(lctx):
    large, small = Call([_largest_item()]), Call(_reuse_call().items[-3:])
    _check(large, lctx, DEAR)
    _check(small, lctx, CHEAP)
    _check(_reuse_call(), lctx, CHEAP)                                        # more slots than the call before
    _check(small, lctx, CHEAP, cap=97)


def test_release_and_a_call_that_works_again(lctx):
    call = Call(_reuse_call().items)
    _check(call, lctx, CHEAP)
    lctx.lib.tredlong_release(lctx.h)
    lctx.lib.tredlong_release(lctx.h)                                        # nothing left to free
    lctx.reset_timing()
    _check(call, lctx, CHEAP)
    assert lctx.get_timing(_lib.KERNEL_CIGAR_LONG)[0] == 1


# ---- 7. the Aligner ---------------------------------------------------------------------------------------------------------------
def test_aligner_gives_the_references_texts(lctx):
    g = rp.golden_long()
    assert len(g["texts"]) == 8
    for k, text in sorted(g["texts"].items()):
        al = ssw.Aligner(g["refs"][k], *g["scoring"][k], report_cigar=True, ctx=lctx).align(g["reads"][k])
        assert [al.score, al.ref_begin, al.ref_end, al.query_begin, al.query_end] == list(g["fields"][k]), k
        assert al.cigar_string == al.cigar == text["cigar_string"], k
        assert list(al.alignment) == text["alignment"] and str(al) == text["str"], k


def test_the_shared_context_takes_the_switch(ctx):
    """ssw.set_long_reads: Aligners without a context of their own report long alignments while it is on."""
    g = rp.golden_long()
    k, text = sorted(g["texts"].items())[0]
    aligner = ssw.Aligner(g["refs"][k], *g["scoring"][k], report_cigar=True)
    ssw.set_long_reads(True)
    try:
        al = aligner.align(g["reads"][k])
        assert al.cigar_string == text["cigar_string"] and str(al) == text["str"]
    finally:
        ssw.set_long_reads(False)                  # (with the long reference still registered)
    short = ssw.Aligner("ACGTACGTTTGACCAGTCAGGCTAGCTAGGATCGATCGGCTA", report_cigar=True).align("TTGACCAGTCAGGCTAGCTAGG")
    assert short.cigar_string == "22M"
    with pytest.raises(_lib.TredGpuError):
        aligner.align(g["reads"][k])


def test_a_second_pass_when_only_the_long_items_overflow(lctx):
    """2 048 bp with one base deleted every 25: far more than the 32 operations the first call has room for.  The Aligner
    asks again with the room the kernel reported; in a mixed call, as Engine.alignments makes it, the short items are done
    in the first round and everything fits in the second."""
    rng = random.Random("second pass, long")
    ref = _seq(rng, 2200)
    read = "".join(ref[26 * k:26 * k + 25] for k in range(82))[:2048]
    assert len(read) == 2048
    lctx.reset_timing()
    al = ssw.Aligner(ref, report_cigar=True, ctx=lctx).align(read)
    assert lctx.get_timing(_lib.KERNEL_CIGAR_LONG)[0] == 2 and lctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0
    fields = (al.score, al.ref_begin, al.ref_end, al.query_begin, al.query_end)
    st, ops = rp.cigar_of(ref, read, fields, *CHEAP)
    assert st == cm.OK and len(ops) > 100 and sum(1 for v in ops if v & 15 == 2) >= 50
    assert al.cigar_string == ssw.PyAlignRes(fields, read, ref, ops).cigar_string
    assert [(n, op) for n, op in al.iter_cigar] == [(v >> 4, "MID"[v & 15]) for v in ops]
    g = cm.golden_scorings()
    short = _golden_items(g, [k for k, v in enumerate(g["scoring"]) if v == CHEAP][:6])
    call = Call(short[:3] + [Item((ref, "A", "", 0), 0, read, fields)] + short[3:])
    got = call.run(lctx, CHEAP)
    assert list(got[2]) == [0, 0, 0, _lib.CIGAR_OVERFLOW, 0, 0, 0] and got[1][3] == len(ops) == got[1].max() and not got[0][3].any()
    again = call.run(lctx, CHEAP, cap=int(got[1].max()))
    assert (again[2] == cm.OK).all() and list(again[0][3]) == ops
    for k in (0, 1, 2, 4, 5, 6):
        assert np.array_equal(again[0][k, :CAP], got[0][k]) and again[1][k] == got[1][k]
