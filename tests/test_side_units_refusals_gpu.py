"""GPU: what the opt-in units (include/tredlong.h, tredcigar.h, tredsecond.h, tredpileup.h) refuse in host code before any
launch, called through ctx.lib directly: the return code together with the whole *_last_error() text.  The long path is
called with n_reads = 0 (its ladder table is checked, no kernel runs) and with one 481 bp read; the two CIGAR units, the
second-best unit and the pileup with one 20 bp item, which also pins what the harness they share (csrc/side_unit.h) owns:
a usable unit after every refusal, the fold of the event pool, and release twice over."""
import ctypes as C

import numpy as np
import pytest

from tredparse_amd import _lib

pytestmark = pytest.mark.gpu

LADDER = ("ACGTTGCAAT", "CAG", "TGACCTAGGT", 3)
LONG_SCORING = ("scoring out of the supported range (match 1..8, mismatch 0..16, 1 <= gap_extend <= gap_open <= 16, "
                "flank 0..255)")
CIGAR_SCORING = "scoring out of the supported range (match 1..8, mismatch 0..16, 1 <= gap_extend <= gap_open <= 16)"


def _table(ladders):
    arr = lambda k: (C.c_char_p * len(ladders))(*[l[k].encode() for l in ladders])
    return len(ladders), arr(0), arr(1), arr(2), np.asarray([l[3] for l in ladders], np.int32)


def _params(**kw):
    p = _lib.default_sw_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _long(ctx, ladder, p=None):
    n, pre, rep, suf, mu = _table([ladder])
    p = p or _lib.default_sw_params()
    rc = ctx.lib.tredlong_sw_classify(ctx.h, n, pre, rep, suf, _lib._ptr(mu), None, None, None, 0, None, C.byref(p),
                                      None, None, None, None, 0)
    return rc, ctx.lib.tredlong_last_error().decode()


@pytest.mark.parametrize("ladder,params,text", [
    (("ACGT", "CAG", "TTGA", -1), {}, "ladder 0: negative max_units"),
    (("ACGT", "", "TTGA", 2), {}, "ladder 0: empty repeat"),
    (("", "A", "", 0), {}, "ladder 0: reference length 0 not in [1,4095]"),
    (("A" * 2048, "C", "G" * 2047, 1), {}, "ladder 0: longest template 4096 exceeds TREDGPU_MAX_LONG_TEMPLATE_LEN=4095"),
    (LADDER, {"match": 0}, LONG_SCORING),
    (LADDER, {"flank": 256}, LONG_SCORING),
])
def test_long_path_refusals(ctx, ladder, params, text):
    assert _long(ctx, LADDER) == (0, "")
    assert _long(ctx, ladder, _params(**params)) == (-2, text)


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _one_item(ctx, unit, ladder=LADDER, p=None, **over):
    """One item on unit "cigar" or "long": the first 20 letters of LADDER's one-unit template of the reverse strand, against
    that template.  over replaces arguments of the entry point by name (a missing pointer is None; scoring: fields of the
    parameters)."""
    pre, rep, suf, _ = LADDER
    read = (_rc(suf) + _rc(rep) + _rc(pre))[:20]
    packed, woff, rlen = _lib.pack_reads([read])
    cap = over.get("cap", 8)
    if "scoring" in over:
        p = _params(**over.pop("scoring"))
    ops, n_ops, status = np.full((1, max(cap, 1)), 7, np.uint32), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    a = dict(prefix=(C.c_char_p * 1)(None if ladder[0] is None else ladder[0].encode()),
             repeat=(C.c_char_p * 1)(ladder[1].encode()), suffix=(C.c_char_p * 1)(ladder[2].encode()),
             max_units=np.asarray([ladder[3]], np.int32), packed=packed, read_off=woff, read_len=rlen, n_items=1,
             item_ladder=np.zeros(1, np.int32), item_template=np.ones(1, np.int32),
             fields=np.array([[20, 0, 19, 0, 19]], np.int16), params=p or _lib.default_sw_params(), cap=cap, out_ops=ops,
             out_n_ops=n_ops, out_status=status, mem=_lib.MEM_HOST)
    a.update(over)
    head = (ctx.h,) if unit == "long" else (ctx.h, a["mem"])
    call = ctx.lib.tredlong_sw_cigar if unit == "long" else ctx.lib.tredcigar_sw_cigar
    rc = call(*head, 1, a["prefix"], a["repeat"], a["suffix"], _lib._ptr(a["max_units"]), _lib._ptr(a["packed"]),
              _lib._ptr(a["read_off"]), _lib._ptr(a["read_len"]), a["n_items"], _lib._ptr(a["item_ladder"]),
              _lib._ptr(a["item_template"]), _lib._ptr(a["fields"]), None if a["params"] is None else C.byref(a["params"]),
              a["cap"], _lib._ptr(a["out_ops"]), _lib._ptr(a["out_n_ops"]), _lib._ptr(a["out_status"]))
    err = (ctx.lib.tredlong_last_error if unit == "long" else ctx.lib.tredcigar_last_error)().decode()
    return rc, err, (int(status[0]), list(ops[0, :max(int(n_ops[0]), 0)]))


def _cigar(ctx, ladder, p=None):
    return _one_item(ctx, "cigar", ladder, p)


GOOD = (0, "", (_lib.CIGAR_OK, [20 << 4]))


@pytest.mark.parametrize("ladder,params,text", [
    (("ACGT", "CAG", "TTGA", -1), {}, "ladder 0: negative max_units"),
    (("ACGT", "", "TTGA", 2), {}, "ladder 0: empty repeat"),
    (LADDER, {"match": 0}, CIGAR_SCORING),
    (LADDER, {"gap_extend": 8}, CIGAR_SCORING),
])
def test_cigar_refusals_leave_the_table_usable(ctx, ladder, params, text):
    assert _cigar(ctx, LADDER) == GOOD
    rc, err, _ = _cigar(ctx, ladder, _params(**params))
    assert (rc, err) == (-2, text)
    assert _cigar(ctx, LADDER) == GOOD          # the same operations as before the refusal


def test_cigar_does_not_check_flank(ctx):
    assert _cigar(ctx, LADDER, _params(flank=256)) == GOOD


def test_each_unit_reports_its_own_error(ctx):
    assert _cigar(ctx, LADDER) == GOOD
    assert _long(ctx, ("ACGT", "", "TTGA", 2))[1] == "ladder 0: empty repeat"
    assert ctx.lib.tredcigar_last_error() == b""
    assert _long(ctx, LADDER) == (0, "")
    assert _cigar(ctx, ("ACGT", "CAG", "TTGA", -1))[1] == "ladder 0: negative max_units"
    assert ctx.lib.tredlong_last_error() == b""


ARGS = "n_items, n_ladders and cap must be positive"
COMMON_REFUSALS = [      # the checks both entry points make, in their order
    (dict(n_items=-1), ARGS),
    (dict(cap=0), ARGS),
    (dict(repeat=None), "NULL ladder argument"),
    (dict(params=None), "params is NULL"),
    (dict(out_n_ops=None), "NULL array argument"),
    (dict(ladder=(None, "CAG", "TGACCTAGGT", 3)), "ladder 0: NULL sequence"),
    (dict(scoring=dict(gap_open=17)), CIGAR_SCORING),
    (dict(read_off=np.array([3, 0], np.int64)), "read_off must be monotone"),
]


@pytest.mark.parametrize("over,text", COMMON_REFUSALS + [
    (dict(read_off=np.array([0, 2], np.int64)), "item 0: its read does not lie inside packed[0 .. read_off[n_items])"),
    (dict(ladder=("A" * 2048, "C", "G" * 2047, 1)),
     "ladder 0: longest template 4096 exceeds TREDGPU_MAX_LONG_TEMPLATE_LEN=4095"),
])
def test_long_cigar_refusals_leave_the_unit_usable(ctx, over, text):
    assert _one_item(ctx, "long") == GOOD
    rc, err, _ = _one_item(ctx, "long", **over)
    assert (rc, err) == (-2, text)
    assert _one_item(ctx, "long") == GOOD


@pytest.mark.parametrize("over,text", COMMON_REFUSALS + [
    (dict(mem=2), "mem must be TREDGPU_MEM_HOST or TREDGPU_MEM_DEVICE"),
])
def test_cigar_argument_refusals_leave_the_unit_usable(ctx, over, text):
    assert _one_item(ctx, "cigar") == GOOD
    rc, err, _ = _one_item(ctx, "cigar", **over)
    assert (rc, err) == (-2, text)
    assert _one_item(ctx, "cigar") == GOOD


@pytest.mark.parametrize("unit,which", [("cigar", _lib.KERNEL_CIGAR), ("long", _lib.KERNEL_CIGAR_LONG)])
def test_event_pool_folds_beyond_256_calls(ctx, unit, which):
    """One event pair per call and 256 pairs held at the most: call 257 folds the finished ones into the totals."""
    ctx.reset_timing()
    for _ in range(260):
        assert _one_item(ctx, unit) == GOOD
    launches, ms = ctx.get_timing(which)
    assert launches == 260 and ms > 0
    assert ctx.get_timing(which) == (260, ms)               # nothing is counted twice
    ctx.reset_timing()
    assert ctx.get_timing(which) == (0, 0.0)


@pytest.mark.parametrize("unit", ["cigar", "long"])
def test_release_twice_then_a_good_call(ctx, unit):
    release = ctx.lib.tredlong_release if unit == "long" else ctx.lib.tredcigar_release
    assert _one_item(ctx, unit) == GOOD
    release(ctx.h)
    release(ctx.h)
    assert _one_item(ctx, unit) == GOOD


# ---- the second-best unit, the pileup and tredlong_sw_classify on the same harness -------------------------------------
def _table_args(ladder, a):
    return dict(prefix=(C.c_char_p * 1)(None if ladder[0] is None else ladder[0].encode()),
                repeat=(C.c_char_p * 1)(ladder[1].encode()), suffix=(C.c_char_p * 1)(ladder[2].encode()),
                max_units=np.asarray([ladder[3]], np.int32), **a)


def _second_item(ctx, ladder=LADDER, **over):
    """_one_item's item on tredsecond_sw_second with maskLen 10 (below 15: no second-best is reported)."""
    pre, rep, suf, _ = LADDER
    packed, woff, rlen = _lib.pack_reads([(_rc(suf) + _rc(rep) + _rc(pre))[:20]])
    p = _params(**over.pop("scoring")) if "scoring" in over else _lib.default_sw_params()
    out, status = np.full((1, 4), 7, np.int32), np.full(1, -1, np.int32)
    a = _table_args(ladder, dict(packed=packed, read_off=woff, read_len=rlen, n_items=1, item_ladder=np.zeros(1, np.int32),
                                 item_template=np.ones(1, np.int32), mask_len=np.full(1, 10, np.int32), params=p, out=out,
                                 out_status=status))
    a.update(over)
    rc = ctx.lib.tredsecond_sw_second(ctx.h, 1, a["prefix"], a["repeat"], a["suffix"], _lib._ptr(a["max_units"]),
                                      _lib._ptr(a["packed"]), _lib._ptr(a["read_off"]), _lib._ptr(a["read_len"]), a["n_items"],
                                      _lib._ptr(a["item_ladder"]), _lib._ptr(a["item_template"]), _lib._ptr(a["mask_len"]),
                                      None if a["params"] is None else C.byref(a["params"]), _lib._ptr(a["out"]),
                                      _lib._ptr(a["out_status"]))
    return rc, ctx.lib.tredsecond_last_error().decode(), (int(status[0]), out[0].tolist())


GOOD_SECOND = (0, "", (_lib.SECOND_OK, [20, 19, 0, -1]))
STRIDE = 32


def _pileup_item(ctx, ladder=LADDER, **over):
    """_one_item's item with its CIGAR, 20M, as the one item of one group."""
    pre, rep, suf, _ = LADDER
    packed, woff, rlen = _lib.pack_reads([(_rc(suf) + _rc(rep) + _rc(pre))[:20]])
    counts, status = np.full((1, STRIDE, _lib.PILEUP_CHANNELS), 7, np.int32), np.full(1, -1, np.int32)
    a = _table_args(ladder, dict(packed=packed, read_off=woff, read_len=rlen, n_items=1, item_ladder=np.zeros(1, np.int32),
                                 item_template=np.ones(1, np.int32), fields=np.array([[20, 0, 19, 0, 19]], np.int16),
                                 ops=np.array([[20 << 4, 0]], np.uint32), cap=2, n_ops=np.ones(1, np.int32),
                                 item_group=np.zeros(1, np.int32), n_groups=1, stride=STRIDE, out_counts=counts,
                                 out_status=status))
    a.update(over)
    rc = ctx.lib.tredpileup_pileup(ctx.h, 1, a["prefix"], a["repeat"], a["suffix"], _lib._ptr(a["max_units"]),
                                   _lib._ptr(a["packed"]), _lib._ptr(a["read_off"]), _lib._ptr(a["read_len"]), a["n_items"],
                                   _lib._ptr(a["item_ladder"]), _lib._ptr(a["item_template"]), _lib._ptr(a["fields"]),
                                   _lib._ptr(a["ops"]), a["cap"], _lib._ptr(a["n_ops"]), _lib._ptr(a["item_group"]),
                                   a["n_groups"], a["stride"], _lib._ptr(a["out_counts"]), _lib._ptr(a["out_status"]))
    return rc, ctx.lib.tredpileup_last_error().decode(), (int(status[0]), counts.tolist())


def _good_pileup():
    """The read is the reverse strand's first 20 letters of the one-unit template (23 columns): forward columns 22 .. 3,
    each with the forward template's own letter."""
    pre, rep, suf, _ = LADDER
    want = np.zeros((1, STRIDE, _lib.PILEUP_CHANNELS), np.int32)
    for c in range(3, 23):
        want[0, c, "ACGT".index((pre + rep + suf)[c])] = 1
    return 0, "", (_lib.PILEUP_OK, want.tolist())


GOOD_PILEUP = _good_pileup()
FLANKED = ("ACGTTGCAATCGGATCCTAGGTCAATGCCA", "CAG", "TGACCTAGGTTCAGGCATTCGAAGCTAAGC", 10)       # 30 bp flanks
_ACGT = lambda n, seed: "".join("ACGT"[i] for i in np.random.default_rng(seed).integers(0, 4, n))
LONG_READ = _ACGT(200, 3) + FLANKED[0] + "CAG" * 5 + FLANKED[2] + _ACGT(206, 4)
assert len(LONG_READ) == 481


def _classify_read(ctx, ladder=FLANKED, **over):
    """One 481 bp read on tredlong_sw_classify: it spans FLANKED's allele of five units."""
    packed, woff, rlen = _lib.pack_reads([LONG_READ])
    p = _params(**over.pop("scoring")) if "scoring" in over else _lib.default_sw_params()
    tag, h, sc = np.full(1, 77, np.uint8), np.full(1, 77, np.int16), np.full(1, 77, np.int16)
    a = _table_args(ladder, dict(packed=packed, read_off=woff, read_len=rlen, n_reads=1, read_ladder=np.zeros(1, np.int32),
                                 params=p, out_tag=tag, out_h=h, out_score=sc, out_dump=None, dump_templates=0))
    a.update(over)
    rc = ctx.lib.tredlong_sw_classify(ctx.h, 1, a["prefix"], a["repeat"], a["suffix"], _lib._ptr(a["max_units"]),
                                      _lib._ptr(a["packed"]), _lib._ptr(a["read_off"]), _lib._ptr(a["read_len"]), a["n_reads"],
                                      _lib._ptr(a["read_ladder"]), None if a["params"] is None else C.byref(a["params"]),
                                      _lib._ptr(a["out_tag"]), _lib._ptr(a["out_h"]), _lib._ptr(a["out_score"]),
                                      _lib._ptr(a["out_dump"]), a["dump_templates"])
    return rc, ctx.lib.tredlong_last_error().decode(), (int(tag[0]), int(h[0]), int(sc[0]))


INSIDE = "item 0: its read does not lie inside packed[0 .. read_off[n_items])"
SHARED_REFUSALS = [      # of call_refusal, set_ladders and reads_refusal, in their order
    (dict(n_items=-1), ARGS),
    (dict(repeat=None), "NULL ladder argument"),
    (dict(out_status=None), "NULL array argument"),
    (dict(ladder=(None, "CAG", "TGACCTAGGT", 3)), "ladder 0: NULL sequence"),
    (dict(read_off=np.array([3, 0], np.int64)), "read_off must be monotone"),
    (dict(read_off=np.array([0, 2], np.int64)), INSIDE),
]


@pytest.mark.parametrize("over,text", SHARED_REFUSALS + [
    (dict(params=None), "params is NULL"),
    (dict(scoring=dict(gap_open=17)), CIGAR_SCORING),
    (dict(ladder=("ACGT", "", "TTGA", 2)), "ladder 0: empty repeat"),
])
def test_second_refusals_leave_the_unit_usable(ctx, over, text):
    assert _second_item(ctx) == GOOD_SECOND
    rc, err, _ = _second_item(ctx, **over)
    assert (rc, err) == (-2, text)
    assert _second_item(ctx) == GOOD_SECOND


@pytest.mark.parametrize("over,text", SHARED_REFUSALS + [
    (dict(cap=0), ARGS),
    (dict(n_groups=-1), "n_groups must not be negative, nor out_counts NULL"),
    (dict(stride=29), "stride 29 must be at least the largest template length + 1 = 30 and at most 65536"),
    (dict(ladder=("ACGT", "", "TTGA", 2)), "ladder 0: empty repeat"),
])
def test_pileup_refusals_leave_the_unit_usable(ctx, over, text):
    assert _pileup_item(ctx) == GOOD_PILEUP
    rc, err, _ = _pileup_item(ctx, **over)
    assert (rc, err) == (-2, text)
    assert _pileup_item(ctx) == GOOD_PILEUP


@pytest.mark.parametrize("over,rc,text", [
    (dict(params=None), -2, "ctx or params is NULL"),
    (dict(repeat=None), -2, "bad ladder arguments"),
    (dict(n_reads=-1), -2, "negative n_reads"),
    (dict(out_h=None), -2, "NULL array argument"),
    (dict(out_dump=np.zeros((1, 6, 6), np.int16)), -2, "dump_templates must be > 0 with out_dump"),
    (dict(scoring=dict(flank=256)), -2, LONG_SCORING),
    (dict(ladder=(None, "CAG", "TGACCTAGGT", 3)), -2, "ladder 0: NULL sequence"),
    (dict(ladder=("", "A", "", 0)), -2, "ladder 0: reference length 0 not in [1,4095]"),
    (dict(ladder=("A" * 2048, "C", "G" * 2047, 1)), -2, "ladder 0: longest template 4096 exceeds TREDGPU_MAX_LONG_TEMPLATE_LEN=4095"),
    (dict(read_len=np.array([2049], np.int32)), -5, "read of 2049 bp exceeds TREDGPU_MAX_LONG_READ_LEN=2048"),
    (dict(read_ladder=np.ones(1, np.int32)), -2, "read 0: ladder 1 not given"),
    (dict(read_off=np.array([0, 40], np.int64)), -2, "read 0: read_off does not match read_len (tredgpu_pack_reads layout)"),
    (dict(read_off=np.array([-3, 44], np.int64)), -2, "read_off must be monotone"),     # (each read fits; the first begins before packed)
    # an earlier check wins: the table before the reads, a read's length before its ladder
    (dict(ladder=("ACGT", "", "TTGA", 2), read_len=np.array([2049], np.int32)), -2, "ladder 0: empty repeat"),
    (dict(read_len=np.array([-1], np.int32), read_ladder=np.ones(1, np.int32)), -5,
     "read of -1 bp exceeds TREDGPU_MAX_LONG_READ_LEN=2048"),
])
def test_long_classify_refusals_leave_the_unit_usable(ctx, over, rc, text):
    good = _classify_read(ctx)
    assert good == (0, "", (_lib.TAG_FULL, 5, 75))
    got = _classify_read(ctx, **over)
    assert got[:2] == (rc, text)
    assert _classify_read(ctx) == good


@pytest.mark.parametrize("call,good,which", [(_second_item, GOOD_SECOND, _lib.KERNEL_SECOND),
                                             (_pileup_item, GOOD_PILEUP, _lib.KERNEL_PILEUP)])
def test_event_pool_folds_beyond_256_calls_second_and_pileup(ctx, call, good, which):
    ctx.reset_timing()
    for _ in range(260):
        assert call(ctx) == good
    launches, ms = ctx.get_timing(which)
    assert launches == 260 and ms > 0
    assert ctx.get_timing(which) == (260, ms)               # nothing is counted twice
    ctx.reset_timing()
    assert ctx.get_timing(which) == (0, 0.0)


@pytest.mark.parametrize("call,release", [(_second_item, "tredsecond_release"), (_pileup_item, "tredpileup_release"),
                                          (_classify_read, "tredlong_release")])
def test_release_twice_then_a_good_call_on_the_other_units(ctx, call, release):
    good = call(ctx)
    assert good[:2] == (0, "")
    getattr(ctx.lib, release)(ctx.h)
    getattr(ctx.lib, release)(ctx.h)
    assert call(ctx) == good
