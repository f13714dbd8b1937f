"""GPU: what the two opt-in units (include/tredlong.h, include/tredcigar.h) refuse in host code before any launch, called
through ctx.lib directly: the return code together with the whole *_last_error() text.  The long path is called with
n_reads = 0 (its ladder table is checked, no kernel runs); the CIGAR unit with one 20 bp item."""
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


def _cigar(ctx, ladder, p=None):
    """One item: the first 20 letters of LADDER's one-unit template of the reverse strand, against that template."""
    pre, rep, suf, _ = LADDER
    read = (_rc(suf) + _rc(rep) + _rc(pre))[:20]
    packed, woff, rlen = _lib.pack_reads([read])
    n, pres, reps, sufs, mu = _table([ladder])
    fields = np.array([[20, 0, 19, 0, 19]], np.int16)
    item_ladder, item_template = np.zeros(1, np.int32), np.ones(1, np.int32)
    cap = 8
    ops, n_ops, status = np.full((1, cap), 7, np.uint32), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    p = p or _lib.default_sw_params()
    rc = ctx.lib.tredcigar_sw_cigar(ctx.h, _lib.MEM_HOST, n, pres, reps, sufs, _lib._ptr(mu), _lib._ptr(packed),
                                    _lib._ptr(woff), _lib._ptr(rlen), 1, _lib._ptr(item_ladder), _lib._ptr(item_template),
                                    _lib._ptr(fields), C.byref(p), cap, _lib._ptr(ops), _lib._ptr(n_ops), _lib._ptr(status))
    return rc, ctx.lib.tredcigar_last_error().decode(), (int(status[0]), list(ops[0, :max(int(n_ops[0]), 0)]))


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
