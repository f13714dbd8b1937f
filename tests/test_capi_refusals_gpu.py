"""GPU: what the host-memory entry points of the C ABI refuse, in which order, and what a refusal leaves behind.

Every refusal the six staged entry points (tredgpu_sw_classify, tredgpu_tally, tredgpu_likelihood_grid[_joint],
tredgpu_pe_kde, tredgpu_genotype_batch_joint, tredgpu_genotype_selected) and tredgpu_genotype_batch make from their
arguments alone: return code and the full text of tredgpu_last_error.  Calls with two faults pin which one is reported.
None of these launches a kernel; after all of them the valid call gives, on the same context, what the three separate
calls give.  Then calls of different kinds and growing sizes on one context against each call on a context of its own:
the staging buffers are shared between the call kinds and regrown between the calls."""
import ctypes as C

import numpy as np
import pytest

from oracle import lik_oracle as lo
from tredparse_amd import _lib, engine as engmod, synth
from tredparse_amd._lib import _ptr as P

pytestmark = pytest.mark.gpu
HD = ("GAGTCCCTCAAGTCCTTC", "CAG", "CAACAGCCGCCACCGCCG", 50)
HS = 52
JOINT_ROOM = 512

SCORING = "scoring out of the supported range (match 1..8, mismatch 0..16, 1 <= gap_extend <= gap_open <= 16)"
PACKED = ("scoring too large for the packed DP values: (rows + 511) * gap_extend + max_read_len * match must stay below "
          "8192 (is {})")
NULLARG = "NULL array argument"
NO_MODEL = "model constants not set (tredgpu_set_model)"
NO_LADDERS = "no ladders registered (tredgpu_set_ladders)"
SPAN = "unit_read_off must span [0,n_reads]"
SLICES = "unit {}: paired-end slices out of range"
LADDER = "unit {}: ladder {} not registered"
MARG = "marg_stride must exceed max(maxinsert, hist_stride)"
STRIDE = "hist_stride {} must exceed the max_units {} of unit {}'s ladder"
TOO_LONG = "read of 481 bp exceeds TREDGPU_MAX_READ_LEN=480"


def _model():
    step, w = lo.load_model()
    return np.array([step[p] for p in range(1, 7)]), np.array(w)


def _hd_locus():
    return [l for l in synth.load_loci() if l["name"] == "HD"][0]


def _valid():
    """The arguments of a valid call of every entry point: two units of one 36 bp read each on the HD ladder."""
    tmpl = HD[0] + "CAG" * 30 + HD[2]
    a = {}
    a["packed"], a["read_off"], a["read_len"] = _lib.pack_reads([tmpl[:36], tmpl[90:126]])
    a["n_reads"], a["n_units"] = 2, 2
    a["uro"], a["ulad"] = np.array([0, 1, 2], np.int32), np.zeros(2, np.int32)
    a["units"] = np.zeros(2, _lib.UNIT_DTYPE)
    a["units"][:] = synth.unit_params_for(_hd_locus(), 36, 30.0, 0, 0, 0, 0)
    a["params"] = _lib.default_sw_params()
    a["pair_id"] = None
    a["gl"], a["n_gl"], a["tl"], a["n_tl"] = np.zeros(1, np.int32), 0, np.zeros(1, np.int32), 0
    a["hs"], a["ms"] = HS, engmod._marg_stride(a["units"], HS)
    a["joff"] = np.arange(3, dtype=np.int64) * JOINT_ROOM
    a["mem"] = _lib.MEM_HOST
    a["dump"], a["dump_templates"], a["grid_off"], a["grid_dump"] = None, 0, None, None
    # what a tally of these reads could have left, for the calls that take histograms
    a["full"], a["pref"], a["rept"] = (np.zeros((2, HS), np.int32) for _ in range(3))
    a["full"][:, 20] = 4
    return _outputs(a)


def _outputs(a):
    """a with fresh output arrays."""
    a = dict(a)
    n, g = max(a["n_reads"], 1), a["n_units"]
    a["tag"], a["h"], a["score"] = np.zeros(n, np.uint8), np.zeros(n, np.int16), np.zeros(n, np.int16)
    a["out_rept"] = np.zeros((g, a["hs"]), np.int32)
    a["out_full"], a["out_pref"] = np.zeros((g, a["hs"]), np.int32), np.zeros((g, a["hs"]), np.int32)
    a["calls"] = np.zeros(g, _lib.CALL_DTYPE)
    a["marg"] = np.zeros((g, 2, a["ms"]), np.float64)
    a["joint"] = np.zeros((int(a["joff"][-1]), 3), np.float64)
    a["jn"], a["jt"] = np.zeros(g, np.int32), np.zeros(g, np.float64)
    a["pdf"], a["kde_status"] = np.zeros((g, _lib.SPAN), np.float64), np.zeros(g, np.int32)
    return a


def _ref(p):
    return C.byref(p) if p is not None else None


# one function per entry point: (ctx, arguments) -> return code
def joint(ctx, v):
    return ctx.lib.tredgpu_genotype_batch_joint(
        ctx.h, P(v["packed"]), P(v["read_off"]), P(v["read_len"]), v["n_reads"], P(v["uro"]), P(v["ulad"]), P(v["units"]),
        v["n_units"], _ref(v["params"]), P(v["pair_id"]), P(v["gl"]), v["n_gl"], P(v["tl"]), v["n_tl"], P(v["tag"]), P(v["h"]),
        P(v["score"]), v["hs"], P(v["out_rept"]), P(v["calls"]), P(v["marg"]), v["ms"], P(v["joff"]), P(v["joint"]), P(v["jn"]),
        P(v["jt"]))


def batch(ctx, v):
    return ctx.lib.tredgpu_genotype_batch(
        ctx.h, v["mem"], P(v["packed"]), P(v["read_off"]), P(v["read_len"]), v["n_reads"], P(v["uro"]), P(v["ulad"]),
        P(v["units"]), v["n_units"], _ref(v["params"]), P(v["pair_id"]), P(v["gl"]), v["n_gl"], P(v["tl"]), v["n_tl"],
        P(v["tag"]), P(v["h"]), P(v["score"]), v["hs"], P(v["out_full"]), P(v["out_pref"]), P(v["out_rept"]), P(v["calls"]))


def classify(ctx, v):
    return ctx.lib.tredgpu_sw_classify(
        ctx.h, v["mem"], P(v["packed"]), P(v["read_off"]), P(v["read_len"]), v["n_reads"], P(v["uro"]), P(v["ulad"]),
        v["n_units"], _ref(v["params"]), P(v["tag"]), P(v["h"]), P(v["score"]), P(v["dump"]), v["dump_templates"])


def tally(ctx, v):
    return ctx.lib.tredgpu_tally(ctx.h, v["mem"], P(v["tag"]), P(v["h"]), v["n_reads"], P(v["uro"]), v["n_units"],
                                 P(v["pair_id"]), v["hs"], P(v["out_full"]), P(v["out_pref"]), P(v["out_rept"]))


def grid(ctx, v):
    return ctx.lib.tredgpu_likelihood_grid(
        ctx.h, v["mem"], P(v["units"]), v["n_units"], v["hs"], P(v["full"]), P(v["pref"]), P(v["rept"]), P(v["gl"]), v["n_gl"],
        P(v["tl"]), v["n_tl"], P(v["calls"]), P(v["grid_off"]), P(v["grid_dump"]), P(v["marg"]), v["ms"])


def grid_joint(ctx, v):
    return ctx.lib.tredgpu_likelihood_grid_joint(
        ctx.h, v["mem"], P(v["units"]), v["n_units"], v["hs"], P(v["full"]), P(v["pref"]), P(v["rept"]), P(v["gl"]), v["n_gl"],
        P(v["tl"]), v["n_tl"], P(v["calls"]), P(v["marg"]), v["ms"], P(v["joff"]), P(v["joint"]), P(v["jn"]), P(v["jt"]))


def kde(ctx, v):
    return ctx.lib.tredgpu_pe_kde(ctx.h, v["mem"], P(v["units"]), v["n_units"], P(v["gl"]), v["n_gl"], P(v["pdf"]),
                                  P(v["kde_status"]))


def selected(ctx, v):
    """tredgpu_genotype_selected without an inflater: one segment that names none."""
    seg = (_lib.SelectedUnits * 1)(_lib.SelectedUnits(None, 2, 0, None))
    off = v.get("unit_off", np.array([0, 1, 2], np.int64))
    return ctx.lib.tredgpu_genotype_selected(
        ctx.h, seg if v.get("segs", True) else None, v.get("n_segs", 1), P(v["uro"]), P(off), P(off), P(off), P(v["ulad"]),
        P(v["units"]), v["n_units"], _ref(v["params"]), P(v["gl"]), v["n_gl"], P(v["tl"]), v["n_tl"], P(v["tag"]), P(v["h"]),
        P(v["score"]), v["hs"], P(v["out_rept"]), P(v["calls"]), P(v["marg"]), v["ms"], P(v["joff"]), P(v["joint"]), P(v["jn"]),
        P(v["jt"]), P(v["read_len"]), P(v["read_off"]), P(v["tag"]), P(v["read_off"]), P(v["tag"]))


def _units(a, *changes):
    """a's units with (unit, field, value) changed."""
    u = a["units"].copy()
    for g, field, value in changes:
        u[g][field] = value
    return u


def _sw(*fields):
    return _lib.SwParams(*fields)


def _table(a):
    """(entry point, mutation of the valid call, return code, text)."""
    i32 = lambda *x: np.array(x, np.int32)
    over_args = _sw(1, 5, 13, 13, 9, 0, 100, 0)          # (112 + 511) * 13 + 100: refused from the arguments
    over_seen = _sw(8, 9, 5, 5, 9, 0, 0, 0)              # passes for the 320 bp assumed; a 400 bp read: (512 + 511) * 5 + 400 * 8
    sw_checks = [
        (dict(params=None), -2, "params is NULL"),
        (dict(params=_sw(1, 5, 2, 7, 9, 0, 0, 0)), -2, SCORING),
        (dict(params=_sw(9, 5, 7, 2, 9, 0, 0, 0)), -2, SCORING),
        (dict(params=_sw(1, 5, 7, 2, 256, 0, 0, 0)), -2, "flank out of range"),
        (dict(params=over_args), -2, PACKED.format(8199)),
    ]
    rows = []
    for fn in (classify, joint, batch, selected):
        rows += [(fn,) + r for r in sw_checks]
    rows += [
        # tredgpu_sw_classify
        (classify, dict(n_reads=-1), -2, "negative sizes"),
        (classify, dict(n_units=-1), -2, "negative sizes"),
        (classify, dict(packed=None), -2, NULLARG),
        (classify, dict(score=None), -2, NULLARG),
        (classify, dict(dump=np.zeros((2, 100, 6), np.int16), dump_templates=0), -2, "dump_templates must be > 0 with out_dump"),
        (classify, dict(mem=7), -2, "mem must be TREDGPU_MEM_HOST or TREDGPU_MEM_DEVICE"),
        (classify, dict(uro=i32(1, 1, 2)), -2, SPAN),
        (classify, dict(uro=i32(0, 1, 3)), -2, SPAN),
        (classify, dict(uro=i32(0, 3, 2)), -2, "unit_read_off not monotone at 1"),
        (classify, dict(ulad=i32(0, 3)), -2, LADDER.format(1, 3)),
        (classify, dict(ulad=i32(-1, 0)), -2, LADDER.format(0, -1)),
        (classify, dict(read_len=i32(36, 481)), -5, TOO_LONG),
        (classify, dict(read_len=i32(36, 400), params=over_seen), -2, PACKED.format(8315)),
        # tredgpu_tally
        (tally, dict(hs=0), -2, "bad sizes"),
        (tally, dict(n_reads=-1), -2, "bad sizes"),
        (tally, dict(n_units=-1), -2, "bad sizes"),
        (tally, dict(out_full=None), -2, NULLARG),
        (tally, dict(uro=None), -2, NULLARG),
        (tally, dict(tag=None), -2, NULLARG),
        (tally, dict(mem=7), -2, "bad mem"),
        # tredgpu_likelihood_grid / _joint
        (grid, dict(n_units=-1), -2, "negative n_units"),
        (grid, dict(units=None), -2, "units is NULL"),
        (grid, dict(hs=0), -2, "hist_stride must be > 0"),
        (grid, dict(full=None), -2, NULLARG),
        (grid, dict(calls=None), -2, NULLARG),
        (grid, dict(grid_off=np.zeros(3, np.int64)), -2, "grid_off and grid_dump go together"),
        (grid, dict(grid_dump=np.zeros(6, np.float64)), -2, "grid_off and grid_dump go together"),
        (grid, dict(ms=0), -2, "marg_stride must be > 0"),
        (grid, dict(mem=7), -2, "bad mem"),
        (grid, dict(units=_units(a, (1, "pe_off", -1))), -2, SLICES.format(1)),
        (grid, dict(units=_units(a, (0, "n_global", 1))), -2, SLICES.format(0)),
        (grid, dict(units=_units(a, (0, "tl_off", 1), (0, "n_target", 0))), -2, SLICES.format(0)),
        (grid, dict(ms=int(a["units"]["maxinsert"].max())), -2, MARG),
        (grid_joint, dict(joff=None), -2, "joint_off is NULL"),
        (grid_joint, dict(joint=None), -2, "joint_off, joint, joint_n and joint_total go together"),
        (grid_joint, dict(jt=None), -2, "joint_off, joint, joint_n and joint_total go together"),
        (grid_joint, dict(units=_units(a, (1, "n_target", -1))), -2, SLICES.format(1)),
        # tredgpu_pe_kde
        (kde, dict(n_units=-1), -2, "bad arguments"),
        (kde, dict(units=None), -2, "bad arguments"),
        (kde, dict(pdf=None), -2, "bad arguments"),
        (kde, dict(mem=7), -2, "bad mem"),
        # tredgpu_genotype_batch_joint
        (joint, dict(n_units=-1), -2, "negative n_units"),
        (joint, dict(units=None), -2, "units is NULL"),
        (joint, dict(n_units=0), -2, "bad sizes"),
        (joint, dict(n_reads=-1), -2, "bad sizes"),
        (joint, dict(ulad=None), -2, NULLARG),
        (joint, dict(marg=None), -2, NULLARG),
        (joint, dict(jn=None), -2, NULLARG),
        (joint, dict(ms=0), -2, NULLARG),
        (joint, dict(read_len=None), -2, NULLARG),
        (joint, dict(tag=None), -2, NULLARG),
        (joint, dict(uro=i32(0, 1, 3)), -2, SPAN),
        (joint, dict(uro=i32(0, 3, 2)), -2, "unit_read_off not monotone at 1"),
        (joint, dict(ulad=i32(0, 3)), -2, LADDER.format(1, 3)),
        (joint, dict(hs=50, ms=a["ms"]), -2, STRIDE.format(50, 50, 0)),
        (joint, dict(units=_units(a, (1, "pe_off", -1))), -2, SLICES.format(1)),
        (joint, dict(units=_units(a, (0, "n_target", 1))), -2, SLICES.format(0)),
        (joint, dict(ms=int(a["units"]["maxinsert"].max())), -2, MARG),
        (joint, dict(units=_units(a, (1, "maxinsert", a["ms"]))), -2, MARG),
        (joint, dict(read_len=i32(36, 481)), -5, TOO_LONG),
        (joint, dict(read_len=i32(36, 400), params=over_seen), -2, PACKED.format(8315)),
        # ... two faults in one call: the first offending unit decides, not the first kind of check
        (joint, dict(units=_units(a, (0, "pe_off", -1)), ulad=i32(0, 3)), -2, SLICES.format(0)),
        (joint, dict(units=_units(a, (0, "pe_off", -1)), ulad=i32(3, 0)), -2, LADDER.format(0, 3)),
        (joint, dict(uro=i32(0, 3, 2), ulad=i32(3, 0)), -2, LADDER.format(0, 3)),
        (joint, dict(units=_units(a, (1, "pe_off", -1)), read_len=i32(36, 481)), -2, SLICES.format(1)),
        (joint, dict(hs=50, ms=50), -2, STRIDE.format(50, 50, 0)),
        (grid, dict(units=_units(a, (0, "maxinsert", a["ms"]), (1, "pe_off", -1))), -2, MARG),
        (grid, dict(units=_units(a, (0, "pe_off", -1), (1, "maxinsert", a["ms"]))), -2, SLICES.format(0)),
        # tredgpu_genotype_selected, as far as it goes without an inflater
        (selected, dict(n_units=-1), -2, "negative n_units"),
        (selected, dict(n_units=0), -2, "bad sizes"),
        (selected, dict(n_segs=0), -2, "bad sizes"),
        (selected, dict(segs=False), -2, "bad sizes"),
        (selected, dict(unit_off=None), -2, NULLARG),
        (selected, dict(marg=None), -2, NULLARG),
        (selected, dict(ms=0), -2, NULLARG),
        (selected, dict(), -2, "params.max_read_len must name the longest selected read"),
        (selected, dict(params=_lib.default_sw_params(max_read_len=481)), -2, "params.max_read_len must name the longest selected read"),
        (selected, dict(params=_lib.default_sw_params(max_read_len=36), unit_off=np.array([1, 1, 2], np.int64)), -2,
         "unit offsets must start at 0"),
        (selected, dict(params=_lib.default_sw_params(max_read_len=36), uro=i32(1, 1, 2)), -2, "unit offsets must start at 0"),
        (selected, dict(params=_lib.default_sw_params(max_read_len=36), tag=None), -2, NULLARG),
        (selected, dict(params=_lib.default_sw_params(max_read_len=36)), -2, "segment 0: bad unit list"),
        # tredgpu_genotype_batch
        (batch, dict(n_units=-1), -2, "negative n_units"),
        (batch, dict(units=None), -2, "units is NULL"),
        (batch, dict(hs=50), -2, "hist_stride 50 must exceed the largest max_units 50"),
        (batch, dict(n_reads=-1), -2, "negative n_reads"),
        (batch, dict(out_pref=None), -2, NULLARG),
        (batch, dict(read_off=None), -2, NULLARG),
        (batch, dict(mem=7), -2, "bad mem"),
        # ... HOST memory composes the three host calls: their refusals come through
        (batch, dict(uro=i32(0, 1, 3)), -2, SPAN),
        (batch, dict(ulad=i32(0, 3)), -2, LADDER.format(1, 3)),
        (batch, dict(read_len=i32(36, 481)), -5, TOO_LONG),
    ]
    return rows


def _refusals(ctx, a, rows):
    """The rows whose call did not return the code and leave the text the row names."""
    bad = []
    for k, (fn, change, code, text) in enumerate(rows):
        rc = fn(ctx, dict(a, **change))
        got = ctx.lib.tredgpu_last_error(ctx.h).decode()
        if (rc, got) != (code, text):
            bad.append((k, fn.__name__, sorted(change), (rc, got), (code, text)))
    return bad


def _sorted_joint(v, u):
    lo_, n = int(v["joff"][u]), int(v["jn"][u])
    return sorted(map(tuple, v["joint"][lo_:lo_ + n].tolist()))


def test_a_fresh_context_asks_for_the_model_then_the_ladders():
    a = _valid()
    ctx = _lib.Context(0)
    try:
        assert _refusals(ctx, a, [(fn, {}, -4, NO_MODEL) for fn in (joint, batch, grid, grid_joint)] +
                         [(selected, dict(params=_lib.default_sw_params(max_read_len=36)), -4, NO_MODEL),
                          (classify, {}, -4, NO_LADDERS)]) == []
        ctx.set_model(*_model())
        assert _refusals(ctx, a, [(fn, {}, -4, NO_LADDERS) for fn in (joint, batch, classify)] +
                         [(selected, dict(params=_lib.default_sw_params(max_read_len=36)), -4, NO_LADDERS)]) == []
    finally:
        ctx.close()


def test_every_refusal_by_code_and_text_then_the_valid_call(ctx):
    a = _valid()
    ctx.set_ladders([HD])
    ctx.set_model(*_model())
    rows = _table(a)
    assert len(rows) >= 100
    assert _refusals(ctx, a, rows) == []
    # (c) the valid call on the same context, against the three separate calls: nothing of a refused call is left in the
    # pinned arena or among the pending read-backs
    one = _outputs(a)
    assert joint(ctx, one) == 0, ctx.lib.tredgpu_last_error(ctx.h)
    b = engmod.PackedUnits()
    b.clip, b._picks, b._texts, b.pair_id = False, None, None, None
    b.packed, b.read_off, b.read_len, b.n_reads = a["packed"], a["read_off"], a["read_len"], 2
    b.unit_read_off, b.n_units, b.ladder_keys, b.max_units = a["uro"], 2, [HD, HD], HD[3]
    b.params, b.global_lens, b.target_lens = a["units"], np.zeros(0, np.int32), np.zeros(0, np.int32)
    eng = engmod.Engine(0, ctx=ctx)                # (not closed: the context is the session's)
    assert engmod.JOINT_CAP == JOINT_ROOM and eng._register(b.ladder_keys).tolist() == [0, 0]
    three = eng._genotype_packed_stepwise(b)
    print("tags", one["tag"], "h", one["h"], "status", one["calls"]["status"], "joint_n", one["jn"])
    for key, other in (("tag", three.tag), ("h", three.h), ("score", three.score), ("out_rept", three.rept),
                       ("calls", three.calls), ("marg", three.marg)):
        assert one[key].tobytes() == np.ascontiguousarray(other).tobytes(), key
    for u in range(2):           # (the entries of a unit arrive in any order: compare them sorted)
        assert _sorted_joint(one, u) == sorted(map(tuple, three.joint[u][0].tolist())), u
        assert one["jt"][u] == three.joint[u][1]
    # (d) no reads at all: every unit is "no evidence"
    none = _outputs(dict(a, n_reads=0, uro=np.zeros(3, np.int32), read_off=None, packed=None, read_len=None))
    assert joint(ctx, none) == 0, ctx.lib.tredgpu_last_error(ctx.h)
    assert none["calls"]["status"].tolist() == [1, 1]
    assert (one["tag"] != _lib.TAG_NONE).all() and (one["calls"]["status"] == 0).all() and (one["jn"] > 0).all()


# ---- buffer reuse ---------------------------------------------------------------------------------------------------

def _big():
    """6 units of about 400 reads on three ladders registered after HD, with the histograms a tally gives them."""
    loci = [l for l in synth.load_loci() if l["name"] in ("HD", "DM2", "SCA10")]
    b = synth.build_batch(77, loci, 2, synth.SynthParams(coverage=20, readlen=150))
    a = dict(packed=b.packed, read_off=b.read_off, read_len=b.read_len, n_reads=b.n_reads, n_units=b.n_units,
             uro=b.unit_read_off, ulad=(b.unit_ladder + 1).astype(np.int32), units=b.units,
             params=_lib.default_sw_params(), pair_id=None, gl=engmod._pad(b.global_lens), n_gl=len(b.global_lens),
             tl=engmod._pad(b.target_lens), n_tl=len(b.target_lens), hs=b.hist_stride, mem=_lib.MEM_HOST,
             dump=None, dump_templates=0, grid_off=None, grid_dump=None)
    a["ms"] = engmod._marg_stride(b.units, b.hist_stride)
    a["joff"] = np.arange(b.n_units + 1, dtype=np.int64) * 4096        # (room for every (h1, h2) pair of a unit)
    return a, [HD] + list(b.ladders)


def _fresh(ladders):
    ctx = _lib.Context(0)
    ctx.set_ladders(ladders)
    ctx.set_model(*_model())
    return ctx


def _results(fn, ctx, a, keys):
    """What call fn writes into fresh arrays of a: {key: bytes}, a unit's joint entries sorted (they arrive in any order)."""
    v = _outputs(a)
    assert fn(ctx, v) == 0, ctx.lib.tredgpu_last_error(ctx.h)
    out = {k: v[k].tobytes() for k in keys}
    if "jn" in keys:
        assert (v["jn"] <= np.diff(v["joff"])).all()       # (else which entries were kept depends on their order)
        out["joint"] = [_sorted_joint(v, u) for u in range(a["n_units"])]
    return out, v


FUSED = ("tag", "h", "score", "out_rept", "calls", "marg", "jn", "jt")


def test_calls_of_different_kinds_and_growing_sizes_share_the_staging_buffers():
    small = _valid()
    big, ladders = _big()
    assert big["n_units"] == 6 and 200 < big["n_reads"] < 800 and big["hs"] == HS
    tmpl = HD[0] + "CAG" * 30 + HD[2]
    ten = ["A", "ACGTA", "N" * 150, "", tmpl[:160], tmpl[5:155], "CAG" * 50, "acgt" * 30 + "nnn", tmpl[:64], tmpl[3:115]]
    dumped = dict(small, n_reads=10, n_units=1, uro=np.array([0, 10], np.int32), ulad=np.zeros(1, np.int32),
                  dump_templates=2 * HD[3])
    dumped["packed"], dumped["read_off"], dumped["read_len"] = _lib.pack_reads(ten)

    def classify_dump(ctx, v):
        v["dump"] = np.zeros((10, 2 * HD[3], 6), np.int16)
        return classify(ctx, v)

    # the histograms and the pair counts the dense grid call of the 6 units needs: from a context of their own
    prep = _fresh(ladders)
    try:
        _, v = _results(batch, prep, big, ())
        dense = dict(big, full=v["out_full"], pref=v["out_pref"], rept=v["out_rept"])
        dense["grid_off"] = np.zeros(7, np.int64)
        dense["grid_off"][1:] = np.cumsum(np.maximum(v["calls"]["n_pairs"], 1))
        assert (v["calls"]["status"] == 0).sum() >= 4
    finally:
        prep.close()

    def grid_dense(ctx, v):
        v["grid_dump"] = np.zeros((int(v["grid_off"][-1]), 6), np.float64)
        return grid(ctx, v)

    steps = [(joint, small, FUSED), (classify_dump, dumped, ("tag", "h", "score", "dump")), (joint, big, FUSED),
             (kde, big, ("pdf", "kde_status")), (grid_dense, dense, ("calls", "marg", "grid_dump")), (joint, small, FUSED)]
    alone = []
    for fn, a, keys in steps[:-1]:
        ctx = _fresh(ladders)
        try:
            alone.append(_results(fn, ctx, a, keys)[0])
        finally:
            ctx.close()
    alone.append(alone[0])
    ctx = _fresh(ladders)
    try:
        for k, (fn, a, keys) in enumerate(steps):
            got = _results(fn, ctx, a, keys)[0]
            for key in got:
                assert got[key] == alone[k][key], (k, fn.__name__, key)
    finally:
        ctx.close()
