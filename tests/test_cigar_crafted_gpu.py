"""GPU: the CIGAR kernel against tests/cigar_model.py on fields ssw_align never returns -- rectangles consistent in size
but cut or moved off the true alignment, with a score any band reaches.  There the traceback's first step can be a gap
(the reference then emits a zero-length M, ssw.c:698-715) or it leaves the band (OFF_EDGE): branches no golden or
fuzz item reaches.  (The closing `e op + 1M` did not appear in the model for any of these constructions either.)"""
import numpy as np
import pytest

from tredparse_amd import _lib

from . import cigar_model as cm

pytestmark = pytest.mark.gpu
VARIANTS = ((0, 0, 0, 0, -2), (0, 0, -3, 0, 0), (0, 0, 0, 3, 0), (0, 1, 0, 0, 0))     # added to {score, rb, re, qb, qe}


def test_kernel_equals_model_on_crafted_fields(ctx):
    g = cm.golden()
    base = [k for k, c in enumerate(g["cls"]) if c in "cde" and len(g["reads"][k]) <= 250][:40]
    idx, fields, want = [], [], []
    for k in base:
        for d in VARIANTS:
            f = np.array(g["fields"][k], np.int16) + np.array(d, np.int16)
            f[0] = 12
            if f[1] > f[2] or f[3] > f[4]:
                continue
            idx.append(k)
            fields.append(f)
            want.append(cm.cigar_of(g["refs"][k], g["reads"][k], f))
    assert sum(1 for st, ops in want if st == cm.OK and any(v >> 4 == 0 for v in ops)) >= 10       # zero-length M
    assert sum(1 for st, _ in want if st == cm.OFF_EDGE) >= 10
    idx = np.array(idx)
    reads = [g["reads"][k] for k in idx]
    packed, woff, rlen = _lib.pack_reads(reads)
    n, cap = len(idx), 32
    ops, n_ops, status = np.full((n, cap), 7, np.uint32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    ctx.sw_cigar(_lib.MEM_HOST, packed, woff, rlen, n, np.ascontiguousarray(g["ladder"][idx]), np.ascontiguousarray(g["template"][idx]),
                 np.ascontiguousarray(np.array(fields, np.int16)), _lib.default_sw_params(), cap, ops, n_ops, status, ladders=g["ladders"])
    for i, (st, w) in enumerate(want):
        assert status[i] == st, (i, idx[i], list(fields[i]), status[i], st)
        assert list(ops[i, :n_ops[i]]) == w and not ops[i, n_ops[i]:].any(), (i, idx[i], list(ops[i]), w)
