"""GPU: what tredlong_sw_classify (csrc/sw_long.hip) keeps between the calls on a context -- the cached ladder table and
the grow-only staging buffers -- called through ctx.lib directly.  A call on a context that has served other tables and
other sizes must give, bit for bit (tag / h / score / dump), what the same call gives on a fresh context; that the values
themselves are the reference's is test_long_reads_gpu's and test_long_sw_shapes_gpu's matter."""
import ctypes as C

import numpy as np
import pytest

from tredparse_amd import _lib

pytestmark = pytest.mark.gpu

MU = 30
X = ("ACGTTGCAATCGGATCCTAGGTCAATG", "CAG", "TGACCTAGGTTCAGGCATTCGAAGCTA", MU)      # period 3
Y = ("ACGTTGCAATCGGATCCTAGGTCAATG", "CCTGA", "TGACCTAGGTTCAGGCATTCGAAGCTA", MU)    # period 5: as many ladders and units
NT = 2 * MU + 3          # rows of a read's dump: three more than the ladder has templates, which keep the fill
GUARD = 2                # rows of the caller's dump behind the call's, which the call must not touch


def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _reads(lengths, seed=5):
    """Reads of the given lengths cut from a genome that holds X's allele of 20 units and Y's of 12."""
    rng = np.random.default_rng(seed)
    g = (_rand(rng, 2100) + X[0] + X[1] * 20 + X[2] + _rand(rng, 300) + Y[0] + Y[1] * 12 + Y[2] + _rand(rng, 2100))
    mid = 2100 + len(X[0]) + 30
    return [g[max(0, mid - L // 2 - 7 * k):][:L] for k, L in enumerate(lengths)]


def _classify(ctx, ladder, reads, dump=True):
    packed, woff, rlen = _lib.pack_reads(reads)
    n = len(reads)
    tag, h, sc = np.full(n, 77, np.uint8), np.full(n, 77, np.int16), np.full(n, 77, np.int16)
    d = np.full((n + GUARD, NT, 6), 0x5A5A, np.int16) if dump else None
    pre, rep, suf = [(C.c_char_p * 1)(ladder[k].encode()) for k in range(3)]
    mu = np.asarray([ladder[3]], np.int32)
    p = _lib.default_sw_params()
    rc = ctx.lib.tredlong_sw_classify(ctx.h, 1, pre, rep, suf, _lib._ptr(mu), _lib._ptr(packed), _lib._ptr(woff),
                                      _lib._ptr(rlen), n, _lib._ptr(np.zeros(n, np.int32)), C.byref(p), _lib._ptr(tag),
                                      _lib._ptr(h), _lib._ptr(sc), _lib._ptr(d), NT if dump else 0)
    assert (rc, ctx.lib.tredlong_last_error()) == (0, b"")
    if dump:
        assert (d[n:] == 0x5A5A).all()                       # nothing behind the call's region of the caller's array
        assert (d[:n, 2 * ladder[3]:] == -1).all()           # the 0xFF fill, where the ladder has no template
        assert (d[:n, :2 * ladder[3], 5] >= 0).all()         # and a tag in every row it has one for
    return tag.tobytes(), h.tobytes(), sc.tobytes(), (d[:n].tobytes() if dump else None)


def _fresh(ctx, *args, **kw):
    """The same call on a context of its own (`ctx` first: torch's HIP runtime is loaded before the library's)."""
    c = _lib.Context(0)
    try:
        return _classify(c, *args, **kw)
    finally:
        c.close()


def test_a_cached_table_is_replaced_by_the_call_s(ctx):
    reads = _reads([500, 533, 567, 600])
    want = {lad: _fresh(ctx, lad, reads) for lad in (X, Y)}
    assert want[X] != want[Y] and want[X][0] != bytes(4)     # the tables tell the reads apart, and some read is tagged
    for lad in (X, Y, X, X, Y):
        assert _classify(ctx, lad, reads) == want[lad]


@pytest.mark.parametrize("dump", [True, False])
def test_buffers_grow_and_are_reused(ctx, dump):
    one = _reads([481])
    many = _reads([481, 600, 1025, 2048] * 10, seed=9)
    first = _classify(ctx, X, one, dump)
    assert _classify(ctx, X, many, dump) == _fresh(ctx, X, many, dump)
    assert _classify(ctx, X, one, dump) == first             # (on buffers the 40 reads have grown and written)
    ctx.lib.tredlong_release(ctx.h)
    ctx.lib.tredlong_release(ctx.h)
    assert _classify(ctx, X, one, dump) == first
