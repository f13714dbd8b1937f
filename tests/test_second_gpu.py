"""GPU: the second-best kernel (include/tredsecond.h, tredparse_amd/csrc/sw_second.hip) against the values of the compiled
reference (tests/golden/sw_second.npz: seven scorings, padding rows, the pass boundary, the mask's edges, every row class)
and ssw.Aligner(report_secondary=True) against the same values and the reference's texts."""
import numpy as np
import pytest

from tredparse_amd import _lib, ssw

from . import second_model as sm

pytestmark = pytest.mark.gpu
SCORINGS = [(1, 5, 7, 2), (2, 2, 3, 1), (1, 16, 16, 1), (4, 6, 10, 1), (8, 16, 16, 16), (8, 0, 1, 1), (1, 1, 1, 1)]
MAX_WAVES = 2560            # wavefronts of a row class's launch at the most (sw_second.hip)


@pytest.fixture(scope="module")
def lctx(ctx):
    """A long-reads context of its own (`ctx` first: torch's HIP runtime is loaded before the library's, conftest.py)."""
    c = _lib.Context(0)
    c.set_long_reads(True)
    yield c
    c.close()


def _params(scoring):
    return _lib.SwParams(*[int(v) for v in scoring], 9, 0, 0, 0)


def _of(g, scoring):
    return np.array([k for k in range(len(g["reads"])) if tuple(g["scoring"][k]) == tuple(scoring)])


def _run(ctx, g, idx, scoring, ladders=None, ladder=None, template=None, mask=None, reads=None):
    reads = [g["reads"][k] for k in idx] if reads is None else reads
    packed, woff, rlen = _lib.pack_reads(reads)
    n = len(reads)
    out, status = np.full((n, 4), 77, np.int32), np.full(n, -1, np.int32)
    ctx.sw_secondary(packed, woff, rlen, n, np.ascontiguousarray(g["ladder"][idx] if ladder is None else ladder, np.int32),
                     np.ascontiguousarray(g["template"][idx] if template is None else template, np.int32),
                     np.ascontiguousarray(g["mask_len"][idx] if mask is None else mask, np.int32), _params(scoring), out, status,
                     ladders=g["ladders"] if ladders is None else ladders)
    return out, status


def _check(g, idx, out, status):
    assert (status == _lib.SECOND_OK).all(), [(int(k), int(s)) for k, s in zip(idx, status) if s][:5]
    bad = [int(k) for i, k in enumerate(idx) if not np.array_equal(out[i], g["expect"][k])]
    assert not bad, [(k, g["cls"][k], len(g["reads"][k]), list(g["expect"][k]), list(out[list(idx).index(k)])) for k in bad[:5]]


@pytest.mark.parametrize("scoring", SCORINGS, ids=lambda s: "/".join(map(str, s)))
def test_every_golden_item_short_and_long_shuffled(ctx, scoring):
    """All four values, the items of a scoring in one call in a shuffled order: at 1/5/7/2 reads of 15 to 2 048 bp, all six
    row classes, side by side."""
    g = sm.golden()
    idx = _of(g, scoring)
    assert len(idx) >= 58
    idx = idx[np.random.default_rng(5).permutation(len(idx))]
    _check(g, idx, *_run(ctx, g, idx, scoring))


@pytest.mark.parametrize("scoring", [s for s in SCORINGS if s != (8, 16, 16, 16)], ids=lambda s: "/".join(map(str, s)))
def test_score1_and_ref_end1_are_those_of_sw_classify(lctx, scoring):
    """The unit computes score1 / ref_end1 itself; the SW kernels' dump row of the same pair says the same.  (8/16/16/16 is
    beyond sw_classify's packed-value bound for short reads and has no dump to compare with.)"""
    g = sm.golden()
    idx = _of(g, scoring)
    n = len(idx)
    lctx.set_ladders(g["ladders"])
    packed, woff, rlen = _lib.pack_reads([g["reads"][k] for k in idx])
    nt = max(max(2 * l[3], 1) for l in g["ladders"])
    tag, h, sc = np.zeros(n, np.uint8), np.zeros(n, np.int16), np.zeros(n, np.int16)
    dump = np.zeros((n, nt, 6), np.int16)
    lctx.sw_classify(_lib.MEM_HOST, packed, woff, rlen, n, np.arange(n + 1, dtype=np.int32),
                     np.ascontiguousarray(g["ladder"][idx]), n, _params(scoring), tag, h, sc, dump, nt)
    rows = dump[np.arange(n), g["template"][idx]]
    out, status = _run(lctx, g, idx, scoring)
    _check(g, idx, out, status)
    assert np.array_equal(rows[:, 0], out[:, 0]) and np.array_equal(rows[:, 2], out[:, 1])


def test_more_items_than_wavefronts(ctx):
    """3 * MAX_WAVES + 37 items of one row class: every wavefront takes a second and a third item, shorter ones after a
    longer one, and the column maxima the longer one left in LDS must not show."""
    g = sm.golden()
    idx = _of(g, (1, 5, 7, 2))
    idx = np.array(sorted((k for k in idx if len(g["reads"][k]) <= 64 and g["mask_len"][k] >= 15), key=lambda k: -len(g["refs"][k])))
    assert len(idx) >= 40 and len(g["reads"][idx[0]]) > 30
    n = 3 * MAX_WAVES + 37
    order = np.concatenate([np.resize(idx[:8], MAX_WAVES), np.resize(idx[8:], n - MAX_WAVES)])
    assert min(len(g["refs"][k]) for k in order[:MAX_WAVES]) > np.median([len(g["refs"][k]) for k in order[MAX_WAVES:]])
    _check(g, order, *_run(ctx, g, order, (1, 5, 7, 2)))


def test_statuses_and_refusals(ctx):
    g = sm.golden()
    idx = _of(g, (1, 5, 7, 2))[:12]
    reads = [g["reads"][k] for k in idx]
    ladders = list(g["ladders"]) + [("ACGT" * 1024, "A", "", 0), ("ACGTTGCA", "CAG", "TTGACC", 5)]
    long_lad, rep_lad = len(ladders) - 2, len(ladders) - 1
    ladder, template = np.array(g["ladder"][idx]), np.array(g["template"][idx])
    reads[1] = "ACGT" * 512 + "A"                    # 2 049 bp
    ladder[3] = long_lad                             # 4 096 columns
    ladder[5] = -1
    ladder[6] = len(ladders)
    ladder[8], template[8] = rep_lad, 10             # a ladder of 5 units has the templates 0..9
    template[9] = 1                                  # a plain reference has template 0 only
    template[10] = -1
    out, status = _run(ctx, g, idx, (1, 5, 7, 2), ladders=ladders, ladder=ladder, template=template, reads=reads)
    want = np.zeros(12, np.int32)
    want[[1, 3]] = _lib.SECOND_TOO_LONG
    want[[5, 6, 8, 9, 10]] = _lib.SECOND_BAD_ITEM
    assert list(status) == list(want)
    assert not out[want != 0].any()                                                    # a refused item's outputs are zero
    keep = np.nonzero(want == 0)[0]
    _check(g, idx[keep], out[keep], status[keep])
    # the ladder with template 9 = 5 units, reverse strand, is taken
    out, status = _run(ctx, g, idx[:1], (1, 5, 7, 2), ladders=ladders, ladder=[rep_lad], template=[9], reads=["GGTCAACTGCTGCTGCTGCTGTGCAACGT"],
                       mask=[15])
    assert status[0] == 0 and tuple(out[0]) == sm.second("GGTCAACTGCTGCTGCTGCTGTGCAACGT", sm.template(ladders[rep_lad], 9), (1, 5, 7, 2), 15)
    assert out[0, 0] == 29
    for bad in ((9, 5, 7, 2), (1, 17, 7, 2), (1, 5, 2, 3), (1, 5, 17, 2), (0, 5, 7, 2)):
        with pytest.raises(_lib.TredGpuError, match=r"tredsecond_sw_second failed \(-2\): scoring out of the supported range"):
            _run(ctx, g, idx, bad)
    with pytest.raises(_lib.TredGpuError, match=r"tredsecond_sw_second failed \(-2\)"):
        ctx.sw_secondary(None, None, None, 3, None, None, None, _params((1, 5, 7, 2)), None, None, ladders=g["ladders"])
    # zero items: nothing is read, written or launched
    before = ctx.get_timing(_lib.KERNEL_SECOND)[0]
    ctx.sw_secondary(None, None, None, 0, None, None, None, _params((1, 5, 7, 2)), None, None, ladders=g["ladders"])
    assert ctx.get_timing(_lib.KERNEL_SECOND)[0] == before
    _check(g, idx, *_run(ctx, g, idx, (1, 5, 7, 2)))                                   # and the next call works


def _aligner_items(g, scoring, short):
    """The items an Aligner reproduces: a plain reference, rule 4's mask_len, within the short kernels' limits or beyond."""
    return [k for k in _of(g, scoring) if g["ladders"][g["ladder"][k]][3] == 0 and g["mask_len"][k] == sm.mask_len_of(g["reads"][k])
            and (len(g["reads"][k]) <= _lib.MAX_READ_LEN and len(g["refs"][k]) <= _lib.MAX_TEMPLATE_LEN) == short]


def test_aligner_report_secondary(ctx):
    g = sm.golden()
    ks = _aligner_items(g, (1, 5, 7, 2), True)
    assert {30, 31, 32} <= {len(g["reads"][k]) for k in ks} and len(ks) >= 60
    ctx.reset_timing()
    seen2 = 0
    for k in ks:
        read, ref, e = g["reads"][k], g["refs"][k], [int(v) for v in g["expect"][k]]
        a = ssw.Aligner(ref, 1, 5, 7, 2, report_secondary=True, ctx=ctx).align(read)
        assert (a.score, a.ref_end, a.score2, a.ref_end2) == tuple(e), (k, g["cls"][k])
        tail = "SUB-OPTIMAL MATCH\nScore 2           {}\nRef_end2          {}\n".format(e[2], e[3]) if e[2] else ""
        assert str(a).endswith("Query end        {}\n".format(a.query_end) + tail) and ("SUB-OPTIMAL" in str(a)) == bool(e[2])
        seen2 += bool(e[2])
    assert seen2 >= 50
    assert ctx.get_timing(_lib.KERNEL_SECOND)[0] == len(ks) and ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0
    # several queries, one call; together with the CIGAR one launch each, the extra lines behind the CIGAR's
    ctx.reset_timing()
    k = next(k for k in ks if g["cls"][k] == "m" and g["expect"][k][2] > 0)
    read, ref, e = g["reads"][k], g["refs"][k], g["expect"][k]
    al = ssw.Aligner(ref, 1, 5, 7, 2, report_secondary=True, report_cigar=True, ctx=ctx).align_many([read, read[3:], "ACGT", read])
    assert ctx.get_timing(_lib.KERNEL_SECOND)[0] == 1 and ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1 and ctx.get_timing(_lib.KERNEL_SW)[0] == 1
    assert (al[0].score2, al[0].ref_end2) == (al[3].score2, al[3].ref_end2) == (e[2], e[3])
    assert str(al[0]).endswith("Cigar_string     {}M\nSUB-OPTIMAL MATCH\nScore 2           {}\nRef_end2          {}\n".format(len(read), e[2], e[3]))
    assert (al[1].score2, al[1].ref_end2) == sm.second(read[3:], ref, (1, 5, 7, 2), sm.mask_len_of(read[3:]))[2:]
    # the default: score2 is None and nothing new is launched
    ctx.reset_timing()
    a = ssw.Aligner(ref, 1, 5, 7, 2, ctx=ctx).align(read)
    assert a.score2 is None and a.ref_end2 is None and "SUB-OPTIMAL" not in str(a)
    assert ctx.get_timing(_lib.KERNEL_SECOND)[0] == 0 and ctx.get_timing(_lib.KERNEL_SW)[0] == 1
    # a filtered query gets None and costs no work
    assert ssw.Aligner(ref, 1, 5, 7, 2, report_secondary=True, ctx=ctx).align("ACGT", min_score=30) is None
    assert ctx.get_timing(_lib.KERNEL_SECOND)[0] == 0


@pytest.mark.parametrize("scoring", [(2, 2, 3, 1), (8, 0, 1, 1)], ids=lambda s: "/".join(map(str, s)))
def test_aligner_report_secondary_at_other_scorings(ctx, scoring):
    g = sm.golden()
    ks = _aligner_items(g, scoring, True)[:20]
    assert len(ks) >= 15
    for k in ks:
        a = ssw.Aligner(g["refs"][k], *scoring, report_secondary=True, ctx=ctx).align(g["reads"][k])
        assert (a.score, a.ref_end, a.score2, a.ref_end2) == tuple(int(v) for v in g["expect"][k]), k


def test_aligner_report_secondary_on_the_long_path(lctx):
    """With a long-reads context the switch serves queries of up to 2 048 bp and references of up to 4 095 letters."""
    g = sm.golden()
    ks = _aligner_items(g, (1, 5, 7, 2), False)
    assert {481, 2047, 2048} <= {len(g["reads"][k]) for k in ks} and max(len(g["refs"][k]) for k in ks) == 4095
    for k in ks:
        a = ssw.Aligner(g["refs"][k], 1, 5, 7, 2, report_secondary=True, ctx=lctx).align(g["reads"][k])
        assert (a.score, a.ref_end, a.score2, a.ref_end2) == tuple(int(v) for v in g["expect"][k]), k
