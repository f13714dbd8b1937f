"""GPU: the long-read SW kernel (csrc/sw_long.hip through Context.set_long_reads) at the edges of its three row classes
(R = 8 / 16 / 32 rows per lane for reads up to 512 / 1 024 / 2 048 bp), at other scorings up to the corners of the accepted
range, with short and empty reads on long ladders, on long plain references, with more reads than wavefronts, and at
dump shapes that do not match the ladder.  Every expected value is the restated ssw_align / _parseReadSW's
(oracle/sw_oracle.c; tests/test_oracle_sw.py pins it to the compiled reference at these scorings on long pairs).

The crafted cases that tell the tie rules and the per-read state apart.  Each was checked on the CPU: the oracle with
that one rule turned the other way, or a model of a wavefront that keeps its arg-max, gives other expected values there
(rows = dump rows of the 880 of a call that change):
  end cell, first column            test_class_edges[513-scoring0]: 400 rows, nine of the eleven reads
  end cell, then smallest row       test_class_edges[513-scoring0]: 240 rows: the pure-repeat reads and the two-letter read
  begin cell, largest start column  test_class_edges[513-scoring1] (1/1/2/1): 123 rows: the two-letter read, the read with N,
                                    the spanning reads; test_range_corners[513-scoring2] (8/0/1/1): 40 rows, the two-letter read
  begin cell, then largest row      test_range_corners[513-scoring2]: 46 rows: the two-letter read and the last-base read
                                    (at 1/5/7/2 no read of these sets ties there: gaps are too dear)
  bestS / bestU / bestTag per read  test_more_reads_than_wavefronts: 25 of the 52 reads that a wavefront takes second would
                                    report the first one's score or tag
"""
import numpy as np
import pytest

from oracle import pyoracle as po
from tredparse_amd import _lib, synth

from .test_long_reads_gpu import _rand, _reads

pytestmark = pytest.mark.gpu

DEFAULT = (1, 5, 7, 2)
FLANK = 9


@pytest.fixture(scope="module")
def lctx(ctx):
    """A context of its own with the long path on (`ctx` first: torch's HIP runtime is loaded before the library's)."""
    c = _lib.Context(0)
    c.set_long_reads(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loci():
    return {l["name"]: l for l in synth.load_loci() if l["name"] in ("HD", "ULD")}


def _ladder(locus, mu):
    return (locus["prefix"], locus["repeat"], locus["suffix"], mu)


def _run(ctx, ladders, reads, uro, ul, scoring=DEFAULT, nt=0, clip=False, guard=0):
    """sw_classify of `reads` in units (uro, ul): (tag, h, score, dump[n + guard, nt, 6]); the guard rows behind the dump
    are filled with 0x5A5A."""
    ctx.set_ladders(ladders)
    packed, woff, rlen = _lib.pack_reads(reads)
    n = len(reads)
    tag = np.zeros(n, np.uint8); h = np.zeros(n, np.int16); sc = np.zeros(n, np.int16)
    d = np.full((n + guard, nt, 6), 0x5A5A, np.int16) if nt else None
    ctx.sw_classify(_lib.MEM_HOST, packed, woff, rlen, n, np.asarray(uro, np.int32), np.asarray(ul, np.int32), len(ul),
                    _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], FLANK, int(clip), 0, 0), tag, h, sc, d, nt)
    return tag, h, sc, d


def _read_ladder(uro, ul):
    return np.repeat(np.asarray(ul, np.int32), np.diff(np.asarray(uro)))


def _check_tags(out, ladders, reads, rl, scoring, clip=False):
    cls = po.classify(reads, rl, po.LocusSet(ladders), clip=clip, scoring=scoring, threads=16)
    got = np.stack([out[0], out[1], out[2]], axis=1).astype(np.int32)
    bad = np.nonzero((got != cls).any(axis=1))[0]
    assert len(bad) == 0, "read {} ({} bp): gpu {} oracle {}".format(bad[0], len(reads[bad[0]]), got[bad[0]], cls[bad[0]])
    return cls


def _check_dump(dump, ladders, reads, rl, scoring, picks=None, rows=None):
    """dump[r, k, :5] against ssw_align for the templates k (picks, default: every one of the read's ladder that the dump
    has a row for); returns the oracle's fields."""
    ls = po.LocusSet(ladders)
    rows = dump.shape[1] if rows is None else rows
    pr, pt, pk = [], [], []
    for r in range(len(reads)):
        nt = ls.lad_off[rl[r] + 1] - ls.lad_off[rl[r]]
        for k in (picks if picks is not None else range(min(nt, rows))):
            pr.append(r); pt.append(ls.lad_off[rl[r]] + k); pk.append(k)
    want = po.sw_pairs(reads, ls.templates, pr, pt, scoring=scoring, threads=16)
    got = dump[pr, pk, :5].astype(np.int32)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "read {} ({} bp) template {}: gpu {} oracle {}".format(
        pr[bad[0]], len(reads[pr[bad[0]]]), pk[bad[0]], got[bad[0]], want[bad[0]])
    return want


def _edge_reads(rng, locus, L):
    """_reads' set (spanning, prefix, suffix, inside, reverse strand, with N, all N) and the reads that make ties or sit
    on the last row: a read whose last base is the only one on the suffix (row L - 1 must win), a pure repeat, and a read
    of two letters of the repeat."""
    pre, rep, suf = locus["prefix"], locus["repeat"], locus["suffix"]
    out = _reads(rng, locus, 30, L)
    body = pre + rep * 20 + suf[:1]
    out.append((_rand(rng, L) + body)[-L:])
    out.append((rep * (L // len(rep) + 2))[1:L + 1])
    out.append("".join(rep[i] for i in rng.integers(0, 2, L)))
    out.append(po.rc(out[-2]))
    assert all(len(r) == L for r in out)
    return out


def _edges(lctx, locus, L, scoring):
    rng = np.random.default_rng(L * 131 + scoring[0] + scoring[1])
    lad = _ladder(locus, 40)
    reads = _edge_reads(rng, locus, L)
    n = len(reads)
    out = _run(lctx, [lad], reads, [0, n], [0], scoring=scoring, nt=80)
    rl = np.zeros(n, np.int32)
    want = _check_dump(out[3], [lad], reads, rl, scoring).reshape(n, 80, 5)
    cls = _check_tags(out, [lad], reads, rl, scoring)
    # the cases are what they claim to be: the last-base read ends on row L - 1 on the template it was cut from
    # (20 units, forward strand; with mismatch 0 an alignment runs on for free and may end anywhere), and some read is tagged
    assert want[7, 2 * 19, 0] > 0 and (want[7, 2 * 19, 4] == L - 1 or scoring[1] == 0)
    assert (cls[:, 0] != 0).any()


@pytest.mark.parametrize("scoring", [DEFAULT, (1, 1, 2, 1)])
@pytest.mark.parametrize("L", [480, 481, 511, 512, 513, 1023, 1024, 1025, 2047, 2048])
def test_class_edges(lctx, loci, L, scoring):
    """Each side of the 512 / 1 024 thresholds and the ends of the range (480: the short kernel on the same ladder, for
    contrast): all 80 templates' fields and the tags."""
    _edges(lctx, loci["HD"], L, scoring)


@pytest.mark.parametrize("scoring", [(8, 16, 16, 16), (1, 16, 16, 1), (8, 0, 1, 1)])
@pytest.mark.parametrize("L", [513, 1025])
def test_range_corners(lctx, loci, L, scoring):
    """The corners of the accepted scoring range (mismatch 16 scores what a padding row scores; gap_open == gap_extend;
    mismatch 0) where one real row sits beside 15 / 31 padding rows of its lane.  Every read of these calls takes the long
    path, so the library's own packed-value bound on the scoring (which refuses gap_extend 16) does not apply."""
    _edges(lctx, loci["HD"], L, scoring)


@pytest.mark.parametrize("bad", [(9, 5, 7, 2), (1, 17, 7, 2), (1, 5, 2, 3), (1, 5, 17, 2), (0, 5, 7, 2)])
def test_scoring_out_of_range_is_refused_through_the_long_route(lctx, loci, bad):
    rng = np.random.default_rng(17)
    with pytest.raises(_lib.TredGpuError, match=r"tredlong_sw_classify failed \(-2\): scoring out of the supported range "
                                                r"\(match 1\.\.8, mismatch 0\.\.16, 1 <= gap_extend <= gap_open <= 16"):
        _run(lctx, [_ladder(loci["HD"], 40)], [_rand(rng, 513)], [0, 1], [0], scoring=bad)


def test_three_classes_and_the_short_kernel_in_one_call(lctx, loci):
    """150 / 500 / 600 / 1 100 / 2 000 bp reads interleaved in one unit, and across three units of two ladders: what each
    class computes alone, and what the oracle says."""
    rng = np.random.default_rng(1505006)
    lads = [_ladder(loci["HD"], 40), _ladder(loci["ULD"], 30)]
    lens = (150, 500, 600, 1100, 2000)
    sets = {(k, L): _edge_reads(rng, loci[name], L)[:4] + _edge_reads(rng, loci[name], L)[7:9]
            for k, name in enumerate(("HD", "ULD")) for L in lens}
    # one unit: HD's reads, lengths interleaved
    one = [sets[0, L][j] for j in range(6) for L in lens]
    # three units (HD, ULD, HD)
    units = [[sets[0, L][j] for j in range(3) for L in lens], [sets[1, L][j] for j in range(6) for L in lens[::-1]],
             [sets[0, L][j] for j in range(3, 6) for L in lens]]
    for reads, uro, ul in ((one, [0, len(one)], [0]),
                           ([r for u in units for r in u], np.concatenate([[0], np.cumsum([len(u) for u in units])]), [0, 1, 0])):
        rl = _read_ladder(uro, ul)
        out = _run(lctx, lads, reads, uro, ul, nt=80)
        _check_tags(out, lads, reads, rl, DEFAULT)
        _check_dump(out[3], lads, reads, rl, DEFAULT)
        # (the long kernel's reads: the rows past their ladder's templates stay -1)
        assert all((out[3][r, 2 * lads[rl[r]][3]:] == -1).all() for r in range(len(reads)) if len(reads[r]) > 480)
        # one class at a time (one unit per read, so that any subset is a call)
        L = np.array([len(r) for r in reads])
        for sel in (L == 150, L == 500, L == 600, L > 1024):
            idx = np.nonzero(sel)[0]
            alone = _run(lctx, lads, [reads[i] for i in idx], np.arange(len(idx) + 1), rl[idx], nt=80)
            for a, b in zip(alone, out):
                assert np.array_equal(a, b[idx])


def _plain_expect(al, T, L):
    """_parseReadSW's rule (bam_parser.py:123-182) for the one template of a plain reference (units 0, max_units 0)."""
    score, rb, re_, qb, qe = (int(x) for x in al)
    min_len = min(L, T) // 2
    if score < max(min_len, 30) or qe - qb + 1 < min_len:
        return 0, 0, 0
    aL, aR, bL, bR = rb, T - re_ - 1, qb, L - qe - 1
    if min(aR + bL, aL + bR, aL + aR, bL + bR) >= FLANK:
        tag = 5
    elif rb < FLANK:
        tag = 1 if re_ > T - FLANK - 1 else 2
    else:
        tag = 3 if re_ > T - FLANK - 1 else 4
    return tag, 0, score


def _check_plain(out, refs, reads, rl, scoring):
    want = po.sw_pairs(reads, refs, list(range(len(reads))), list(rl), scoring=scoring, threads=16)
    got = out[3][:len(reads), 0, :5].astype(np.int32)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "read {} ({} bp): gpu {} oracle {}".format(bad[0], len(reads[bad[0]]), got[bad[0]], want[bad[0]])
    exp = np.array([_plain_expect(want[r], len(refs[rl[r]]), len(reads[r])) for r in range(len(reads))], np.int32)
    got = np.stack(out[:3], axis=1).astype(np.int32)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, "read {}: gpu (tag, h, score) {} expected {}".format(bad[0], got[bad[0]], exp[bad[0]])
    return want, exp


def test_more_reads_than_wavefronts(lctx):
    """2 100 reads of one class: the launch has 2 048 wavefronts, so 52 of them take a second read and must start it from
    fresh state (rows, H / E, the best cell, and the arg-max bestS / bestU / bestTag).  The reads at list positions k and
    k + 2 048 are copies of different originals; of the 52 pairs most differ in score, many have the lower score or no tag
    at all in the second read -- which a stale arg-max would not report."""
    rng = np.random.default_rng(2100)
    ref = _rand(rng, 60)
    base = []
    for j in range(50):
        L = 481 + j % 20
        core = list(ref[:60 - (j % 5) * 6] if j % 3 else ref[(j % 4) * 5:])
        for k in rng.choice(len(core), j % 7, replace=False):
            core[k] = "N" if j % 2 else "ACGT"[("ACGT".index(core[k]) + 1) % 4]
        core = "".join(core) if j % 10 != 9 else ""
        a = int(rng.integers(0, L - len(core)))
        base.append(_rand(rng, a) + core + _rand(rng, L - a - len(core)))
    reads = []
    for k in range(2100):
        r = list(base[k % 50])
        r[int(rng.integers(0, 5))] = "ACGT"[int(rng.integers(4))]        # a copy, not the original (outside the core mostly)
        reads.append("".join(r))
    assert all(481 <= len(r) <= 500 for r in reads)
    lad = (ref, "A", "", 0)
    out = _run(lctx, [lad], reads, [0, 2100], [0], nt=1)
    want, exp = _check_plain(out, [ref], reads, np.zeros(2100, np.int32), DEFAULT)
    first, second = exp[:52], exp[2048:]
    assert (first[:, 2] != second[:, 2]).sum() >= 26 and (second[:, 2] < first[:, 2]).sum() >= 10
    assert ((second[:, 0] == 0) & (first[:, 0] != 0)).any() and ((second[:, 0] != 0) & (first[:, 0] != second[:, 0])).any()


@pytest.mark.parametrize("scoring", [DEFAULT, (1, 0, 1, 1)])
@pytest.mark.parametrize("mu", [200, 1353])
def test_short_reads_on_a_long_ladder(lctx, loci, mu, scoring):
    """Reads of 0 ... 480 bp on a ladder of 636 / 4 095 columns go to sw_long_kernel<8> with most lanes all padding (the
    binding hides routed reads from the library as length 0, and hands the long kernel a real length-0 read)."""
    rng = np.random.default_rng(mu)
    hd = loci["HD"]
    pre, rep, suf = hd["prefix"], hd["repeat"], hd["suffix"]
    lad = _ladder(hd, mu)
    assert len(pre) + len(suf) + 3 * mu == (636 if mu == 200 else 4095)
    span = pre[-10:] + rep * 40 + suf
    reads = ["", "N", "CA", (rep * 12)[:35], (rep * 4 + suf + "ACGTAC")[:36], po.rc((pre + rep * 20)[-64:]),
             (_rand(rng, 40) + span + _rand(rng, 40))[:150], rep * 160, "", po.rc(rep * 160), "N" * 64, _rand(rng, 480),
             (pre + rep * 150 + suf)[:480]]
    assert sorted(set(len(r) for r in reads)) == [0, 1, 2, 35, 36, 64, 150, 480]
    n = len(reads)
    out = _run(lctx, [lad], reads, [0, n], [0], scoring=scoring, nt=2 * mu)
    rl = np.zeros(n, np.int32)
    if mu == 200:
        _check_dump(out[3], [lad], reads, rl, scoring)
        _check_tags(out, [lad], reads, rl, scoring)
    else:
        picks = sorted(set(range(8)) | set(range(2 * mu - 8, 2 * mu)) | set(rng.choice(2 * mu, 30, replace=False).tolist()))
        _check_dump(out[3], [lad], reads, rl, scoring, picks=picks)
    empty = [i for i, r in enumerate(reads) if not r]
    assert (out[0][empty] == 0).all() and (out[3][empty, :, :5] == [0, -1, -1, 0, 0]).all()
    assert (out[3][:, :, 0] > 0).any()


@pytest.mark.parametrize("scoring", [DEFAULT, (1, 0, 1, 1), (8, 16, 16, 16)])
def test_long_plain_references(lctx, scoring):
    """max_units = 0 (one template, next_end = alen - 1, period 1) at 512, 1 000 and 4 095 letters, reads of all three
    classes and of the short kernel's length."""
    rng = np.random.default_rng(5124095)
    refs = [_rand(rng, n) for n in (512, 1000, 4095)]
    reads, uro, ul = [], [0], []
    for i, ref in enumerate(refs):
        for L in (150, 600, 2048):
            for _ in range(2):
                a = int(rng.integers(0, max(1, len(ref) - 30)))
                frag = ref[a:a + L - 8]
                frag = frag[:len(frag) // 2] + "ACGTNACG" + frag[len(frag) // 2:]
                frag = frag + _rand(rng, L - len(frag))
                reads.append(frag)
        uro.append(len(reads))
        ul.append(i)
    out = _run(lctx, [(r, "A", "", 0) for r in refs], reads, uro, ul, scoring=scoring, nt=1)
    want, exp = _check_plain(out, refs, reads, _read_ladder(uro, ul), scoring)
    assert (exp[:, 0] != 0).any() and (want[:, 0] > 100).sum() >= 9


def test_score_16384_fits_its_int16(lctx):
    """match 8 over 2 048 rows: the largest score the path can produce.  Every column from 2 047 on reaches it; the first
    one wins."""
    ref, read = "A" * 4095, "A" * 2048
    out = _run(lctx, [(ref, "A", "", 0)], [read], [0, 1], [0], scoring=(8, 16, 16, 16), nt=1)
    want, exp = _check_plain(out, [ref], [read], np.zeros(1, np.int32), (8, 16, 16, 16))
    assert list(want[0]) == [16384, 0, 2047, 0, 2047] and out[2][0] == 16384


def test_dump_shapes(lctx, loci):
    """Two ladders of 20 and 60 templates in one call.  dump_templates 60: the first ladder's rows 20 ... 59 stay -1.
    dump_templates 7 (odd, fewer than either ladder has): rows 0 ... 6 are right, and nothing is written behind the
    array (guard rows) or -- which would show in the next read's rows -- behind a read's seven."""
    rng = np.random.default_rng(760)
    lads = [_ladder(loci["HD"], 10), _ladder(loci["ULD"], 30)]
    per = [[r for L in (513, 600, 1100) for r in _reads(rng, loci[name], 8, L)[:3]] for name in ("HD", "ULD")]
    reads = per[0] + per[1]
    uro, ul = [0, len(per[0]), len(reads)], [0, 1]
    rl = _read_ladder(uro, ul)
    n = len(reads)
    wide = _run(lctx, lads, reads, uro, ul, nt=60, guard=2)
    _check_dump(wide[3][:n], lads, reads, rl, DEFAULT)
    assert (wide[3][:len(per[0]), 20:] == -1).all() and (wide[3][len(per[0]):n, :, 0] >= 0).all()
    assert (wide[3][n:] == 0x5A5A).all()
    narrow = _run(lctx, lads, reads, uro, ul, nt=7, guard=2)
    _check_dump(narrow[3][:n], lads, reads, rl, DEFAULT, rows=7)
    assert np.array_equal(narrow[3][:n], wide[3][:n, :7]) and (narrow[3][n:] == 0x5A5A).all()
    for a, b in zip(narrow[:3], wide[:3]):
        assert np.array_equal(a, b)
    _check_tags(wide, lads, reads, rl, DEFAULT)
