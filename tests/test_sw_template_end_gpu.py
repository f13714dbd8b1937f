"""The template-end code of sw_cont_kernel (csrc/sw_ladder.hip: combine by batched continuation reads + LDS max atomics,
resolve_best, the row reductions of the arg-max, the drop test, steady_exit) on hand-built reads, through the public
classify entry point, at every instantiation (R = 4, 7, 10, 16, 20, 32 rows per lane) and two scorings.

Three small ladders (prefix and suffix shorter than 30 bases, so that the default scoring runs the production kernel and
2/3/5/2 -- outside the 6-mer filter's premise -- the generic one with its sweep of the branch alone):
  P3  period 3, 8 units, 18-base suffix that begins with a copy of the unit   (the loop unrolled by the period)
  P4  period 4, 7 units, 18-base suffix that begins with half a unit          (the generic loop)
  P0  period 3, 6 units, no suffix            (forward strand: blen == 0, the branch without combine; reverse: alen == 0)
and per ladder a few dozen reads:
  inside     pure repeat, or the prefix's tail + repeat: the best cell lies on the trunk, the parked note must be resolved
  spanning   prefix tail + u units + suffix head for every u, alone and inside unrelated flanks up to the read length:
             the continuation candidate wins; for small u every later template end is dropped
  tie        k < u units and nothing else against a suffix that begins like the repeat: the alignment that ends on the
             trunk and the one that leaves through the suffix's first bases score the same -- the smaller end column
             (and then the start coordinates) decide, so the note has to be resolved although the scores are equal
  N          the same reads with N in the repeat, in the suffix and at the junction
Each case checks (1) the production launch against oracle/pyoracle.classify, (2) every record of the kernel's own
per-template dump against the oracle's ssw_align restatement (score and all four coordinates: this is where a wrong
tie rule or a stale note shows), (3) the production launch against the arg-max of that dump."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tredparse_amd import _lib

pytestmark = pytest.mark.gpu

LADDERS = [
    ("TGACCTGAAGTCCATGGACTTACGT", "CAG", "CAGTTCGATACCGGATTC", 8),
    ("ACGTTGCAATCGGATCCTAAGTCGA", "CCTG", "CCATGGACTAGTCATTCG", 7),
    ("GGATCTTACGACCTGATTCAAGCTA", "GAA", "", 6),
]
READLENS = (36, 100, 150, 250, 300, 470)      # -> R = 4, 7, 10, 16, 20, 32
SCORINGS = ((1, 5, 7, 2), (2, 3, 5, 2))


def _junk(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _with_n(s, at):
    s = list(s)
    for i in at:
        if 0 <= i < len(s):
            s[i] = "N"
    return "".join(s)


def _reads_for(rng, ladder, L):
    """Hand-built reads of one ladder, none longer than L, the first of exactly L bases."""
    a, rep, b, mu = ladder
    P = len(rep)
    out = []
    # inside the repeat: pure repeat at every phase, long and short; prefix tail + more units than any template has
    out.append((rep * (L // P + 2))[:L])
    for ph in range(P):
        out.append((rep * 40)[ph:ph + min(L, 36 + ph)])
    out.append((a[-12:] + rep * (mu + 4))[:L])
    out.append((a[-20:] + rep * (mu + 10))[:L])
    # spanning: every unit count, bare and inside flanks; small u leaves many later template ends to drop
    for u in range(1, mu + 1):
        core = a[-15:] + rep * u + b[:12]
        out.append(core[:L])
        pad = max(0, min(L, 30 + 20 * u) - len(core))
        out.append((_junk(rng, pad // 2) + core + _junk(rng, pad - pad // 2))[:L])
    full = a + rep * 3 + b
    out.append((_junk(rng, max(0, (L - len(full)) // 2)) + full + _junk(rng, L))[:L])
    out.append(po.rc((a + rep * 5 + b)[:L]))                       # the reverse strand's best
    # ties between the trunk's best and the continuation: k units, with and without an anchor in the prefix
    for k in range(2, mu):
        out.append((rep * k)[:L])
        out.append((a[-6:] + rep * k)[:L])
        out.append((rep * k + b[:P])[:L])
    # N: in the repeat, at the junction, in the suffix, and a run of them
    core = a[-15:] + rep * 4 + b
    j = 15 + 4 * P
    for at in ((16,), (j - 1, j), (j + 2, j + 7), (15 + P, 15 + P + 1, 15 + P + 2), tuple(range(10, 18))):
        out.append(_with_n(core, at)[:L])
    out.append(_with_n((rep * 14)[:min(L, 40)], (5, 20)))
    out.append("N" * min(L, 30))
    return [r for r in out if len(r) >= 1]


def _build(L, seed):
    rng = np.random.default_rng(seed)
    reads, uro, ul = [], [0], []
    for li, lad in enumerate(LADDERS):
        rr = _reads_for(rng, lad, L)
        # two units per ladder, the second with a number of reads that is no multiple of four
        cut = (len(rr) // 2) | 1
        for part in (rr[:cut], rr[cut:]):
            reads += part
            uro.append(len(reads))
            ul.append(li)
    return reads, np.asarray(uro, np.int32), np.asarray(ul, np.int32)


def _classify(ctx, reads, uro, ul, params, dump_templates=0):
    packed, woff, rlen = _lib.pack_reads(reads)
    n = len(reads)
    tag = np.zeros(n, np.uint8); h = np.zeros(n, np.int16); sc = np.zeros(n, np.int16)
    dump = np.zeros((n, dump_templates, 6), np.int16) if dump_templates else None
    ctx.sw_classify(_lib.MEM_HOST, packed, woff, rlen, n, uro, ul, len(ul), params, tag, h, sc, dump, dump_templates)
    return tag, h, sc, dump


def _argmax_of_dump(dump, nt_of_read):
    n, nt = dump.shape[:2]
    k = np.arange(nt)
    units, strand = k // 2 + 1, k % 2
    score, dtag = dump[:, :, 0].astype(np.int64), dump[:, :, 5].astype(np.int64)
    live = (dtag != _lib.TAG_NONE) & (k[None, :] < nt_of_read[:, None])
    key = np.where(live, (score << 11) | ((511 - units)[None, :] << 1) | (1 - strand)[None, :], -1)
    at = key.argmax(1)
    rows = np.arange(n)
    none = key[rows, at] < 0
    return (np.where(none, _lib.TAG_NONE, dtag[rows, at]), np.where(none, 0, units[at]), np.where(none, 0, score[rows, at]))


_ORACLE = {}


def _oracle(L, scoring):
    """(reads, unit offsets, unit ladders, read -> ladder, classify result, per-pair ssw result): computed once per case."""
    key = (L, scoring)
    if key not in _ORACLE:
        reads, uro, ul = _build(L, 7000 + L)
        read_locus = np.repeat(ul, np.diff(uro))
        ls = po.LocusSet(LADDERS)
        cls = po.classify(reads, read_locus, ls, scoring=scoring, threads=4)
        pr, pt = [], []
        for r, g in enumerate(read_locus):
            for t in range(ls.lad_off[g], ls.lad_off[g + 1]):
                pr.append(r)
                pt.append(t)
        pairs = po.sw_pairs(reads, ls.templates, pr, pt, scoring=scoring, threads=4)
        _ORACLE[key] = (reads, uro, ul, read_locus, ls, cls, np.asarray(pr), np.asarray(pt), pairs)
    return _ORACLE[key]


@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("L", READLENS)
def test_template_ends_against_oracle_and_dump(ctx, L, scoring):
    reads, uro, ul, read_locus, ls, cls, pr, pt, pairs = _oracle(L, scoring)
    assert max(len(r) for r in reads) == L
    ctx.set_ladders(LADDERS)
    params = _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], 9, 0, L, 0)
    ctx.reset_timing()
    tag, h, sc, _ = _classify(ctx, reads, uro, ul, params)
    cnt = ctx.get_sw_counters()
    nt = 2 * max(l[3] for l in LADDERS)
    t2, h2, s2, dump = _classify(ctx, reads, uro, ul, params, nt)
    # (1) the production launch against the oracle
    bad = np.nonzero((tag != cls[:, 0]) | (h != cls[:, 1]) | (sc != cls[:, 2]))[0]
    assert len(bad) == 0, (L, scoring, bad[:5], [reads[i] for i in bad[:3]], tag[bad[:5]], h[bad[:5]], sc[bad[:5]], cls[bad[:5]])
    assert np.array_equal(tag, t2) and np.array_equal(h, h2) and np.array_equal(sc, s2)
    # (2) every dump record: score, ref_begin, ref_end, read_begin, read_end of every (read, template)
    col = pt - np.asarray(ls.lad_off)[read_locus[pr]]
    got = dump[pr, col, :5].astype(np.int32)
    badp = np.nonzero((got != pairs).any(axis=1))[0]
    assert len(badp) == 0, (L, scoring, len(badp), [(reads[pr[i]], int(col[i]), got[i], pairs[i]) for i in badp[:3]])
    # (3) the production launch is the arg-max of the dump
    nt_of_read = 2 * np.asarray([l[3] for l in LADDERS])[read_locus]
    wt, wh, ws = _argmax_of_dump(dump, nt_of_read)
    assert np.array_equal(tag, wt) and np.array_equal(h, wh) and np.array_equal(sc, ws)
    # the cases are there: alignments that end on the trunk and in the suffix, tags of more than one kind, and the
    # production launch both combined and dropped template ends and emitted some from the trunk alone (P0 forward)
    p3 = read_locus[pr] == 0
    fwd = col % 2 == 0
    alen, units = len(LADDERS[0][0]), col // 2 + 1
    hit = pairs[:, 0] > 0
    assert (p3 & fwd & hit & (pairs[:, 2] >= alen + 3 * units)).any() and (p3 & fwd & hit & (pairs[:, 2] < alen + 3 * units)).any()
    assert len(set(tag.tolist())) >= 3
    assert cnt["templates_combined"] > 0 and cnt["emitted_from_trunk"] > 0
    if scoring == SCORINGS[0]:
        assert cnt["templates_dropped"] > 0


def test_ties_between_trunk_and_continuation_exist():
    """The tie reads are ties: k units against the template of u > k units score the same on the trunk alone
    (prefix + repeat * u) and on the whole template, whose suffix begins with one more copy of the unit -- an alignment
    one unit further right, ending inside the suffix, has the same score, and the reported end stays on the trunk."""
    a, rep, b, mu = LADDERS[0]
    assert b.startswith(rep)
    reads = [rep * k for k in range(2, mu)]
    refs = [a + rep * mu, a + rep * mu + b, rep * (mu - 1) + b]
    n = len(reads)
    trunk = po.sw_pairs(reads, refs, list(range(n)), [0] * n)
    whole = po.sw_pairs(reads, refs, list(range(n)), [1] * n)
    shifted = po.sw_pairs(reads, refs, list(range(n)), [2] * n)
    assert np.array_equal(trunk[:, 0], whole[:, 0]) and np.array_equal(trunk[:, 0], shifted[:, 0])
    assert np.array_equal(trunk, whole) and (whole[:, 2] < len(a) + 3 * mu).all()


@pytest.mark.parametrize("q", (1, 2, 3, 4))
def test_quads_of_one_to_four_reads(ctx, q):
    """One wavefront with q of its four read slots filled (identical reads share a bin): the empty slots' lanes take
    part in every wave-wide test of the template end and must not change the others' results."""
    a, rep, b, mu = LADDERS[0]
    for read in (a[-15:] + rep * 3 + b[:12], rep * 5, _with_n(a[-15:] + rep * 6 + b, (20, 36))):
        reads = [read] * q
        uro, ul = np.asarray([0, q], np.int32), np.zeros(1, np.int32)
        ctx.set_ladders(LADDERS)
        for scoring in SCORINGS:
            params = _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], 9, 0, 150, 0)
            tag, h, sc, _ = _classify(ctx, reads, uro, ul, params)
            t2, h2, s2, dump = _classify(ctx, reads, uro, ul, params, 2 * mu)
            cls = po.classify(reads, np.zeros(q, np.int32), po.LocusSet(LADDERS), scoring=scoring)
            assert np.array_equal(tag, cls[:, 0]) and np.array_equal(h, cls[:, 1]) and np.array_equal(sc, cls[:, 2])
            assert np.array_equal(tag, t2) and np.array_equal(h, h2) and np.array_equal(sc, s2)
            want = po.sw_pairs([read], po.LocusSet(LADDERS).templates[:2 * mu], [0] * (2 * mu), list(range(2 * mu)), scoring=scoring)
            for r in range(q):
                assert np.array_equal(dump[r, :, :5].astype(np.int32), want), (q, r, read)
