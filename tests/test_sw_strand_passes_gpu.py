"""The two strand passes of the SW kernel (csrc/sw_ladder.hip: pass A sweeps strand 0, repack_kernel hands the reads that
are still open to pass B, which sweeps strand 1; csrc/capi.hip run_sw_device), through tredgpu_sw_classify and
tredgpu_genotype_batch on device memory.

Every case compares the tag, h and score of every read with oracle/pyoracle.classify and with the arg-max of the
kernel's own per-template dump, which still runs as one launch over both strands.  A CPU model of the re-pack -- the 6-mer
counts restated in Python, the per-template tags restated from the oracle's alignments, the kernel's entry test for
strand 1 -- says which reads must reach pass B; the library's counter of the reads handed to pass B (counter 7 of
tredgpu_get_sw_counters) has to agree, and the model is what shows that the cases named below are really there.

  shared 6-mers   ULD (data/treds.json: its motif shares 6-mers with its reverse complement) and a palindromic ladder
                  (prefix = rc(suffix), motif = rc(motif): the two strands' templates are the same strings): forward reads
                  that strand 0 settles, reads that stay open and whose strand-1 candidate wins / loses, reverse-strand
                  reads of class 2, equal (score, units) on both strands
  bins and quads  bins of 1, 4 and 5 reads in each pass, an empty pass B, a pass B with every read, a unit without reads
  other paths     a plain reference (max_units == 0, the only ladders with one strand) next to a two-strand ladder,
                  clip = 1, a scoring outside the 6-mer filter's premise (every read is of class 3, no cap from the counts)
  read lengths    64, 150 and 160 (the edges of the 4- and 10-row instantiations), one read beyond the rows in each
  reproducibility two batches on one context against fresh contexts (the arg-max workspace is set again by every call)
"""
import numpy as np
import pytest

from oracle import lik_oracle as lo
from oracle import pyoracle as po
from tredparse_amd import _lib

pytestmark = pytest.mark.gpu

ULD = ("GCCCCGCAAGAAGGGACG", "CGCGGGGCGGGG", "AACCTGGCCACCACTCGC")
PAL_PREFIX = "TGACCTGAAGTCCATGGA"
PAL = (PAL_PREFIX, "GAATTC", po.rc(PAL_PREFIX))
HD = ("GAGTCCCTCAAGTCCTTC", "CAG", "CAACAGCCGCCACCGCCG")
PLAIN = ("ACGTTGCAATCGGATCCTAAGTCGAGGATCTTACGACCTGATTCAAGCTATTGCCAGT", "A", "", 0)
DEFAULT = (1, 5, 7, 2)
LOOSE = (2, 3, 5, 2)          # mismatch < 5 * match: outside the 6-mer filter's premise
FLANK = 9


def _lad(l, L):
    return (l[0], l[1], l[2], -(-L // len(l[1])))


def _junk(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _mutate(rng, s, k):
    s = list(s)
    for i in rng.choice(len(s), k, replace=False):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def _rows(max_len):
    for cap, r in ((64, 4), (112, 7), (160, 10), (256, 16), (320, 20)):
        if max_len <= cap:
            return r
    return 32


class Case:
    def __init__(self, ladders, units, scoring=DEFAULT, clip=0, max_len=150):
        """units: [(ladder index, [reads])]"""
        self.ladders, self.scoring, self.clip, self.max_len = list(ladders), scoring, clip, max_len
        self.reads = [r for _, rr in units for r in rr]
        self.uro = np.cumsum([0] + [len(rr) for _, rr in units]).astype(np.int32)
        self.ul = np.asarray([l for l, _ in units], np.int32)
        self.read_lad = np.repeat(self.ul, np.diff(self.uro))
        self._model = None

    # ---- the CPU model --------------------------------------------------------------------------------------
    def _template_tag(self, row, L, T, u, mu_rept, period):
        score, rb, re, qb, qe = (int(x) for x in row)
        min_len = min(L, T) >> 1
        if score < max(min_len, 30) or qe - qb + 1 < min_len:
            return _lib.TAG_NONE
        aL, aR, bL, bR = rb, T - re - 1, qb, L - qe - 1
        if min(aR + bL, aL + bR, aL + aR, bL + bR) >= FLANK:
            return _lib.TAG_HANG
        pre, suf = rb < FLANK, re > T - FLANK - 1
        if pre:
            return _lib.TAG_FULL if suf else _lib.TAG_PREF
        if suf:
            return _lib.TAG_POST
        return _lib.TAG_REPT if u >= mu_rept - 1 and u * period <= L else _lib.TAG_NONE

    def model(self):
        """want (n, 3), to_b (n) bool, cls (n) strand-class bits, win1 (n) bool: the strand-1 candidate replaces strand 0's."""
        if self._model is not None:
            return self._model
        m, x, go, ge = self.scoring
        thr = -(-30 // m) - 5 if min(x, go) >= 5 * m else 0
        with_kcap = thr > 0 and _rows(self.max_len) in (7, 10)
        n = len(self.reads)
        want = np.zeros((n, 3), np.int64)
        to_b, cls, win1, tie = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, bool), np.zeros(n, bool)
        two = [i for i in range(n) if self.ladders[self.read_lad[i]][3] > 0]
        ls = po.LocusSet([l if l[3] > 0 else ("A", "C", "G", 1) for l in self.ladders])
        if two:
            got = po.classify([self.reads[i] for i in two], self.read_lad[two], ls, clip=bool(self.clip), scoring=self.scoring, threads=4)
            want[two] = got
        pr, pt = [], []
        for i in two:
            g = self.read_lad[i]
            pr += [i] * (ls.lad_off[g + 1] - ls.lad_off[g])
            pt += list(range(ls.lad_off[g], ls.lad_off[g + 1]))
        pairs = po.sw_pairs(self.reads, ls.templates, pr, pt, scoring=self.scoring, threads=4) if two else np.zeros((0, 5))
        ksets = {}
        at = 0
        for i in two:
            g = int(self.read_lad[i])
            a, rep, b, mu = self.ladders[g]
            if g not in ksets:
                ksets[g] = [set(t[j:j + 6] for t in ls.templates[ls.lad_off[g] + s:ls.lad_off[g + 1]:2] for j in range(len(t) - 5))
                            for s in (0, 1)]
            read, L, P = self.reads[i], len(self.reads[i]), len(rep)
            cnt = [sum(1 for j in range(5, L) if "N" in read[j - 5:j + 1] or read[j - 5:j + 1] in ksets[g][s]) for s in (0, 1)]
            cls[i] = sum(1 << s for s in (0, 1) if thr == 0 or cnt[s] >= thr)
            mu_rept = -(-L // P) if self.clip else mu
            best = [None, None]      # per strand: (score, -u, tag) of the first maximal candidate
            for k in range(2 * mu):
                u, s = k // 2 + 1, k % 2
                T = len(a) + P * u + len(b)
                tag = self._template_tag(pairs[at + k], L, T, u, mu_rept, P)
                c = (int(pairs[at + k][0]), -u, tag)
                if tag != _lib.TAG_NONE and (best[s] is None or c[:2] > best[s][:2]):
                    best[s] = c
            at += 2 * mu
            if L > 16 * _rows(self.max_len):
                want[i] = (_lib.TAG_INVALID, 0, 0)
                continue
            # the restated arg-max is the oracle's (strand 0 first: strand 1 needs a larger (score, -units))
            merged = best[0] if best[1] is None or (best[0] is not None and best[1][:2] <= best[0][:2]) else best[1]
            assert tuple(want[i]) == ((merged[2], -merged[1], merged[0]) if merged else (0, 0, 0)), (i, read, want[i], best)
            cap = min((cnt[1] + 5) * m if with_kcap else 1 << 20, L * m)
            need = max(max(min(L, len(a) + P + len(b)) >> 1, 30), (best[0][0] if best[0] else -1) + 1)
            to_b[i] = bool(cls[i] & 2) and need <= cap
            win1[i] = to_b[i] and merged is not None and merged is best[1]
            tie[i] = best[0] is not None and best[1] is not None and best[0][:2] == best[1][:2]
        for i in range(n):
            if self.ladders[self.read_lad[i]][3] == 0 and len(self.reads[i]) > 16 * _rows(self.max_len):
                want[i] = (_lib.TAG_INVALID, 0, 0)
        self._model = dict(want=want, to_b=to_b, cls=cls, win1=win1, tie=tie, two=np.asarray(two, np.int64))
        return self._model


# ---- the GPU side -------------------------------------------------------------------------------------------------

def _device_inputs(case):
    import torch
    dev = torch.device("cuda", 0)
    packed, woff, rlen = _lib.pack_reads(case.reads)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dev, dict(packed=dv(packed.view(np.int32)), roff=dv(woff), rlen=dv(rlen), uoff=dv(case.uro), ulad=dv(case.ul))


def _params(case):
    s = case.scoring
    return _lib.SwParams(s[0], s[1], s[2], s[3], FLANK, case.clip, case.max_len, 0)


def _handed_to_pass_b(ctx):
    out = np.zeros(8, np.uint64)
    assert ctx.lib.tredgpu_get_sw_counters(ctx.h, out.ctypes.data) == 0
    return int(out[7])


def _classify(ctx, case, dump_templates=0):
    import torch
    dev, d = _device_inputs(case)
    n = len(case.reads)
    tag = torch.zeros(n, dtype=torch.uint8, device=dev); h = torch.zeros(n, dtype=torch.int16, device=dev)
    sc = torch.zeros(n, dtype=torch.int16, device=dev)
    dump = torch.zeros((n, dump_templates, 6), dtype=torch.int16, device=dev) if dump_templates else None
    torch.cuda.synchronize()
    ctx.sw_classify(_lib.MEM_DEVICE, d["packed"], d["roff"], d["rlen"], n, d["uoff"], d["ulad"], len(case.ul), _params(case),
                    tag, h, sc, dump, dump_templates)
    ctx.sync()
    return tag.cpu().numpy(), h.cpu().numpy(), sc.cpu().numpy(), dump.cpu().numpy() if dump_templates else None


def _genotype(ctx, case):
    import torch
    step, w = lo.load_model()
    ctx.set_model(np.array([step[k] for k in range(1, 7)]), np.array(w))
    dev, d = _device_inputs(case)
    n, g = len(case.reads), len(case.ul)
    hs = max(l[3] for l in case.ladders) + 2
    units = np.zeros(g, _lib.UNIT_DTYPE)
    for u in range(g):
        period = len(case.ladders[case.ul[u]][1]) if case.ladders[case.ul[u]][3] > 0 else 3
        units[u]["period"], units[u]["readlen"], units[u]["ploidy"], units[u]["maxinsert"] = period, 150, 2, 300
        units[u]["ref_len"], units[u]["minpe"], units[u]["cutoff_risk"] = 10 * period, 10 * period + 20, 40
        units[u]["is_expansion"], units[u]["half_depth"] = 1, 15.0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    tag, h, sc = z(n, torch.uint8), z(n, torch.int16), z(n, torch.int16)
    full, pref, rept = z((g, hs), torch.int32), z((g, hs), torch.int32), z((g, hs), torch.int32)
    calls = z(g * _lib.CALL_DTYPE.itemsize, torch.uint8)
    d_units = torch.from_numpy(units.view(np.uint8)).to(dev)
    lens = z(1, torch.int32)
    torch.cuda.synchronize()
    ctx.genotype_batch(_lib.MEM_DEVICE, d["packed"], d["roff"], d["rlen"], n, d["uoff"], d["ulad"], d_units, g, _params(case), None,
                       lens, 0, lens, 0, tag, h, sc, hs, full, pref, rept, calls)
    ctx.sync()
    return tag.cpu().numpy(), h.cpu().numpy(), sc.cpu().numpy(), full.cpu().numpy(), pref.cpu().numpy(), rept.cpu().numpy()


def _argmax_of_dump(case, dump):
    """(tag, h, score) per read from the per-template dump: largest (score, -units), strand 0 before strand 1."""
    n, nt = dump.shape[:2]
    out = np.zeros((n, 3), np.int64)
    for i in range(n):
        mu = case.ladders[case.read_lad[i]][3]
        if len(case.reads[i]) > 16 * _rows(case.max_len):
            out[i] = (_lib.TAG_INVALID, 0, 0)
            continue
        best = None
        for k in range(2 * mu if mu > 0 else 1):
            u, s = (k // 2 + 1, k % 2) if mu > 0 else (0, 0)
            score, tag = int(dump[i, k, 0]), int(dump[i, k, 5])
            if tag != _lib.TAG_NONE and (best is None or (score, -u, -s) > best[:3]):
                best = (score, -u, -s, tag)
        if best:
            out[i] = (best[3], -best[1], best[0])
    return out


def _check(ctx, case):
    """Runs the case through both entry points and the dump; returns the number of reads handed to pass B."""
    M = case.model()
    want = M["want"]
    ctx.set_ladders(case.ladders)
    ctx.reset_timing()
    tag, h, sc, _ = _classify(ctx, case)
    handed = _handed_to_pass_b(ctx)
    got = np.stack([tag, h, sc], 1).astype(np.int64)
    nt = max(1, 2 * max(l[3] for l in case.ladders))
    t2, h2, s2, dump = _classify(ctx, case, nt)
    by_dump = _argmax_of_dump(case, dump)
    two = M["two"]
    bad = two[np.nonzero((got[two] != want[two]).any(1))[0]]
    assert len(bad) == 0, ("oracle", bad[:5], [case.reads[i] for i in bad[:3]], got[bad[:5]], want[bad[:5]])
    bad = np.nonzero((got != by_dump).any(1))[0]
    assert len(bad) == 0, ("dump", bad[:5], [case.reads[i] for i in bad[:3]], got[bad[:5]], by_dump[bad[:5]])
    assert np.array_equal(got, np.stack([t2, h2, s2], 1))        # the dump call's own tags: one launch, both strands
    # a read beyond the instantiation's rows is flagged, once, and nothing else is
    too_long = np.asarray([len(r) > 16 * _rows(case.max_len) for r in case.reads])
    assert np.array_equal(tag == _lib.TAG_INVALID, too_long)
    assert handed == int(M["to_b"].sum()), (handed, int(M["to_b"].sum()))
    gt, gh, gs, full, pref, rept = _genotype(ctx, case)
    assert np.array_equal(np.stack([gt, gh, gs], 1), got)
    hs = full.shape[1]
    wf, wp, wr = np.zeros_like(full), np.zeros_like(pref), np.zeros_like(rept)
    for u in range(len(case.ul)):
        for i in range(case.uro[u], case.uro[u + 1]):
            t, hh = int(got[i, 0]), int(got[i, 1])
            if t in (_lib.TAG_NONE, _lib.TAG_HANG) or not 0 <= hh < hs:
                continue
            (wf if t == _lib.TAG_FULL else wr if t == _lib.TAG_REPT else wp)[u, hh] += 1
    assert np.array_equal(full, wf) and np.array_equal(pref, wp) and np.array_equal(rept, wr)
    return handed


# ---- the reads ----------------------------------------------------------------------------------------------------

def _windows(rng, lad, L, units, step, n_mut=(0,)):
    """Reads of L bases along a haplotype junk + prefix + repeat * units + suffix + junk, forward and reverse strand."""
    a, rep, b = lad[:3]
    hap = _junk(rng, L) + a + rep * units + b + _junk(rng, L)
    out = []
    for k, s in enumerate(range(0, len(hap) - L + 1, step)):
        r = hap[s:s + L]
        r = _mutate(rng, r, n_mut[k % len(n_mut)]) if n_mut[k % len(n_mut)] else r
        out.append(r if k % 2 == 0 else po.rc(r))
    return out


def _pal_open(L=150):
    """A read of the palindromic ladder that stays open after strand 0.  A mismatch would not do: it costs the score as much
    as the six windows it spoils cost the cap.  An N scores 0 and its windows count as present: score L - 3, cap L."""
    a, rep, b = PAL
    r = list((a + rep * 12 + b)[:L])
    for k in (40, 77, 101):
        r[k] = "N"
    return "".join(r)


def _shared_case(clip=0, scoring=DEFAULT):
    rng = np.random.default_rng(101)
    L = 150
    uld = _windows(rng, ULD, L, 6, 7, (0, 0, 2, 3)) + _windows(rng, ULD, L, 11, 11, (0, 1))
    # inside the repeat, both strands: pure motif copies share their 6-mers with the other strand's templates
    uld += [(ULD[1] * 14)[k:k + L] for k in (0, 5)] + [po.rc((ULD[1] * 14)[k:k + L]) for k in (0, 7)]
    uld += [_mutate(rng, (ULD[0][-10:] + ULD[1] * 13)[:L], 2), po.rc(_mutate(rng, (ULD[1] * 12 + ULD[2])[-L:], 3))]
    pal = _windows(rng, PAL, L, 9, 13, (0, 1, 0, 2)) + [_pal_open(), (PAL[0] + PAL[1] * 12 + PAL[2])[:L], (PAL[1] * 30)[:L],
                                                         _mutate(rng, (PAL[1] * 30)[:L], 2)]
    hd = _windows(rng, HD, L, 20, 17, (0, 0, 1))
    # shorter than the ladder was sized for: with clip = 1 the REPT cut-off follows the read's own length
    hd += [(HD[1] * 40)[:80], po.rc((HD[1] * 40)[:95]), (HD[0][-8:] + HD[1] * 40)[:70]]
    pal += [(PAL[1] * 30)[:90]]
    lads = [_lad(ULD, L), _lad(PAL, L), _lad(HD, L)]
    return Case(lads, [(0, uld[:len(uld) // 2]), (1, pal), (2, hd), (0, uld[len(uld) // 2:])], scoring=scoring, clip=clip, max_len=L)


_CASES = {}


def _cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def test_shared_six_mers_every_kind_of_read(ctx):
    case = _cached("shared", _shared_case)
    M = case.model()
    uld, pal, hd = (case.read_lad == k for k in (0, 1, 2))
    c3 = M["cls"] == 3
    assert (uld & c3 & ~M["to_b"]).any()                       # class 3, settled by strand 0: no strand 1
    assert (uld & c3 & M["to_b"] & M["win1"]).any()            # stays open, strand 1 wins
    assert ((uld | pal) & c3 & M["to_b"] & ~M["win1"] & (M["want"][:, 0] != 0)).any()   # stays open, strand 1 loses
    assert (hd & (M["cls"] == 2) & M["to_b"]).any() and (hd & (M["cls"] == 1)).any()    # reverse-strand reads, forward reads
    # equal (score, units) on both strands of the palindromic ladder, with strand 1 really swept
    assert (pal & M["tie"] & M["to_b"]).any() and (pal & M["tie"])[pal & (M["want"][:, 0] != 0)].all()
    handed = _check(ctx, case)
    assert 0 < handed < len(case.reads)


def _edge_units(kind):
    L = 150
    a, rep, b = PAL
    x = _pal_open()
    perfect = (a + rep * 12 + b)[:L]
    hd_f = ("TTGACCAGTA" * 3 + HD[0] + HD[1] * 20 + HD[2] + "GATTACAGGC" * 8)[10:10 + L]
    if kind == "bins":          # the same read 1, 4 and 5 times in three ladders of the same sequences: one bin each, in both passes
        return [(0, [x]), (1, [x] * 4), (2, [x] * 5)]
    if kind == "none":          # settled by strand 0 / forward only; the second unit has no reads
        return [(0, [perfect] * 3), (1, []), (3, [hd_f] * 6)]
    assert kind == "all"        # open after strand 0 / reverse only
    return [(0, [x] * 2), (2, []), (3, [po.rc(hd_f)] * 5), (1, [x] * 7)]


@pytest.mark.parametrize("kind", ("bins", "none", "all"))
def test_bin_and_quad_edges(ctx, kind):
    L = 150
    case = _cached(kind, lambda: Case([_lad(PAL, L)] * 3 + [_lad(HD, L)], _edge_units(kind), max_len=L))
    M = case.model()
    n = len(case.reads)
    if kind == "bins":
        assert M["to_b"].all() and (M["cls"] == 3).all()
    assert int(M["to_b"].sum()) == {"bins": n, "none": 0, "all": n}[kind]
    assert _check(ctx, case) == {"bins": n, "none": 0, "all": n}[kind]


def test_plain_reference_next_to_a_ladder(ctx):
    """A plain reference (max_units == 0: one strand, no pass B for its reads) and a two-strand ladder in one call; the plain
    reference's results are checked against the single-launch dump and its scores against the oracle's alignment."""
    rng = np.random.default_rng(5)
    L = 150
    ref = PLAIN[0]
    plain = [ref, ref[5:50], _mutate(rng, ref, 2), po.rc(ref), _junk(rng, 40) + ref[3:45] + _junk(rng, 30), _junk(rng, 60)]
    hd = _windows(rng, HD, L, 18, 29)
    case = Case([PLAIN, _lad(HD, L)], [(0, plain[:4]), (1, hd), (0, plain[4:])], max_len=L)
    M = case.model()
    assert M["to_b"].any() and not M["to_b"][case.read_lad == 0].any()
    _check(ctx, case)
    tag, h, sc, _ = _classify(ctx, case)
    idx = np.nonzero(case.read_lad == 0)[0]
    pairs = po.sw_pairs(case.reads, [ref], idx, [0] * len(idx))
    for i, row in zip(idx, pairs):
        assert h[i] == 0 and (tag[i] == _lib.TAG_NONE or sc[i] == row[0]), (i, tag[i], sc[i], row)
    assert (tag[idx] != _lib.TAG_NONE).any()


def test_clipped_reads(ctx):
    case = _cached("clip", lambda: _shared_case(clip=1))
    assert 0 < _check(ctx, case)
    assert (case.model()["want"] != _cached("shared", _shared_case).model()["want"]).any()   # clip changes some REPT tag


def test_scoring_outside_the_filter_premise(ctx):
    """mismatch < 5 * match: no 6-mer threshold and no cap from the counts -- every read is of class 3, and the re-pack
    falls back to L * match."""
    case = _cached("loose", lambda: _shared_case(scoring=LOOSE))
    M = case.model()
    assert (M["cls"] == 3).all() and M["to_b"].any() and not M["to_b"].all()
    _check(ctx, case)


@pytest.mark.parametrize("L", (64, 150, 160))
def test_read_lengths_at_the_instantiation_edges(ctx, L):
    def make():
        rng = np.random.default_rng(300 + L)
        lads = [_lad(ULD, L), _lad(PAL, L), _lad(HD, L)]
        units = []
        for k, lad in enumerate((ULD, PAL, HD)):
            rr = _windows(rng, lad, L, max(2, L // (3 * len(lad[1]))), 11 if L > 64 else 5, (0, 1, 0, 2))
            rr += [r[:L - 7] for r in rr[:4]] + [r[:max(30, L // 2)] for r in rr[4:7]]
            units.append((k, rr))
        # one read longer than 16 * rows: never aligned, flagged once
        units.append((1, [(PAL[0] + PAL[1] * 40 + PAL[2])[:16 * _rows(L) + 3]]))
        return Case(lads, units, max_len=L)
    case = _cached(("len", L), make)
    M = case.model()
    assert max(len(r) for r in case.reads[:-1]) == L and len(case.reads[-1]) > 16 * _rows(L)
    assert M["to_b"].any() and not M["to_b"].all() and (M["want"][:, 0] == _lib.TAG_INVALID).sum() == 1
    _check(ctx, case)


def test_two_batches_on_one_context_match_fresh_contexts(ctx):
    """The arg-max words of a call must not leak into the next one: same read indices, other reads."""
    first = _cached("shared", _shared_case)
    second = Case(first.ladders, [(int(l), first.reads[first.uro[u]:first.uro[u + 1]][::-1])
                                   for u, l in list(enumerate(first.ul))[::-1]], max_len=150)
    ctx.set_ladders(first.ladders)
    on_one = [_classify(ctx, c)[:3] for c in (first, second, first)]
    fresh = []
    for c in (first, second):
        c2 = _lib.Context(0)
        try:
            c2.set_ladders(c.ladders)
            fresh.append(_classify(c2, c)[:3])
        finally:
            c2.close()
    for got, ref in zip(on_one, fresh + fresh[:1]):
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    for c, got in zip((first, second), on_one):
        assert np.array_equal(np.stack(got, 1).astype(np.int64), c.model()["want"])
