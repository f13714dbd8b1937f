"""The N-aware 6-mer score cap of the SW kernel (csrc/sw_ladder.hip: kmer_weight / kmer_cap, the class tables of
csrc/kmer_host.h) through tredgpu_sw_classify on device memory: one batch of four ladders -- OPMD (motif GCN), BPES (NGC), a
palindromic N ladder (prefix = rc(suffix), motif GCNNGC) and HD (no N) -- at read lengths 150 (10 rows per lane), 100 (7) and
64 (4: results only, that instantiation uses no cap).

Every read's tag, h and score must equal oracle/pyoracle.classify and the arg-max of the kernel's own per-template dump (one
launch, filter off).  The library's counter of the reads handed to pass B (counter 7) must equal a Python restatement of the
re-pack's entry test with the weight W = cnt - ceil(J / 6) (tests/kmer_weight_model.py); the same restatement with the plain
count hands over strictly more of the forward reads of the N ladders, which shows that the batch exercises the change."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tredparse_amd import _lib

from . import kmer_weight_model as km

pytestmark = pytest.mark.gpu

OPMD = ("CCAGTCTGAGCGGCGATG", "GCN", "GGGGCTGCGGGCGGTCGG")
BPES = ("GCCAGGGCTACCGGGGCC", "NGC", "CATCTGGCAGGAGGCATA")
PAL_PREFIX = "TGACCTGAAGTCCATGGA"
PAL = (PAL_PREFIX, "GCNNGC", po.rc(PAL_PREFIX))
HD = ("GAGTCCCTCAAGTCCTTC", "CAG", "CAACAGCCGCCACCGCCG")
LADS = (OPMD, BPES, PAL, HD)
SCORING = (1, 5, 7, 2)
FLANK = 9


def _rows(max_len):
    return 4 if max_len <= 64 else 7 if max_len <= 112 else 10


def _junk(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _fill(rng, s):
    return "".join("ACGT"[int(rng.integers(0, 4))] if c == "N" else c for c in s)


def _mutate(rng, s, k):
    s = list(s)
    for i in rng.choice(len(s), k, replace=False):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + int(rng.integers(0, 3))) % 4] if s[i] != "N" else "A"
    return "".join(s)


def _with_n(rng, s, k):
    s = list(s)
    for i in rng.choice(len(s), k, replace=False):
        s[i] = "N"
    return "".join(s)


def make_reads(L):
    """[(ladder, read, forward)]: about 120 reads per length."""
    rng = np.random.default_rng(1100 + L)
    out = []
    for g, lad in enumerate(LADS):
        a, rep, b = lad
        for units in (6, 20):
            hap = _junk(rng, L) + _fill(rng, a + rep * units + b) + _junk(rng, L)
            n_win = 6 if units == 6 else 4
            for k, s in enumerate(np.linspace(L // 3, len(hap) - L - L // 3, n_win).astype(int)):
                r = hap[s:s + L]                                     # PREF, FULL, POST and (20 units, short reads) REPT windows
                out.append((g, r, True))
                out.append((g, po.rc(r), False))
                if k % 3 == 0:
                    out.append((g, _mutate(rng, r, 1 + k % 3), True))
                if k % 3 == 1:
                    out.append((g, _with_n(rng, r, 1 + k % 2), True))
        inside = _fill(rng, (rep * 80)[:L + 4])                        # inside the repeat, both orientations
        out += [(g, inside[:L], True), (g, po.rc(inside[2:L + 2]), False), (g, _mutate(rng, inside[1:L + 1], 3), True)]
    # the palindromic ladder: the two strands' templates are the same strings (GCNNGC is its own reverse complement), so a
    # read that stays open after strand 0 finds an equal (score, units) on strand 1 -- an N in the read keeps it open (it
    # scores 0 but its windows count as present: score L - 3 against a cap of about L)
    a, rep, b = PAL
    t = _fill(rng, a + rep * (L // 6) + b)[:L]
    out += [(2, _with_n(rng, t, 3), True), (2, t, True)]
    return out


class Case:
    def __init__(self, L):
        self.L = L
        rr = make_reads(L)
        order = sorted(range(len(rr)), key=lambda i: rr[i][0])        # one unit per ladder
        self.reads = [rr[i][1] for i in order]
        self.forward = np.asarray([rr[i][2] for i in order])
        self.read_lad = np.asarray([rr[i][0] for i in order], np.int32)
        self.ladders = [(l[0], l[1], l[2], -(-L // len(l[1]))) for l in LADS]
        self.uro = np.searchsorted(self.read_lad, np.arange(len(LADS) + 1)).astype(np.int32)
        self.ul = np.arange(len(LADS), dtype=np.int32)
        self._model = None

    def _template_tag(self, row, L, T, u, mu, period):
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
        return _lib.TAG_REPT if u >= mu - 1 and u * period <= L else _lib.TAG_NONE

    def model(self):
        """want (n, 3); to_b / to_b_plain (n): handed to pass B under the weight W / under the plain count; win1, tie."""
        if self._model is not None:
            return self._model
        m = SCORING[0]
        thr = -(-30 // m) - 5
        with_kcap = _rows(self.L) in (7, 10)
        n = len(self.reads)
        ls = po.LocusSet(self.ladders)
        want = po.classify(self.reads, self.read_lad, ls, scoring=SCORING, threads=4).astype(np.int64)
        pr, pt = [], []
        for i in range(n):
            g = self.read_lad[i]
            pr += [i] * (ls.lad_off[g + 1] - ls.lad_off[g])
            pt += list(range(ls.lad_off[g], ls.lad_off[g + 1]))
        pairs = po.sw_pairs(self.reads, ls.templates, pr, pt, scoring=SCORING, threads=4)
        tables = [km.ladder_tables(*l) for l in self.ladders]
        to_b, to_b_plain, win1, tie = (np.zeros(n, bool) for _ in range(4))
        at = 0
        for i in range(n):
            g = int(self.read_lad[i])
            a, rep, b, mu = self.ladders[g]
            read, L, P = self.reads[i], len(self.reads[i]), len(rep)
            flag, tt = tables[g]
            cnt1, _, W1 = km.read_weight(read, tt[1], with_n=flag)
            best = [None, None]
            for k in range(2 * mu):
                u, s = k // 2 + 1, k % 2
                T = len(a) + P * u + len(b)
                tag = self._template_tag(pairs[at + k], L, T, u, mu, P)
                c = (int(pairs[at + k][0]), -u, tag)
                if tag != _lib.TAG_NONE and (best[s] is None or c[:2] > best[s][:2]):
                    best[s] = c
            at += 2 * mu
            merged = best[0] if best[1] is None or (best[0] is not None and best[1][:2] <= best[0][:2]) else best[1]
            assert tuple(want[i]) == ((merged[2], -merged[1], merged[0]) if merged else (0, 0, 0)), (i, read, want[i], best)
            need = max(max(min(L, len(a) + P + len(b)) >> 1, 30), (best[0][0] if best[0] else -1) + 1)
            for w, dst in ((W1, to_b), (cnt1, to_b_plain)):
                cap = min((w + 5) * m if with_kcap else 1 << 20, L * m)
                dst[i] = w >= thr and need <= cap
            win1[i] = to_b[i] and merged is not None and merged is best[1]
            tie[i] = best[0] is not None and best[1] is not None and best[0][:2] == best[1][:2]
        self._model = dict(want=want, to_b=to_b, to_b_plain=to_b_plain, win1=win1, tie=tie)
        return self._model


_CASES = {}


def _case(L):
    if L not in _CASES:
        _CASES[L] = Case(L)
    return _CASES[L]


def _classify(ctx, case, dump_templates=0):
    import torch
    dev = torch.device("cuda", 0)
    packed, woff, rlen = _lib.pack_reads(case.reads)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(case.reads)
    tag = torch.zeros(n, dtype=torch.uint8, device=dev); h = torch.zeros(n, dtype=torch.int16, device=dev)
    sc = torch.zeros(n, dtype=torch.int16, device=dev)
    dump = torch.zeros((n, dump_templates, 6), dtype=torch.int16, device=dev) if dump_templates else None
    torch.cuda.synchronize()
    ctx.sw_classify(_lib.MEM_DEVICE, dv(packed.view(np.int32)), dv(woff), dv(rlen), n, dv(case.uro), dv(case.ul), len(case.ul),
                    _lib.SwParams(SCORING[0], SCORING[1], SCORING[2], SCORING[3], FLANK, 0, case.L, 0), tag, h, sc, dump, dump_templates)
    ctx.sync()
    return np.stack([tag.cpu().numpy(), h.cpu().numpy(), sc.cpu().numpy()], 1).astype(np.int64), dump.cpu().numpy() if dump_templates else None


def _argmax_of_dump(case, dump):
    n = dump.shape[0]
    out = np.zeros((n, 3), np.int64)
    for i in range(n):
        mu = case.ladders[case.read_lad[i]][3]
        best = None
        for k in range(2 * mu):
            u, s = k // 2 + 1, k % 2
            score, tag = int(dump[i, k, 0]), int(dump[i, k, 5])
            if tag != _lib.TAG_NONE and (best is None or (score, -u, -s) > best[:3]):
                best = (score, -u, -s, tag)
        if best:
            out[i] = (best[3], -best[1], best[0])
    return out


@pytest.mark.parametrize("L", (150, 100, 64))
def test_results_and_reads_handed_to_pass_b(ctx, L):
    case = _case(L)
    M = case.model()
    n = len(case.reads)
    assert n <= 135                                                      # three lengths: about 400 reads in all
    n_lad = case.read_lad < 3
    fwd_n = n_lad & case.forward
    print("L", L, "reads", n, "to pass B with W", int(M["to_b"].sum()), "with the plain count", int(M["to_b_plain"].sum()),
          "forward N-ladder reads", int(fwd_n.sum()), "of them to pass B", int((fwd_n & M["to_b"]).sum()), "/", int((fwd_n & M["to_b_plain"]).sum()),
          "strand-1 wins", int(M["win1"].sum()), "ties", int((M["tie"] & M["to_b"]).sum()))
    # the batch holds what it claims
    tags = set(M["want"][:, 0])
    assert {_lib.TAG_FULL, _lib.TAG_PREF, _lib.TAG_POST, _lib.TAG_REPT} <= tags
    assert M["win1"].any()                                               # a read whose strand-1 candidate wins
    assert (M["tie"] & M["to_b"] & (case.read_lad == 2)).any()           # an equal score on the palindromic ladder, strand 1 swept
    assert not (M["to_b"] & ~M["to_b_plain"]).any()                      # W <= count: the weight never hands over more
    if _rows(L) in (7, 10):
        # the old rule would hand over strictly more of the forward reads of the N ladders
        assert (fwd_n & M["to_b_plain"]).sum() > (fwd_n & M["to_b"]).sum()
        assert (M["to_b_plain"] == M["to_b"])[~n_lad].all()              # HD: no class table, nothing changes
    ctx.set_ladders(case.ladders)
    ctx.reset_timing()
    got, _ = _classify(ctx, case)
    out = np.zeros(8, np.uint64)
    assert ctx.lib.tredgpu_get_sw_counters(ctx.h, out.ctypes.data) == 0
    handed = int(out[7])
    bad = np.nonzero((got != M["want"]).any(1))[0]
    assert len(bad) == 0, ("oracle", bad[:5], [case.reads[i] for i in bad[:3]], got[bad[:5]], M["want"][bad[:5]])
    nt = 2 * max(l[3] for l in case.ladders)
    got2, dump = _classify(ctx, case, nt)
    by_dump = _argmax_of_dump(case, dump)
    bad = np.nonzero((got != by_dump).any(1))[0]
    assert len(bad) == 0, ("dump", bad[:5], [case.reads[i] for i in bad[:3]], got[bad[:5]], by_dump[bad[:5]])
    assert np.array_equal(got, got2)
    assert handed == int(M["to_b"].sum()), (handed, int(M["to_b"].sum()), int(M["to_b_plain"].sum()))
