"""When sw_cont_kernel leaves a strand, restated in numpy (csrc/sw_ladder.hip: sweep_column, template_end, steady_exit).

The trunk prefix + repeat * max_units is swept column by column for all reads of one ladder and strand at once, every value
one integer score << 18 | start_col << 9 | start_row as in the kernel (true scores here, not the kernel's anti-diagonal
scale), with the kernel's recurrences: the stored H holds the floor Z (score 0, start at the next cell), E is fed from H
without the vertical-gap term, padding rows score PAD.  At every template end the H and E entries of the column give

  lo   the smallest recorded start column (the steady-state test: lo >= alen, one period later lo >= alen + period)
  M1   the largest score + G1(row) over the entries whose start column is < alen + period      (-BIG: no such entry)
  M2   the same with G2                                                                        (the new test: M < need)

  G1(row) = match * (L - 1 - row)                                  what any path can still gain in the rows below `row`
  G2(row) = match * min(L - 1 - row, 5 + Wtail[lane of row])       Wtail = the read's 6-mer windows that start at or after
                                                                   the lane's first row and are present in the strand's
                                                                   templates (a window with a read N counts as present)

Template scores and coordinates come from the oracle (oracle/pyoracle.sw_pairs: the unpruned sweep), the tag rules are
bam_parser.py:133-168 as the kernel has them.  `replay` walks a wave of up to four reads through a strand exactly as the
kernel's loop does -- template drop, strand exit, the steady-state test and, by `rule`, the test of this module -- and
returns the trunk columns swept and every read's arg-max word.

Run as a program it builds reads with synth.build_batch, packs them into quads by (ladder, weight // 6) as the device does
and prints per read the exit period under the old and the new rule and the predicted change of trunk columns per wave:

    python -m tests.sw_exit_model [--samples 3] [--readlen 150] [--seed 1]
"""
import argparse
import sys

import numpy as np

from . import kmer_weight_model as km

K = 1 << 18
PAY = K - 1
BIG = 1 << 40
PAD = -(1 << 12)          # score of a padding row against any letter
TAG_NONE, TAG_FULL, TAG_PREF, TAG_POST, TAG_REPT, TAG_HANG = 0, 1, 2, 3, 4, 5
FLANK = 9
CODE = {c: i for i, c in enumerate("ACGT")}


def kernel_rule(R, generic):
    """The rule sw_cont_kernel runs: the bounded-gain test is compiled into the two production instantiations (7 and 10 rows
    per lane, GENERIC = false: no dump, no branch long enough to pass the score filter alone); the others keep the old one."""
    return "tier1" if not generic and R in (7, 10) else "old"


def rows_per_lane(max_len):
    return 4 if max_len <= 64 else 7 if max_len <= 112 else 10 if max_len <= 160 else 16 if max_len <= 256 else 20 if max_len <= 320 else 32


def encode(s):
    return np.asarray([CODE.get(c, 4) for c in s.upper()], np.int64)


def kmer_threshold(scoring):
    m, x, go, _ = scoring
    return -(-30 // m) - 5 if min(x, go) >= 5 * m else 0


def strand_parts(prefix, repeat, suffix):
    """[(a, rep, b)] of the two strands (bam_parser.py:92-93)."""
    return [(km.letters(prefix), km.letters(repeat), km.letters(suffix)), (km.rc(suffix), km.rc(repeat), km.rc(prefix))]


class Tables:
    """The 6-mer tables of one ladder: per strand presence (4096 bools) and class j (4096 ints), and the N flag."""

    def __init__(self, prefix, repeat, suffix, max_units):
        self.flag, tabs = km.ladder_tables(prefix, repeat, suffix, max_units)
        self.present = np.zeros((2, 4096), bool)
        self.cls = np.zeros((2, 4096), np.int64)
        for s in range(2):
            for kmer, j in tabs[s].items():
                self.present[s, km.index_of(kmer)] = True
                self.cls[s, km.index_of(kmer)] = j


def window_presence(codes, lens, tables, strand):
    """present [n, Lmax - 5] (window starting at row w lies in the read and counts), weight W [n] = cnt - ceil(J / 6)."""
    n, lmax = codes.shape
    nw = max(lmax - 5, 0)
    idx = np.zeros((n, nw), np.int64)
    has_n = np.zeros((n, nw), bool)
    for k in range(6):
        c = codes[:, k:k + nw]
        idx |= (c & 3) << (2 * k)
        has_n |= c >= 4
    inside = np.arange(nw)[None, :] + 6 <= lens[:, None]
    plain = inside & ~has_n
    pres = inside & (has_n | tables.present[strand][idx])
    jsum = np.where(plain & pres, tables.cls[strand][idx], 0).sum(1) if tables.flag else np.zeros(n, np.int64)
    return pres, pres.sum(1) - (jsum + 5) // 6


def gain_bounds(lens, pres, R, match, tier2):
    """G1, G2 [n, 16R]: what a path can still gain in the rows below each row (G2 = G1 where tier2 is off)."""
    n = len(lens)
    rows = np.arange(16 * R)
    g1 = match * (lens[:, None] - 1 - rows[None, :])
    if not tier2:
        return g1, g1.copy()
    nw = pres.shape[1]
    # windows that start at or after row w, w = 0 .. : a suffix sum; lanes beyond the last window have none
    tail = np.zeros((n, 16 * R + 1), np.int64)
    tail[:, :nw] = np.cumsum(pres[:, ::-1], 1)[:, ::-1]
    wtail = np.minimum(tail[:, (rows // R) * R], 255)
    return g1, np.minimum(g1, match * (5 + wtail))


def sweep_trunk(codes, lens, trunk, alen, period, max_units, scoring, R, g1, g2):
    """lo, M1, M2 [max_units + 1, n] (index u = the template whose end column the state belongs to; index 0 unused)."""
    m, x, go, ge = scoring
    n = codes.shape[0]
    nr = 16 * R
    rows = np.arange(nr, dtype=np.int64)
    rd = np.full((n, nr), 5, np.int64)
    rd[:, :codes.shape[1]] = codes[:, :nr]
    rd[rows[None, :] >= lens[:, None]] = 5
    # profile: score of every row against the letters 0..3 and N
    prof = np.zeros((5, n, nr), np.int64)
    for l in range(4):
        prof[l] = np.where(rd == 5, PAD, np.where(rd == 4, 0, np.where(rd == l, m, -x)))
    prof[4] = np.where(rd == 5, PAD, 0)
    prof *= K
    H = np.broadcast_to(rows + 1, (n, nr)).copy()          # Z(i, -1)
    E = np.full((n, nr), -BIG, np.int64)
    ramp = rows * ge * K
    lo = np.zeros((max_units + 1, n), np.int64)
    M1 = np.full((max_units + 1, n), -BIG, np.int64)
    M2 = np.full((max_units + 1, n), -BIG, np.int64)
    thr_new = (alen + period) << 9
    u = 1
    for c in range(alen + period * max_units):
        diag = np.empty_like(H)
        diag[:, 1:] = H[:, :-1]
        diag[:, 0] = c << 9                               # Z(-1, c - 1)
        z = ((c + 1) << 9) + rows + 1
        v = np.maximum(np.maximum(diag + prof[trunk[c]], z[None, :]), E)
        # F[i] = max over i' < i of v[i'] - go - (i - i' - 1) * ge
        acc = np.maximum.accumulate(v + ramp[None, :] - go * K, axis=1)
        F = np.full_like(v, -BIG)
        F[:, 1:] = acc[:, :-1] - ramp[None, :-1]
        H = np.maximum(v, F)
        E = np.maximum(E - ge * K, v - go * K)
        if c == alen + period * u - 1:
            both = np.concatenate([H, E], 1)
            start = both & 0x3FE00
            lo[u] = start.min(1)
            old = start < thr_new
            sc = both >> 18
            M1[u] = np.where(old, sc + np.concatenate([g1, g1], 1), -BIG).max(1)
            M2[u] = np.where(old, sc + np.concatenate([g2, g2], 1), -BIG).max(1)
            u += 1
    return lo >> 9, M1, M2


def template_tags(res, L, T, u, mu_rept, period, flank=FLANK):
    """bam_parser.py:133-168 on arrays: res [..., 5] = score, ref_begin, ref_end, read_begin, read_end."""
    score, rb, re, qb, qe = (res[..., k].astype(np.int64) for k in range(5))
    min_len = np.minimum(L, T) >> 1
    ok = (score >= np.maximum(min_len, 30)) & (qe - qb + 1 >= min_len)
    aL, aR, bL, bR = rb, T - re - 1, qb, L - qe - 1
    hang = np.minimum(np.minimum(aR + bL, aL + bR), np.minimum(aL + aR, bL + bR))
    pre, suf = rb < flank, re > T - flank - 1
    tag = np.where(hang >= flank, TAG_HANG,
                   np.where(pre, np.where(suf, TAG_FULL, TAG_PREF),
                            np.where(suf, TAG_POST, np.where((u >= mu_rept - 1) & (u * period <= L), TAG_REPT, TAG_NONE))))
    return np.where(ok, tag, TAG_NONE)


class Strand:
    """Everything the replay needs for the reads of one ladder on one strand."""

    def __init__(self, reads, ladder, strand, scoring, R, clip=False, oracle_threads=4):
        from oracle import pyoracle as po
        prefix, repeat, suffix, mu = ladder
        a, rep, b = strand_parts(prefix, repeat, suffix)[strand]
        self.alen, self.blen, self.period, self.mu, self.R = len(a), len(b), len(rep), mu, R
        self.scoring = tuple(scoring)
        m = scoring[0]
        n = len(reads)
        self.lens = np.asarray([len(r) for r in reads], np.int64)
        lmax = max(16 * R, int(self.lens.max()) if n else 0)
        codes = np.full((n, lmax), 4, np.int64)
        for i, r in enumerate(reads):
            codes[i, :len(r)] = encode(r)
        tables = Tables(prefix, repeat, suffix, mu)
        thr = kmer_threshold(scoring)
        self.premise = thr > 0
        self.thr = thr
        pres, self.W = window_presence(codes, self.lens, tables, strand)
        self.tier2 = self.premise and R in (7, 10)
        self.g1, self.g2 = gain_bounds(self.lens, pres, R, m, self.tier2)
        self.kcap = (self.W + 5) * m if self.tier2 else np.full(n, 1 << 20, np.int64)
        self.cap = np.minimum(self.kcap, self.lens * m)
        trunk = encode(a + rep * mu)
        self.lo, self.M1, self.M2 = sweep_trunk(codes, self.lens, trunk, self.alen, self.period, mu, scoring, R, self.g1, self.g2)
        tmpl = [a + rep * u + b for u in range(1, mu + 1)]
        pr = np.repeat(np.arange(n), mu)
        pt = np.tile(np.arange(mu), n)
        res = po.sw_pairs(list(reads), tmpl, pr, pt, scoring=scoring, threads=oracle_threads).reshape(n, mu, 5)
        us = np.arange(1, mu + 1)[None, :]
        self.T = self.alen + self.period * us + self.blen                       # [1, mu]
        mu_rept = -(-self.lens // self.period)[:, None] if clip else mu
        self.score = np.zeros((n, mu + 2), np.int64)
        self.tag = np.zeros((n, mu + 2), np.int64)
        self.score[:, 1:mu + 1] = res[..., 0]
        self.tag[:, 1:mu + 1] = template_tags(res, self.lens[:, None], self.T, us, mu_rept, self.period)

    def min_score(self, i, u):
        return max(min(int(self.lens[i]), self.alen + self.period * u + self.blen) >> 1, 30)

    def still_open(self, i, u, best):
        return max(self.min_score(i, u), (best >> 12) + 1) <= self.cap[i]

    def need(self, i, u, best):
        bestS, bestU = best >> 12, 511 - ((best >> 3) & 511)
        return max(self.min_score(i, u), bestS + 1 if u >= bestU else bestS)


def replay(st, idx, best, rule):
    """One wave (reads idx of Strand st, arg-max words best) through the strand.  rule: 'none' (no steady-state exit),
    'old', 'tier1', 'tier2' (tier 2 where the strand has it).  -> (trunk columns swept, new arg-max words, exit reason)."""
    idx = list(idx)
    best = list(best)
    if st.tier2 and not any(st.W[i] >= st.thr for i in idx):
        return 0, best, "filter"
    if not any(st.still_open(i, 1, best[k]) for k, i in enumerate(idx)):
        return 0, best, "closed"
    M = st.M2 if rule == "tier2" else st.M1
    cols = st.alen
    ok_run = 0
    u = 1
    while True:
        cols += st.period
        need = [st.need(i, u, best[k]) for k, i in enumerate(idx)]
        dropped = not any(st.score[i, u] >= need[k] for k, i in enumerate(idx))
        if not dropped:
            for k, i in enumerate(idx):
                cand = (int(st.score[i, u]) << 9 | (511 - u)) << 3
                if st.tag[i, u] != TAG_NONE and cand > (best[k] | 7):
                    best[k] = cand | int(st.tag[i, u])
        u += 1
        if not any(st.still_open(i, u, best[k]) for k, i in enumerate(idx)):
            return cols, best, "strand"
        if u > st.mu:
            return cols, best, "end"
        if not dropped or rule == "none":
            ok_run = 0
            continue
        # (the kernel asks the new test only once some read of the wave has a candidate)
        if rule in ("tier1", "tier2") and any(x >= 0 for x in best) and all(M[u - 1, i] < st.need(i, u, best[k]) for k, i in enumerate(idx)):
            return cols, best, "new"
        thr = st.alen + (st.period if ok_run else 0)
        if any(st.lo[u - 1, i] < thr for i in idx):
            ok_run = 0
        elif ok_run:
            return cols, best, "steady"
        else:
            ok_run = 1


def winners(best):
    """(tag, units, score) of an arg-max word, as the kernel's epilogue writes them."""
    if best < 0 or best & 7 == TAG_NONE:
        return (0, 0, 0)
    return (best & 7, 511 - ((best >> 3) & 511), best >> 12)


def level_key(w):
    return 31 - min(31, int(w) // 6)


def pack_quads(weights, members):
    """Quads of one ladder and pass: the reads `members` by level, high levels first, four to a quad in index order."""
    out = []
    by = {}
    for i in members:
        by.setdefault(level_key(weights[i]), []).append(i)
    for key in sorted(by):
        g = by[key]
        out += [g[k:k + 4] for k in range(0, len(g), 4)]
    return out


def ladder_passes(reads, ladder, scoring, R, rules, clip=False):
    """Both passes of one ladder's reads under each rule -> {rule: dict(cols, waves, best, periods)}; periods: per read and
    strand the number of periods a wave of that read alone sweeps (-1: the read does not enter the strand)."""
    n = len(reads)
    st = [Strand(reads, ladder, s, scoring, R, clip) for s in range(2)]
    out = {}
    for rule in rules:
        best = [-1] * n
        cols = waves = 0
        periods = np.full((n, 2), -1, np.int64)
        for s in range(2):
            if s == 0:
                members = [i for i in range(n) if st[0].W[i] >= st[0].thr or not st[0].premise]
            else:
                members = [i for i in range(n) if (st[1].W[i] >= st[1].thr or not st[1].premise) and st[1].still_open(i, 1, best[i])]
            for i in members:
                c, _, _ = replay(st[s], [i], [best[i]], rule)
                periods[i, s] = (c - st[s].alen) // st[s].period if c else 0
            for quad in pack_quads(st[s].W, members):
                c, nb, _ = replay(st[s], quad, [best[i] for i in quad], rule)
                for i, b in zip(quad, nb):
                    best[i] = b
                cols += c
                waves += 1
        out[rule] = dict(cols=cols, waves=waves, best=best, periods=periods)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--readlen", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--per-read", action="store_true", help="print one line per read: ladder, read, exit period old / tier 1 / tier 2")
    args = ap.parse_args(argv)
    from tredparse_amd import synth
    loci = [l for l in synth.load_loci() if l["name"] not in ("FXTAS", "AR")]
    b = synth.build_batch(args.seed, loci, args.samples, synth.SynthParams(readlen=args.readlen))
    scoring = (1, 5, 7, 2)
    R = rows_per_lane(args.readlen)
    rules = ("none", "old", "tier1", "tier2")
    tot = {r: [0, 0] for r in rules}
    hist = {r: np.zeros(64, np.int64) for r in rules}
    read_lad = np.repeat(b.unit_ladder, np.diff(b.unit_read_off))
    for li, lad in enumerate(b.ladders):
        rows = np.nonzero(read_lad == li)[0]
        reads = [synth.decode(b.codes[i]) for i in rows]
        res = ladder_passes(reads, lad, scoring, R, rules)
        for r in rules:
            tot[r][0] += res[r]["cols"]
            tot[r][1] += res[r]["waves"]
            p = res[r]["periods"]
            hist[r] += np.bincount(np.minimum(p[p >= 0], 63), minlength=64)
            assert [winners(x) for x in res[r]["best"]] == [winners(x) for x in res["none"]["best"]], (lad, r)
        if args.per_read:
            for k, i in enumerate(rows):
                print(loci[li]["name"], int(i), *(tuple(res[r]["periods"][k]) for r in ("old", "tier1", "tier2")))
        print("{:8s} reads {:5d}  trunk columns none {:7d} old {:7d} tier1 {:7d} tier2 {:7d}".format(
            loci[li]["name"], len(rows), *(res[r]["cols"] for r in rules)), flush=True)
    print("readlen", args.readlen, "samples", args.samples, "reads", b.n_reads)
    for r in rules:
        print("{:6s} waves {:7d} trunk columns {:9d}  per wave {:7.2f}  vs old {:+.2%}".format(
            r, tot[r][1], tot[r][0], tot[r][0] / max(1, tot[r][1]), tot[r][0] / max(1, tot["old"][0]) - 1))
    for r in ("old", "tier1", "tier2"):
        h = hist[r]
        print(r, "mean periods swept by a read alone {:.2f}".format((h * np.arange(64)).sum() / max(1, h.sum())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
