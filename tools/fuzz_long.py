#!/usr/bin/env python3
"""Randomised parity campaign of the long-read kernel (csrc/sw_long.hip, tredlong_sw_classify through
Context.set_long_reads) against the restated ssw_align / _parseReadSW of oracle/sw_oracle.c (plain ints, no size limit;
tests/test_oracle_sw.py pins it to the compiled reference, long pairs at these scorings included).

Per round: one of ten scorings (the last three are corners of the accepted range), 2-3 ladders of periods 3 / 4 / 5 / 6 /
12 with a small max_units, one of them beyond 511 columns; ~40 reads of 1 ... 2 048 bp on both strands, so that the three
row classes (8 / 16 / 32 rows per lane) meet in every call; reads of <= 480 bp go to the long ladder, the only way they
reach this kernel.  Compared: (tag, h, score) of every read, and every template's dump row field by field (the rows
beyond a ladder's own templates must stay -1).  Not part of the test suite beyond the fixed-seed slice of
tests/test_fuzz_gpu.py; prints one JSON line.

usage: python tools/fuzz_long.py [rounds] [seed]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCORINGS = ((1, 5, 7, 2), (2, 2, 3, 1), (1, 4, 6, 1), (1, 1, 2, 1), (3, 5, 7, 2), (1, 0, 1, 1), (1, 9, 12, 3),
            (8, 16, 16, 16), (8, 0, 1, 1), (1, 16, 16, 1))
LENGTHS = (1, 36, 150, 481, 511, 512, 513, 700, 1023, 1024, 1025, 1500, 2047, 2048)
LOCI = {3: "HD", 4: "DM2", 5: "SCA10", 6: "SCA36", 12: "ULD"}
KINDS = ("spanning", "prefix", "suffix", "inside", "pure", "random", "all_n", "n_runs", "two_letter")
# the oracle's cost is reads x templates x cells: on a ladder beyond this many columns only reads up to 700 bp are drawn
WIDE = 1200


def _rand(rng, n, letters="ACGT"):
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


def _mutate(rng, s, rate):
    """Substitutions, insertions and deletions, each base at `rate` (a third each)."""
    if rate == 0 or not s:
        return s
    out = []
    for ch, x in zip(s, rng.random(len(s))):
        if x >= rate:
            out.append(ch)
        elif x < rate / 3:
            out.append("ACGT"[int(rng.integers(4))])
        elif x < 2 * rate / 3:
            out.append(ch + "ACGT"[int(rng.integers(4))])
    return "".join(out)


def draw_read(rng, ladder, L, kind):
    """One read of exactly L letters of the given kind against `ladder` (forward strand; the caller turns it)."""
    pre, rep, suf, mu = ladder
    p = len(rep)
    units = int(rng.integers(1, mu + 3))
    left, right = _rand(rng, L + 20), _rand(rng, L + 20)
    g = left + pre + rep * units + suf + right
    a = len(left)
    b = a + len(pre) + p * units
    if kind in ("spanning", "prefix", "suffix", "inside", "n_runs"):
        start = {"spanning": (a + b + len(suf)) // 2 - L // 2, "prefix": a + len(pre) + 3 * p - L, "suffix": b - 3 * p,
                 "inside": a + len(pre) + int(rng.integers(0, p * units)),
                 "n_runs": a + int(rng.integers(-L // 2, len(pre) + p * units))}[kind]
        start = min(max(start, 0), len(g) - L - 20)
        r = _mutate(rng, g[start:start + L + 20], float(rng.choice([0.0, 0.01, 0.05])))
        r = (r + right)[:L]
        if kind == "n_runs":
            r = list(r)
            for _ in range(int(rng.integers(1, 4))):
                k = int(rng.integers(0, L))
                n = int(rng.integers(1, 51))
                r[k:k + n] = "N" * len(r[k:k + n])
            r = "".join(r)
    elif kind == "pure":
        ph = int(rng.integers(p))
        r = _mutate(rng, (rep * (L // p + 4))[ph:ph + L + 20], float(rng.choice([0.0, 0.0, 0.01])))
        r = (r + rep * (L // p + 2))[:L]
    elif kind == "random":
        r = _rand(rng, L)
    elif kind == "all_n":
        r = "N" * L
    else:
        # two letters of the repeat, in runs or alternating: many cells share the best score (end- and begin-cell ties)
        two = "".join(sorted(set(rep)))[:2] if len(set(rep)) > 1 else rep[0] + "A"
        mode = int(rng.integers(3))
        if mode == 0:
            r = _rand(rng, L, two)
        elif mode == 1:
            r = (two * (L // 2 + 1))[:L]
        else:
            r = two[int(rng.integers(2))] * L
    assert len(r) == L
    return r


def draw_round(rng, by_period):
    """(ladders, reads, unit_read_off, unit_ladder, clip): one call's worth."""
    periods = [int(x) for x in rng.choice(sorted(LOCI), int(rng.integers(2, 4)), replace=False)]
    ladders = []
    long_k = int(rng.integers(len(periods)))
    for k, p in enumerate(periods):
        l = by_period[p]
        flanks = len(l["prefix"]) + len(l["suffix"])
        mu = min(int(rng.integers(5, 61)), (511 - flanks) // p)
        if k == long_k:
            # beyond 511 columns through max_units; now and then far beyond, up to the 4 095 the path takes
            cols = int(rng.choice([512, 513, 600, 800, 1100])) if rng.random() < 0.85 else int(rng.integers(2000, 4096))
            mu = max(-(-(cols - flanks) // p), (512 - flanks) // p + 1)
            mu = min(mu, (4095 - flanks) // p)
        ladders.append((l["prefix"], l["repeat"], l["suffix"], mu))
        assert (512 <= flanks + p * mu <= 4095) if k == long_k else (flanks + p * mu <= 511)
    long_cols = len(ladders[long_k][0]) + len(ladders[long_k][2]) + periods[long_k] * ladders[long_k][3]
    per_unit = []
    units = [int(x) for x in rng.permutation(np.repeat(np.arange(len(ladders)), 2))]
    for lad in units:
        reads = []
        for _ in range(int(rng.integers(4, 10))):
            L = int(rng.choice(LENGTHS))
            if lad != long_k and L <= 480:
                L = int(rng.choice([x for x in LENGTHS if x > 480]))
            if lad == long_k and long_cols > WIDE and L > 700:
                L = int(rng.choice([x for x in LENGTHS if x <= 700]))
            r = draw_read(rng, ladders[lad], L, KINDS[int(rng.integers(len(KINDS)))])
            reads.append(r if rng.random() < 0.5 else _rc(r))
        per_unit.append(reads)
    reads = [r for u in per_unit for r in u]
    uro = np.concatenate([[0], np.cumsum([len(u) for u in per_unit])]).astype(np.int32)
    return ladders, reads, uro, np.asarray(units, np.int32), bool(rng.random() < 0.3)


def _rc(s):
    return s.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


def campaign(rounds=20, seed=1, threads=16):
    """Runs the campaign and returns its summary (tests/test_fuzz_gpu.py runs a fixed-seed slice of it).  The scorings are
    drawn without replacement, ten rounds at a time, so that ten rounds meet every one of them."""
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    from oracle import pyoracle as po
    from tredparse_amd import _lib, synth
    by_period = {len(l["repeat"]): l for l in synth.load_loci() if l["name"] in LOCI.values()}
    rng = np.random.default_rng(seed)
    ctx = _lib.Context(0)
    ctx.set_long_reads(True)
    n_reads = n_bad = n_pairs = n_bad_pairs = 0
    classes = np.zeros(3, np.int64)
    seen = {}
    t_oracle = 0.0
    t0 = time.time()
    order = []
    for k in range(rounds):
        if not order:
            order = [int(x) for x in rng.permutation(len(SCORINGS))]
        scoring = SCORINGS[order.pop()]
        seen["/".join(map(str, scoring))] = seen.get("/".join(map(str, scoring)), 0) + 1
        ladders, reads, uro, ulad, clip = draw_round(rng, by_period)
        n = len(reads)
        lens = np.array([len(r) for r in reads])
        ctx.set_ladders(ladders)
        packed, woff, rlen = _lib.pack_reads(reads)
        nt = max(2 * l[3] for l in ladders)
        tag = np.zeros(n, np.uint8); h = np.zeros(n, np.int16); sc = np.zeros(n, np.int16)
        dump = np.zeros((n, nt, 6), np.int16)
        ctx.sw_classify(_lib.MEM_HOST, packed, woff, rlen, n, uro, ulad, len(ulad),
                        _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], 9, int(clip), 0, 0), tag, h, sc, dump, nt)
        t1 = time.time()
        rl = np.repeat(ulad, np.diff(uro))
        ls = po.LocusSet(ladders)
        cls = po.classify(reads, rl, ls, clip=clip, scoring=scoring, threads=threads)
        pr, pt, where = [], [], []
        for r in range(n):
            for j, t in enumerate(range(ls.lad_off[rl[r]], ls.lad_off[rl[r] + 1])):
                pr.append(r); pt.append(t); where.append((r, j))
        want = po.sw_pairs(reads, ls.templates, pr, pt, scoring=scoring, threads=threads)
        t_oracle += time.time() - t1
        where = np.asarray(where)
        got = dump[where[:, 0], where[:, 1], :5].astype(np.int32)
        bad_pairs = np.nonzero((got != want).any(axis=1))[0]
        # the rows past a ladder's own templates: untouched (-1)
        beyond = [r for r in range(n) if not (dump[r, 2 * ladders[rl[r]][3]:] == -1).all()]
        bad = np.nonzero((tag != cls[:, 0]) | (h != cls[:, 1]) | (sc != cls[:, 2]))[0]
        n_reads += n
        n_bad += len(bad)
        n_pairs += len(pr)
        n_bad_pairs += len(bad_pairs) + len(beyond)
        classes += np.bincount(np.digitize(lens, [513, 1025]), minlength=3)
        head = "seed {} round {} scoring {} clip {}".format(seed, k, scoring, clip)
        for i in bad[:4]:
            print("MISMATCH", head, "read", i, "L", lens[i], "ladder", ladders[rl[i]][1], ladders[rl[i]][3], "gpu",
                  (tag[i], h[i], sc[i]), "oracle", cls[i], file=sys.stderr)
        for i in bad_pairs[:4]:
            r, j = where[i]
            print("PAIR MISMATCH", head, "read", r, "L", lens[r], "template", j, "T", len(ls.templates[pt[i]]), "gpu", got[i],
                  "oracle", want[i], file=sys.stderr)
        for r in beyond[:2]:
            print("ROWS BEYOND THE LADDER WRITTEN", head, "read", r, "L", lens[r], file=sys.stderr)
    ctx.close()
    return {"tool": "tools/fuzz_long.py", "rounds": rounds, "seed": seed, "reads": int(n_reads), "mismatches": int(n_bad),
            "template_pairs": int(n_pairs), "pair_mismatches": int(n_bad_pairs), "class8": int(classes[0]),
            "class16": int(classes[1]), "class32": int(classes[2]), "scorings": seen, "checker": "restatement",
            "oracle_seconds": round(t_oracle, 1), "seconds": round(time.time() - t0, 1)}


def main():
    res = campaign(int(sys.argv[1]) if len(sys.argv) > 1 else 20, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    from tredparse_amd import _lib
    res["library"] = _lib.version()
    print(json.dumps(res))
    return 1 if (res["mismatches"] or res["pair_mismatches"]) else 0


if __name__ == "__main__":
    sys.exit(main())
