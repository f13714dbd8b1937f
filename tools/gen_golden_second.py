#!/usr/bin/env python3
"""Record the reference's second-best alignments as golden vectors: tests/golden/sw_second.npz.

BUILD-CONTAINER ONLY (CPU): every expected value is the compiled reference's -- src/ssw.c as oracle/_ref/libssw.so,
ssw_init(..., 2) and ssw_align with flag 0 through ctypes (tools/fuzz_second.py: run_reference), so that its CIGAR pass
and that pass's faults are never reached.  Nothing of the reference is stored, only these inputs and outputs.

Items (class, ladder, template, read, scoring, mask_len -> score1, ref_end1, score2, ref_end2):
  r  per scoring about 30 random / periodic plain pairs of tools/fuzz_second.py's make_pair (substitutions, N, indels)
  l  per scoring about 30 reads on template ladders of period 2-12, both strands, the template one of the ladder's own
  p  padding: reads of 15, 16, 17, 24 and 25 bp (1 / 0 / 15 byte and 1 / 0 / 7 word padding rows), and reads whose last
     row carries a value out of the mask over mismatching reference letters (the plain recurrence decays there)
  b  pass boundary: exact-match reads of 249 and 250 bp at 1/5/7/2 (score1 + 5 = 254 / 255) with the runner-up ending
     exactly at ref_end1 + maskLen and at ref_end1 + maskLen + 1
  m  mask edges: the optimal path's own cell at ref_end1 - maskLen - 1; ref_end1 - maskLen <= 0; ref_end1 + maskLen >=
     refLen; equal maxima on both sides (the left one wins) and a greater one on the right; no second best (0, 0);
     mask_len 14 (0, -1); reads of 30, 31 and 32 bp (maskLen 15, 15, 16)
  c  row classes: reads on both sides of the unit's thresholds (64, 128, 256, 512, 1 024 bp), 480 / 481, 2 047 / 2 048,
     and a 4 095-column template
The crafted classes are at 1/5/7/2; what each is crafted for is asserted on the reference's values here.

A pair on which tests/second_model differs from the reference may be left out only when gap_open == gap_extend, the
word pass counts (score1 + mismatch >= 255) and the reference's score2 is the lower one (its lazy-F loop's early exit,
src/ssw.c:468-479); any other difference stops the generator.  At a scoring with gap_open == gap_extend the draw of the
classes r and l is repeated with the next seed until it holds none of the other kind (meta: "draw"), and at most 5 % of
a scoring's pairs may be left out.
"""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_second as fs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sw_second.npz")
SCORINGS = ((1, 5, 7, 2), (2, 2, 3, 1), (1, 16, 16, 1), (4, 6, 10, 1), (8, 16, 16, 16), (8, 0, 1, 1), (1, 1, 1, 1))
BASE = (1, 5, 7, 2)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
SHORT = (15, 16, 17, 24, 25, 30, 31, 32, 36, 64, 65, 100, 129, 150, 150, 250)


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def template(ladder, t):
    """Template t of a ladder in db order (u=1 fwd, u=1 rc, u=2 fwd, ...); max_units 0: the plain reference."""
    prefix, repeat, suffix, mu = ladder
    if mu == 0:
        return prefix
    s = prefix + repeat * (t // 2 + 1) + suffix
    return rc(s) if t % 2 else s


def plain(ref):
    return (ref, "A", "", 0)


def other_letter(rng, c):
    return rng.choice([b for b in "ACGT" if b != c])


def unlike(rng, n, avoid):
    """n letters that differ, position by position, from avoid (cycled): nothing of avoid aligns along them."""
    return "".join(other_letter(rng, avoid[k % len(avoid)]) for k in range(n))


def must(holds):
    """A check of an item's reference values: holds(values) is what the item is crafted for."""
    def check(v):
        assert holds(v), v
    return check


def ladder_item(rng):
    motif = fs.randseq(rng, rng.choice([2, 3, 4, 5, 6, 12]))
    n = rng.choice(SHORT)
    mu = -(-n // len(motif)) + rng.randint(0, 3)
    lad = (fs.randseq(rng, rng.randint(5, 30)), motif, fs.randseq(rng, rng.randint(5, 30)), mu)
    t = 2 * (rng.randint(max(1, mu // 3), mu) - 1) + rng.randint(0, 1)
    src = template(lad, t)
    L = min(n, len(src))
    at = rng.choice([0, len(src) - L, rng.randint(0, len(src) - L)])
    read = list(src[at:at + L])
    if rng.random() < 0.4 and L > 20:
        p, g = rng.randint(5, L - 5), rng.choice([1, 2, 3, 6])
        if rng.random() < 0.5:
            del read[p:p + g]
        else:
            read[p:p] = list(fs.randseq(rng, g))
    read = "".join(other_letter(rng, c) if rng.random() < 0.02 else "N" if rng.random() < 0.005 else c for c in read)
    return lad, t, read


def drawn(scoring, draw):
    rng = random.Random("sw_second {} {}".format("/".join(map(str, scoring)), draw))
    items = []
    for _ in range(30):
        ref, read = fs.make_pair(rng, SHORT)
        items.append(("r", plain(ref), 0, read, scoring, fs.mask_len_of(read)))
    for _ in range(30):
        lad, t, read = ladder_item(rng)
        items.append(("l", lad, t, read, scoring, fs.mask_len_of(read)))
    return items


def crafted(rng):
    """[(class, ladder, template, read, scoring, mask_len, check)]; check(values) asserts what the item is crafted for."""
    items = []

    def add(cls, ref, read, check=None, mask=None):
        items.append((cls, plain(ref), 0, read, BASE, fs.mask_len_of(read) if mask is None else mask, check))

    # p: padding rows
    for L in (15, 16, 17, 24, 25):
        for k in range(3):
            read = fs.randseq(rng, L)
            ref = fs.randseq(rng, rng.randint(0, 20)) + read + fs.randseq(rng, rng.randint(16, 30)) + read[k:L - k] + fs.randseq(rng, rng.randint(0, 20))
            add("p", ref, read)
    # the last row's value leaves the mask: the read's last `tail` letters again, ending `short` columns inside the mask,
    # then letters nothing aligns to.  Only the padding rows carry the tail's score to the first column that counts.
    # (maskLen = L here: with L / 2 the optimal path's own cell left of the mask always scores more than such a tail.)
    for L, tail, short in ((40, 17, 3), (41, 16, 2), (45, 20, 2), (57, 24, 5), (73, 30, 4), (90, 40, 1)):
        read = fs.randseq(rng, L)
        mask = L
        assert short < -L % 16
        between = mask - short - tail                       # letters that differ from the read's along the tail's diagonal
        ref = fs.randseq(rng, 12) + read + unlike(rng, between, read[L - tail - between:L - tail]) + read[L - tail:] + unlike(rng, 40, read)
        end1 = 12 + L - 1
        add("p", ref, read, must(lambda v, L=L, end1=end1, mask=mask, tail=tail: v == (L, end1, tail, end1 + mask + 1)), mask=mask)
    # b: the pass boundary.  The runner-up is the read's last maskLen (+ 1) letters again, right behind the read: it ends at
    # ref_end1 + maskLen (+ 1).  250 bp, word pass: that column counts.  249 bp, byte pass: it does not -- the path's own
    # cell left of the mask (as high, and first) is reported instead -- and one column further it does.
    for L in (249, 250):
        for extra in (0, 1):
            mask = L // 2
            tail = mask + extra
            read = fs.randseq(rng, L)
            while read[L - 1] == read[L - tail - 1]:          # (the tail's diagonal must not go on into the read)
                read = fs.randseq(rng, L)
            ref = fs.randseq(rng, 9) + read + read[L - tail:] + unlike(rng, 60, read)
            end1 = 9 + L - 1
            want = (tail, end1 + mask + extra) if (L == 250 or extra) else (L - mask - 1, end1 - mask - 1)
            add("b", ref, read, must(lambda v, L=L, end1=end1, want=want: v == (L, end1) + want))
    # m: mask edges
    for L in (30, 31, 32, 40, 64):
        read = fs.randseq(rng, L)
        mask = fs.mask_len_of(read)
        ref = unlike(rng, 25, read) + read + unlike(rng, 40, read)
        end1 = 25 + L - 1

        def check(v, L=L, end1=end1, mask=mask):            # the optimal path's own cell, one column outside the mask
            assert v[:2] == (L, end1), v
            if L - mask - 1 > 0:
                assert v[2:] == (L - mask - 1, end1 - mask - 1), v
        add("m", ref, read, check)
    read = fs.randseq(rng, 15)                                # ref_end1 - maskLen <= 0
    add("m", read + unlike(rng, 30, read) + read[:9] + unlike(rng, 6, read[9:]), read, must(lambda v: v == (15, 14, 9, 53)))
    read = fs.randseq(rng, 36)                                # ref_end1 + maskLen >= refLen
    add("m", unlike(rng, 30, read) + read + unlike(rng, 5, read), read, must(lambda v: v[1] == 65))
    add("m", unlike(rng, 30, read) + read, read, must(lambda v: v[1] == 65))
    read = fs.randseq(rng, 40)                                # equal maxima: 19 left (the path's own) and 19 right
    body = unlike(rng, 30, read) + read + unlike(rng, 30, read)
    add("m", body + read[:19] + unlike(rng, 10, read[19:]), read, must(lambda v: v[2:] == (19, 30 + 39 - 21)))
    add("m", body + read[:20] + unlike(rng, 10, read[20:]), read, must(lambda v: (v[2] == 20 and v[3] > 69)))
    read = fs.randseq(rng, 15)                                # nothing outside the mask
    add("m", read, read, must(lambda v: v == (15, 14, 0, 0)))
    read = fs.randseq(rng, 40)
    add("m", unlike(rng, 30, read) + read + unlike(rng, 30, read), read, must(lambda v: v[2:] == (0, -1)), mask=14)
    # c: the unit's row classes
    for L in (64, 65, 128, 129, 256, 257, 480, 481, 512, 513, 1024, 1025, 2047, 2048):
        motif = fs.randseq(rng, rng.choice([3, 5, 6]))
        cols = 4095 if L == 2047 else L + rng.randint(40, 200)
        ref = fs.randseq(rng, 20) + (motif * (cols // len(motif) + 1))[:cols - 40] + fs.randseq(rng, 20)
        at = rng.randint(0, len(ref) - L)
        read = "".join(other_letter(rng, c) if rng.random() < 0.02 else c for c in ref[at:at + L])
        add("c", ref, read, must(lambda v, L=L: v[0] > L // 2))
    return items


def main():
    rng = random.Random(20261019)
    items, checks = [], []
    for it in crafted(rng):
        items.append(it[:6])
        checks.append(it[6])
    draws = {}
    per_scoring = {}
    for scoring in SCORINGS:
        for draw in range(50):
            part = drawn(scoring, draw)
            pairs = [(template(lad, t), read) for _, lad, t, read, _, _ in part]
            ref, _ = fs.run_reference(pairs, scoring)
            mod = fs.run_model(pairs, scoring)
            bad = [k for k in range(len(part)) if ref[k] != mod[k] and not fs.excusable(scoring, ref[k], mod[k])]
            if not bad:
                break
            assert scoring[2] == scoring[3], ("the model differs from the reference", scoring, pairs[bad[0]], ref[bad[0]], mod[bad[0]])
        else:
            raise AssertionError("no draw without a difference of the other kind at {}".format(scoring))
        draws["/".join(map(str, scoring))] = draw
        items += part
        checks += [None] * len(part)
    kept, left_out, total, cpu_s = [], {}, {}, 0.0
    for scoring in SCORINGS:
        tag = "/".join(map(str, scoring))
        idx = [k for k, it in enumerate(items) if it[4] == scoring]
        pairs = [(template(items[k][1], items[k][2]), items[k][3]) for k in idx]
        masks = [items[k][5] for k in idx]
        ref, spent = fs.run_reference(pairs, scoring, masks)
        cpu_s += spent
        mod = fs.run_model(pairs, scoring, masks)
        total[tag], left_out[tag] = len(idx), 0
        for i, k in enumerate(idx):
            if ref[i] != mod[i]:
                assert fs.excusable(scoring, ref[i], mod[i]), ("the model differs from the reference", scoring, pairs[i], ref[i], mod[i])
                assert checks[k] is None
                left_out[tag] += 1
                continue
            if checks[k] is not None:
                checks[k](ref[i])
            kept.append(items[k] + (ref[i],))
        assert scoring[2] == scoring[3] or left_out[tag] == 0
        assert left_out[tag] <= 0.05 * total[tag], (tag, left_out, total)
    ladders = []
    for it in kept:
        if it[1] not in ladders:
            ladders.append(it[1])
    meta = {"generator": "tools/gen_golden_second.py: the reference's ssw_align (src/ssw.c compiled), flag 0, score_size 2",
            "scorings": ["/".join(map(str, s)) for s in SCORINGS], "ladders": [list(l) for l in ladders],
            "total": total, "kept": {t: total[t] - left_out[t] for t in total}, "left_out": left_out, "draw": draws,
            "classes": {c: sum(1 for it in kept if it[0] == c) for c in "rlpbmc"},
            "with_second": sum(1 for it in kept if it[6][2] > 0),
            "word_pass": sum(1 for it in kept if it[6][0] + it[4][1] >= 255),
            "reference_cpu_ms": round(cpu_s * 1e3, 2), "reference_cells": int(sum(len(it[3]) * len(template(it[1], it[2])) for it in kept))}
    print(json.dumps({k: v for k, v in meta.items() if k != "ladders"}, indent=1))
    reads = [it[3].encode() for it in kept]
    off = np.zeros(len(kept) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    np.savez_compressed(
        OUT, cls=np.array([it[0] for it in kept]), ladder=np.array([ladders.index(it[1]) for it in kept], np.int32),
        template=np.array([it[2] for it in kept], np.int32), reads=np.frombuffer(b"".join(reads), np.uint8), read_off=off,
        scoring=np.array([it[4] for it in kept], np.int32), mask_len=np.array([it[5] for it in kept], np.int32),
        expect=np.array([it[6] for it in kept], np.int32), meta=np.array(json.dumps(meta)))
    print("wrote {} ({} bytes, {} items)".format(OUT, os.path.getsize(OUT), len(kept)))


if __name__ == "__main__":
    main()
