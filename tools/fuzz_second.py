#!/usr/bin/env python3
"""Randomised parity of the second-best kernel (tredsecond_sw_second) against the compiled reference: N random
(reference, read) pairs -- random sequences and periodic ones, with substitutions, N and indels of 1-24 bases, a few of
them long (reads beyond 480 bp, references beyond 511 columns) -- are aligned by oracle/_ref/libssw.so (ssw_init(..., 2)
and ssw_align with flag 0 and Aligner.align's maskLen, loaded with ctypes; flag 0 ends before the reverse pass, so the
reference's CIGAR pass and its faults are never reached) and by the GPU; all four values (score1, ref_end1, score2,
ref_end2) must agree.  Without oracle/_ref the yardstick is tests/second_model (pinned to the reference by
tests/test_second_model.py).

Pair k is scored with scorings[k % len(scorings)].  With gap_open == gap_extend the reference's word pass can leave its
lazy-F loop early (src/ssw.c:468-479) and report a column maximum below the recurrence's.  A pair on which reference
and model differ while gap_open == gap_extend and the word pass counts (the full recurrence's score1 + mismatch >= 255)
is excluded and counted: as `excluded_word_pass_early_exit` when the reference's score2 is the lower one (the rule of
tools/gen_golden_second.py), as `excluded_word_pass_other` otherwise (a lower score1 or a later ref_end1 of the
reference moves its mask).  Any other difference between reference and model is reported as `model_differs`.

    python tools/fuzz_second.py N SEED [out.json]      (on the GPU)
"""
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
LIBSSW = os.path.join(ROOT, "oracle", "_ref", "libssw.so")
HAVE_REF = os.path.exists(LIBSSW)
DEFAULT_SCORINGS = ((1, 5, 7, 2), (2, 2, 3, 1), (1, 16, 16, 1), (4, 6, 10, 1), (8, 16, 16, 16), (8, 0, 1, 1))


class SAlign(C.Structure):          # s_align, ssw.h:42-52
    _fields_ = [("score1", C.c_uint16), ("score2", C.c_uint16), ("ref_begin1", C.c_int32), ("ref_end1", C.c_int32),
                ("read_begin1", C.c_int32), ("read_end1", C.c_int32), ("ref_end2", C.c_int32),
                ("cigar", C.POINTER(C.c_uint32)), ("cigarLen", C.c_int32)]


def mask_len_of(read):
    return len(read) // 2 if len(read) > 30 else 15          # ssw_wrap.py:198-201


def run_reference(pairs, scoring, masks=None):
    """[(score1, ref_end1, score2, ref_end2)] of the compiled reference for every (ref, read), and the CPU seconds of its
    ssw_init / ssw_align calls.  maskLen < 15 makes the reference write a line to stderr; it is let through."""
    match, mismatch, gap_open, gap_extend = scoring
    lib = C.CDLL(LIBSSW)
    lib.ssw_init.restype = C.c_void_p
    lib.ssw_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int8]
    lib.ssw_align.restype = C.POINTER(SAlign)
    lib.ssw_align.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint16, C.c_int32, C.c_int32]
    lib.init_destroy.argtypes = [C.c_void_p]
    lib.align_destroy.argtypes = [C.POINTER(SAlign)]
    mat = np.array([0 if 4 in (a, b) else match if a == b else -mismatch for a in range(5) for b in range(5)], np.int8)
    out, spent = [], 0.0
    for k, (ref, read) in enumerate(pairs):
        r = np.array([CODE.get(c, 4) for c in ref.upper()], np.int8)
        q = np.array([CODE.get(c, 4) for c in read.upper()], np.int8)
        mask = mask_len_of(read) if masks is None else int(masks[k])
        t0 = time.perf_counter()
        prof = lib.ssw_init(q.ctypes.data, len(q), mat.ctypes.data, 5, 2)
        al = lib.ssw_align(prof, r.ctypes.data, len(r), gap_open, gap_extend, 0, 0, 0, mask)
        spent += time.perf_counter() - t0
        a = al.contents
        out.append((int(a.score1), int(a.ref_end1), int(a.score2), int(a.ref_end2)))
        lib.align_destroy(al)
        lib.init_destroy(prof)
    return out, spent


def run_model(pairs, scoring, masks=None):
    from tests import second_model as sm
    return [sm.second(read, ref, scoring, mask_len_of(read) if masks is None else int(masks[k]))
            for k, (ref, read) in enumerate(pairs)]


def word_pass_equal_gaps(scoring, model_val):
    """Where the reference's own values may fall short of the recurrence's: gap_open == gap_extend and the word pass."""
    return scoring[2] == scoring[3] and model_val[0] + scoring[1] >= 255


def excusable(scoring, ref_val, model_val):
    """The one difference between reference and model a fixture may leave out: the word pass's early exit lowered score2."""
    return word_pass_equal_gaps(scoring, model_val) and ref_val[2] < model_val[2]


def randseq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def make_pair(rng, lengths=(15, 16, 17, 24, 25, 31, 36, 64, 65, 100, 128, 129, 150, 150, 250, 257, 480), max_ref=511):
    """(ref, read): half of the references periodic -- where a read inside the repeat scores almost as well one period
    further along -- and the reads drawn from them with indels, substitutions and N."""
    n = rng.choice(lengths)
    if rng.random() < 0.5:
        motif = randseq(rng, rng.choice([2, 3, 4, 5, 6, 12]))
        ref = (randseq(rng, rng.randint(5, 40)) + motif * ((n + rng.randint(0, 2 * n)) // len(motif) + 1) + randseq(rng, rng.randint(5, 40)))[:max_ref]
    else:
        ref = randseq(rng, min(max_ref, n + rng.randint(0, 2 * n + 60)))
    L = min(n, len(ref))
    at = rng.randint(0, len(ref) - L)
    read = list(ref[at:at + L])
    for _ in range(rng.choice([0, 0, 1, 1, 2, 3])):
        if len(read) < 4:
            break
        p, g = rng.randint(1, len(read) - 1), rng.choice([1, 2, 3, 3, 6, 12, 24])
        if rng.random() < 0.5:
            del read[p:p + g]
        else:
            read[p:p] = [rng.choice("ACGT") for _ in range(g)]
    read = [rng.choice("ACGT") if rng.random() < 0.02 else "N" if rng.random() < 0.005 else c for c in read][:max(lengths)]
    if rng.random() < 0.02:
        ref = "".join("N" if rng.random() < 0.01 else c for c in ref)
    return ref, "".join(read)


def make_long_pair(rng):
    return make_pair(rng, (481, 513, 700, 1024, 1025, 1500, 2048), 4095)


def gpu_second(ctx, pairs, scoring, masks=None):
    """The kernel's four values and statuses for (ref, read) pairs, each reference a plain one-template ladder."""
    from tredparse_amd import _lib
    refs = sorted({p[0] for p in pairs})
    lid = {r: i for i, r in enumerate(refs)}
    n = len(pairs)
    packed, woff, rlen = _lib.pack_reads([p[1] for p in pairs])
    mask = np.array([mask_len_of(p[1]) for p in pairs] if masks is None else masks, np.int32)
    out, status = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
    ctx.sw_secondary(packed, woff, rlen, n, np.array([lid[p[0]] for p in pairs], np.int32), np.zeros(n, np.int32), mask,
                     _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], 9, 0, 0, 0), out, status,
                     ladders=[(r, "A", "", 0) for r in refs])
    return out, status


def campaign(n=4000, seed=7, scorings=DEFAULT_SCORINGS, yardstick=None, long_share=0.02):
    """n pairs, pair k at scorings[k % len(scorings)].  yardstick: "reference" (oracle/_ref), "model", default: the
    reference when it is built."""
    from tredparse_amd import _lib
    yardstick = yardstick or ("reference" if HAVE_REF else "model")
    scorings = [tuple(s) for s in scorings]
    rng = random.Random(seed)
    pairs = [make_long_pair(rng) if rng.random() < long_share else make_pair(rng) for _ in range(n)]
    ctx = _lib.Context(0)
    mismatches, excluded, other, model_differs, compared, second_found, word_pass, cpu_s = [], 0, 0, 0, 0, 0, 0, 0.0
    for si, scoring in enumerate(scorings):
        ks = list(range(si, n, len(scorings)))
        part = [pairs[k] for k in ks]
        want = run_model(part, scoring)
        if yardstick == "reference":
            ref, spent = run_reference(part, scoring)
            cpu_s += spent
            for i in range(len(part)):
                if ref[i] != want[i]:
                    if word_pass_equal_gaps(scoring, want[i]):
                        excluded += excusable(scoring, ref[i], want[i])
                        other += not excusable(scoring, ref[i], want[i])
                        ks[i] = None
                    else:
                        model_differs += 1
            want = ref
        out, status = gpu_second(ctx, part, scoring)
        for i, k in enumerate(ks):
            if k is None:
                continue
            compared += 1
            second_found += want[i][2] > 0
            word_pass += want[i][0] + scoring[1] >= 255
            if status[i] != 0 or tuple(int(v) for v in out[i]) != tuple(want[i]):
                mismatches.append(k)
    launches, ms = ctx.get_timing(_lib.KERNEL_SECOND)
    res = {"tool": "tools/fuzz_second.py", "pairs": n, "seed": seed, "compared": compared, "excluded_word_pass_early_exit": excluded,
           "excluded_word_pass_other": other,
           "model_differs": model_differs, "mismatches": len(mismatches), "first_mismatches": sorted(mismatches)[:5],
           "with_second": int(second_found), "word_pass": int(word_pass), "long_pairs": sum(1 for p in pairs if len(p[1]) > 480 or len(p[0]) > 511),
           "calls": launches, "kernel_ms": ms, "reference_cpu_ms": cpu_s * 1e3, "library": _lib.version(),
           "scorings": ["/".join(map(str, s)) for s in scorings], "yardstick": yardstick}
    ctx.close()
    return res


def main():
    n, seed = int(sys.argv[1]), int(sys.argv[2])
    out = campaign(n, seed)
    print(json.dumps(out))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fp:
            json.dump(out, fp, indent=1)
    return 1 if out["mismatches"] or out["model_differs"] else 0


if __name__ == "__main__":
    sys.exit(main())
