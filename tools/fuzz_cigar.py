#!/usr/bin/env python3
"""Randomised parity of the CIGAR kernel (tredcigar_sw_cigar) against the compiled reference: N random (reference,
read) pairs -- random sequences and periodic ones, with substitutions, N and indels of 1-24 bases -- are aligned by
oracle/_ref/libssw.so (ssw_init / ssw_align with flag 1, exactly Aligner.align, src/ssw_wrap.py:177-227; loaded with
ctypes) in child processes that report pair by pair, so that a fault of the reference's CIGAR pass loses one pair and
not the campaign; the GPU traces the same pairs from the reference's own fields.  A pair is excluded (and counted) when
the reference faulted or when its operations do not consume exactly the aligned bases.

Pair k is scored with scorings[k % len(scorings)]; the default is 1/5/7/2 alone.  Without oracle/_ref the yardstick is
tests/cigar_model.py (pinned to the reference by tests/test_cigar_model.py) on the fields of the SW kernel, and the reads
are drawn up to 250 bp so that the Python model stays fast.  `wide_tier` counts the pairs the model predicts for the
wide kernel: by all the bands it ran where the model is the yardstick, by the first band alone (a lower bound) where
the reference is.

    python tools/fuzz_cigar.py N SEED [out.json]      (on the GPU, with oracle/_ref built)
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


class SAlign(C.Structure):          # s_align, ssw.h:42-52
    _fields_ = [("score1", C.c_uint16), ("score2", C.c_uint16), ("ref_begin1", C.c_int32), ("ref_end1", C.c_int32),
                ("read_begin1", C.c_int32), ("read_end1", C.c_int32), ("ref_end2", C.c_int32),
                ("cigar", C.POINTER(C.c_uint32)), ("cigarLen", C.c_int32)]


DEFAULT_SCORINGS = ((1, 5, 7, 2),)
HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libssw.so"))


def worker(scoring):
    match, mismatch, gap_open, gap_extend = scoring
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libssw.so"))
    lib.ssw_init.restype = C.c_void_p
    lib.ssw_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int8]
    lib.ssw_align.restype = C.POINTER(SAlign)
    lib.ssw_align.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint16, C.c_int32, C.c_int32]
    mat = np.array([0 if 4 in (a, b) else match if a == b else -mismatch for a in range(5) for b in range(5)], np.int8)
    for line in sys.stdin:
        ref, read = json.loads(line)
        r = np.array([CODE.get(c, 4) for c in ref], np.int8)
        q = np.array([CODE.get(c, 4) for c in read], np.int8)
        prof = lib.ssw_init(q.ctypes.data, len(q), mat.ctypes.data, 5, 2)
        al = lib.ssw_align(prof, r.ctypes.data, len(r), gap_open, gap_extend, 1, 0, 0, len(q) // 2 if len(q) > 30 else 15).contents
        out = {"fields": [al.score1, al.ref_begin1, al.ref_end1, al.read_begin1, al.read_end1],
               "ops": [int(al.cigar[k]) for k in range(al.cigarLen)]}
        sys.stdout.write(json.dumps(out) + "\n")
        sys.stdout.flush()


def run_reference(pairs, scoring=DEFAULT_SCORINGS[0], chunk=500):
    out, k = [None] * len(pairs), 0
    while k < len(pairs):
        part = pairs[k:k + chunk]
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "/".join(map(str, scoring))], input="".join(json.dumps(x) + "\n" for x in part),
                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, universal_newlines=True)
        lines = [l for l in p.stdout.split("\n") if l.endswith("}")]
        for i, l in enumerate(lines):
            out[k + i] = json.loads(l)
        k += len(lines) + (0 if len(lines) == len(part) else 1)       # the pair the child died on is skipped
    return out


def make_pair(rng, lengths=(36, 100, 150, 150, 250, 480)):
    n = rng.choice(lengths)
    if rng.random() < 0.5:
        motif = "".join(rng.choice("ACGT") for _ in range(rng.choice([3, 4, 5, 6, 12])))
        flank = lambda: "".join(rng.choice("ACGT") for _ in range(rng.randint(10, 30)))
        ref = (flank() + motif * (n // len(motif)) + flank())[:511]
    else:
        ref = "".join(rng.choice("ACGT") for _ in range(min(511, n + rng.randint(0, 60))))
    L = min(n, len(ref))
    at = rng.randint(0, len(ref) - L)
    read = list(ref[at:at + L])
    for _ in range(rng.choice([0, 0, 1, 1, 2, 3])):
        p, g = rng.randint(1, len(read) - 1), rng.choice([1, 2, 3, 3, 6, 12, 24])
        if rng.random() < 0.5:
            del read[p:p + g]
        else:
            read[p:p] = [rng.choice("ACGT") for _ in range(g)]
    read = [rng.choice("ACGT") if rng.random() < 0.01 else "N" if rng.random() < 0.005 else c for c in read][:max(lengths)]
    return ref, "".join(read)


def run_model(ctx, pairs, scoring):
    """The yardstick without the compiled reference: the SW kernel's fields, tests/cigar_model.py's operations and bands."""
    from tests import cigar_model as cm
    from tredparse_amd import _lib
    refs = sorted({p[0] for p in pairs})
    lid = {r: i for i, r in enumerate(refs)}
    n = len(pairs)
    ctx.set_ladders([(r, "A", "", 0) for r in refs])
    packed, woff, rlen = _lib.pack_reads([p[1] for p in pairs])
    tag, h, sc = np.zeros(n, np.uint8), np.zeros(n, np.int16), np.zeros(n, np.int16)
    dump = np.zeros((n, 1, 6), np.int16)
    p = _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], 9, 0, 0, 0)
    ctx.sw_classify(_lib.MEM_HOST, packed, woff, rlen, n, np.arange(n + 1, dtype=np.int32),
                    np.array([lid[p_[0]] for p_ in pairs], np.int32), n, p, tag, h, sc, dump, 1)
    out = []
    for (ref, read), rec in zip(pairs, dump[:, 0]):
        fields = [int(v) for v in rec[:5]]
        st, ops, passes = cm.passes_of(ref, read, fields, *scoring)
        out.append({"fields": fields, "ops": ops if st == cm.OK else [], "bands": [b for b, _ in passes]})
    return out


def campaign(n=4000, seed=7, scorings=DEFAULT_SCORINGS, yardstick=None):
    """n pairs, pair k at scorings[k % len(scorings)].  yardstick: "reference" (oracle/_ref), "model", default: the
    reference when it is built."""
    from tests import cigar_model as cm
    from tredparse_amd import _lib
    yardstick = yardstick or ("reference" if HAVE_REF else "model")
    scorings = [tuple(s) for s in scorings]
    rng = random.Random(seed)
    pairs = [make_pair(rng) if yardstick == "reference" else make_pair(rng, (36, 100, 150, 150, 250)) for _ in range(n)]
    ctx = _lib.Context(0)
    res = [None] * n
    for si, scoring in enumerate(scorings):
        ks = list(range(si, n, len(scorings)))
        part = [pairs[k] for k in ks]
        out = run_reference(part, scoring) if yardstick == "reference" else run_model(ctx, part, scoring)
        for k, r in zip(ks, out):
            res[k] = r
    keep, faulted, inconsistent = [], 0, 0
    for k, r in enumerate(res):
        if r is None:
            faulted += 1
            continue
        f, ops = r["fields"], r["ops"]
        q = sum(v >> 4 for v in ops if v & 15 in (0, 1))
        t = sum(v >> 4 for v in ops if v & 15 in (0, 2))
        if not ops or q != f[4] - f[3] + 1 or t != f[2] - f[1] + 1:
            inconsistent += 1
            continue
        keep.append(k)
    mismatches, wide = [], 0
    cap = max(max(len(res[k]["ops"]) for k in keep), 1)
    for si, scoring in enumerate(scorings):
        sub = [k for k in keep if k % len(scorings) == si]
        if not sub:
            continue
        refs = sorted({pairs[k][0] for k in sub})
        lid = {r: i for i, r in enumerate(refs)}
        ladders = [(r, "A", "", 0) for r in refs]
        m = len(sub)
        packed, woff, rlen = _lib.pack_reads([pairs[k][1] for k in sub])
        ops, n_ops, status = np.zeros((m, cap), np.uint32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        ctx.sw_cigar(_lib.MEM_HOST, packed, woff, rlen, m, np.array([lid[pairs[k][0]] for k in sub], np.int32), np.zeros(m, np.int32),
                     np.array([res[k]["fields"] for k in sub], np.int16), _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], 9, 0, 0, 0),
                     cap, ops, n_ops, status, ladders=ladders)
        mismatches += [k for i, k in enumerate(sub) if status[i] != 0 or list(ops[i, :n_ops[i]]) != res[k]["ops"]]
        for k in sub:
            f = res[k]["fields"]
            wide += cm.is_wide(res[k].get("bands") or [abs((f[2] - f[1]) - (f[4] - f[3])) + 1], f[4] - f[3] + 1)
    launches, ms = ctx.get_timing(_lib.KERNEL_CIGAR)
    out = {"tool": "tools/fuzz_cigar.py", "pairs": n, "seed": seed, "compared": len(keep), "reference_faulted": faulted,
           "reference_inconsistent": inconsistent, "mismatches": len(mismatches), "first_mismatches": sorted(mismatches)[:5],
           "with_gap": sum(1 for k in keep if any(v & 15 for v in res[k]["ops"])),
           "more_than_3_ops": sum(1 for k in keep if len(res[k]["ops"]) > 3), "max_ops": cap, "kernel_ms": ms,
           "library": _lib.version(), "scorings": ["/".join(map(str, s)) for s in scorings], "yardstick": yardstick,
           "wide_tier": int(wide)}
    ctx.close()
    return out


def main():
    n, seed = int(sys.argv[1]), int(sys.argv[2])
    out = campaign(n, seed)
    print(json.dumps(out))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fp:
            json.dump(out, fp, indent=1)
    return 1 if out["mismatches"] else 0


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(tuple(int(v) for v in sys.argv[sys.argv.index("--worker") + 1].split("/")))
    else:
        sys.exit(main())
