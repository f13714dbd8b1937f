#!/usr/bin/env python3
"""Device time of the interrupted-tract scan (tredtract_scan, csrc/tract.hip) beside the perfect scan (tredscan_scan) on the
same letters in the same run -- the yardstick -- and beside the model on one core.

MB million letters over ACGT drawn with `seed`, in segments of 16 million: about every 10 000 letters a planted tract of a
random period 1 .. 6 made of two to four perfect stretches of 5 to 30 copies with one substituted unit's worth of letters
(1 .. p) between them, a stretch of 100 000 N, and one satellite of a million letters (period 5).  Both calls run with their
defaults (_lib.SCAN_MIN_COPIES; _lib.TRACT_SEED_COPIES and _lib.TRACT_MAX_GAP_DEFAULT: choices, not measurements).
get_timing's selectors give the device times (HIP events around a call's launches; the reads of a count between them are
inside): the median of REPEATS calls after a warm-up, and their range.  The wall time of a call adds the copy of the letters
to the device and of the records back (and, for the tracts, the merge of the periods' lists on the host).  `seeds` is what
the perfect scan counts with seed_copies in the place of min_copies: the entries of the tract unit's seed list.  A slice of
the first segment then goes through tests/tract_model.py on one core, and its records must be the call's.  Fixes no
target: one JSON line.

    python tools/tract_bench.py [MB] [seed] [REPEATS]        (on the GPU; 256, 1 and 5 by default)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEGMENT = 16_000_000
SLICE = 2_000_000
MOTIFS = {1: "A", 2: "AC", 3: "CAG", 4: "GATA", 5: "AACCT", 6: "AAGGCT"}


def synthetic(n, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    buf = letters[rng.integers(0, 4, n, dtype=np.uint8)]
    planted = 0
    for at in range(5000, n - 2000, 10000):
        p = int(rng.integers(1, 7))
        motif = np.frombuffer(MOTIFS[p].encode(), np.uint8)
        stretches = [p * int(rng.integers(5, 31)) for _ in range(int(rng.integers(2, 5)))]
        length = sum(stretches) + (len(stretches) - 1) * p
        tract = np.resize(motif, length).copy()
        x = 0
        for s in stretches[:-1]:
            x += s
            g = int(rng.integers(1, p + 1))
            tract[x:x + g] = letters[(np.searchsorted(letters, tract[x:x + g]) + 1) % 4]     # substituted: another letter
            x += p
        buf[at:at + length] = tract
        planted += 1
    if n >= 2 * SEGMENT:
        buf[SEGMENT + 3_000_000:SEGMENT + 4_000_000] = np.resize(np.frombuffer(b"AACCT", np.uint8), 1_000_000)
    if n >= 1_000_000:
        buf[700_000:800_000] = ord("N")
    return buf, planted


def median_range(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def main(argv):
    from tredparse_amd import _lib
    from tests import tract_model as tm
    mb = int(argv[0]) if len(argv) > 0 else 256
    seed = int(argv[1]) if len(argv) > 1 else 1
    repeats = int(argv[2]) if len(argv) > 2 else 5
    n = min(mb * 1_000_000, _lib.SCAN_MAX_LETTERS)
    t0 = time.perf_counter()
    buf, planted = synthetic(n, seed)
    off = np.asarray(list(range(0, n, SEGMENT)) + [n], np.int64)
    print("{} letters, {} planted tracts, made in {:.1f} s".format(n, planted, time.perf_counter() - t0), file=sys.stderr, flush=True)
    ctx = _lib.Context(0)
    cap = 1 << 20
    out = ctx.scan_tracts(buf, off, cap=cap)            # the warm-ups: the buffers are made here
    perfect = ctx.scan(buf, off, cap=cap)
    assert out[6] <= cap and perfect[4] <= cap, "more records than the bench has room for"
    seeds = ctx.scan(buf, off, _lib.TRACT_SEED_COPIES, cap=0)[4]

    def timed(call, kernel):
        ctx.reset_timing()
        t0 = time.perf_counter()
        call(buf, off, cap=cap)
        return ctx.get_timing(kernel)[1], (time.perf_counter() - t0) * 1e3

    tract_runs, scan_runs = [], []
    for _ in range(repeats):                            # by turns: what the device does in between is the same for both
        tract_runs.append(timed(ctx.scan_tracts, _lib.KERNEL_TRACT))
        scan_runs.append(timed(ctx.scan, _lib.KERNEL_SCAN))
    first = min(SLICE, int(off[1]))
    ours = ctx.scan_tracts(buf[:first], [0, first], cap=cap)
    ctx.close()
    t0 = time.perf_counter()
    model = tm.tracts_segment(buf[:first])
    numpy_ms = (time.perf_counter() - t0) * 1e3
    assert list(zip(*(x.tolist() for x in ours[1:6]))) == model, "the model and the kernel disagree on the slice"
    dev, wall = median_range([r[0] for r in tract_runs]), median_range([r[1] for r in tract_runs])
    sdev, swall = median_range([r[0] for r in scan_runs]), median_range([r[1] for r in scan_runs])
    print(json.dumps({"tool": "tools/tract_bench.py", "letters": n, "segments": len(off) - 1, "seed": seed, "repeats": repeats,
                      "planted": planted, "seeds": int(seeds), "seeds_per_letter": seeds / n,
                      "tracts": int(out[6]), "tracts_of_two_seeds_or_more": int((out[4] >= 2).sum()),
                      "most_seeds": int(out[4].max()) if out[6] else 0, "perfect_records": int(perfect[4]),
                      "tract_device_ms": dev, "tract_call_wall_ms": wall, "scan_device_ms": sdev, "scan_call_wall_ms": swall,
                      "tract_over_scan_device": dev["median"] / sdev["median"],
                      "tract_over_scan_call": wall["median"] / swall["median"],
                      "tract_letters_per_s_device": n / (dev["median"] * 1e-3),
                      "numpy_letters": first, "numpy_one_core_ms": numpy_ms,
                      "numpy_one_core_ms_scaled_to_all_letters": numpy_ms * n / first,
                      "numpy_over_device": numpy_ms * n / first / dev["median"]}))


if __name__ == "__main__":
    main(sys.argv[1:])
