#!/usr/bin/env python3
"""Device time of the tandem-repeat scan (tredscan_scan, csrc/scan.hip) beside the numpy model on one core.

MB million letters over ACGT drawn with `seed`, in segments of 16 million: a planted tract of a random period 1 .. 6 and 5 to
60 copies about every 10 000 letters, one satellite of a million letters (period 5) in the second segment, and a stretch
of 100 000 N.  get_timing's selector gives the device time (HIP events around the call's five launches; the read of the
records' total between the count and the write is inside): the median of REPEATS calls after a warm-up, and their range.
The wall time of a call adds the copy of the letters to the device and of the records back.  The kernels read every
letter three times (summary, count, write); `input_GB_per_s` is letters per device second, `read_GB_per_s` three times
that, to be held against the HBM rate of the device.  The first segment then goes through tests/scan_model.py on one
core, and its records must be the call's.  Fixes no target: one JSON line.

    python tools/scan_bench.py [MB] [seed] [REPEATS]        (on the GPU; 256, 1 and 5 by default)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEGMENT = 16_000_000
MOTIFS = {1: "A", 2: "AC", 3: "CAG", 4: "GATA", 5: "AACCT", 6: "AAGGCT"}


def synthetic(n, seed):
    rng = np.random.default_rng(seed)
    buf = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    planted = 0
    for at in range(5000, n - 1000, 10000):
        p = int(rng.integers(1, 7))
        length = p * int(rng.integers(5, 61)) + int(rng.integers(0, p))
        buf[at:at + length] = np.resize(np.frombuffer(MOTIFS[p].encode(), np.uint8), length)
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
    from tests import scan_model as sm
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
    out = ctx.scan(buf, off, cap=cap)                   # the warm-up: the buffers are made here
    total = out[4]
    assert total <= cap, "more records than the bench has room for"

    def timed():
        ctx.reset_timing()
        t0 = time.perf_counter()
        ctx.scan(buf, off, cap=cap)
        return ctx.get_timing(_lib.KERNEL_SCAN)[1], (time.perf_counter() - t0) * 1e3

    runs = [timed() for _ in range(repeats)]
    ctx.close()
    first = int(off[1])
    t0 = time.perf_counter()
    model = sm.scan_segment(buf[:first])
    numpy_ms = (time.perf_counter() - t0) * 1e3
    k = int(np.searchsorted(out[0], 1))
    got = list(zip(out[1][:k].tolist(), out[2][:k].tolist(), out[3][:k].tolist()))
    assert got == model, "the model and the kernel disagree on the first segment"
    dev, wall = median_range([r[0] for r in runs]), median_range([r[1] for r in runs])
    rate = n / (dev["median"] * 1e-3)
    print(json.dumps({"tool": "tools/scan_bench.py", "letters": n, "segments": len(off) - 1, "seed": seed, "repeats": repeats,
                      "planted": planted, "records": int(total), "longest_record": int(out[2].max()) if total else 0,
                      "device_ms": dev, "call_wall_ms": wall, "letters_per_s_device": rate, "input_GB_per_s": rate / 1e9,
                      "read_GB_per_s": 3 * rate / 1e9, "letters_per_s_call": n / (wall["median"] * 1e-3),
                      "numpy_letters": first, "numpy_one_core_ms": numpy_ms,
                      "numpy_one_core_ms_scaled_to_all_letters": numpy_ms * n / first,
                      "numpy_over_device": numpy_ms * n / first / dev["median"]}))


if __name__ == "__main__":
    main(sys.argv[1:])
