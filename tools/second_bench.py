#!/usr/bin/env python3
"""Device time of the second-best kernel on the headline read set: bench.py's config3 reads (30x, 150 bp, 30 loci) are
classified with the dump, the winning row of every tagged read (highest score, first in db order = fewest units) goes
through one sw_secondary call with Aligner.align's maskLen, and get_timing's selectors give the time of both steps on the
same reads: the median of REPEATS calls after a warm-up, and their range.

    python tools/second_bench.py [SAMPLES [REPEATS [out.json]]]      (on the GPU)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    from tredparse_amd import synth
    loci = [l for l in synth.load_loci() if l["name"] not in ("FXTAS", "AR")]      # the 30 loci with distinct coordinates
    b = synth.build_batch(20240229, loci, samples, synth.SynthParams(), workers=min(16, len(loci)))   # before the GPU is touched
    from tredparse_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_ladders(b.ladders)
    n, g = b.n_reads, b.n_units
    nt = max(2 * l[3] for l in b.ladders)
    params = _lib.default_sw_params(max_read_len=b.readlen)
    tag, h, sc = np.zeros(n, np.uint8), np.zeros(n, np.int16), np.zeros(n, np.int16)
    dump = np.zeros((n, nt, 6), np.int16)
    ctx.sw_classify(_lib.MEM_HOST, b.packed, b.read_off, b.read_len, n, b.unit_read_off, b.unit_ladder, g, params, tag, h, sc, dump, nt)
    key = np.where(dump[:, :, 5] > 0, dump[:, :, 0].astype(np.int32), -1)
    win = key.argmax(axis=1)
    items = np.nonzero(tag != _lib.TAG_NONE)[0]
    m = len(items)
    read_ladder = np.repeat(b.unit_ladder, np.diff(b.unit_read_off)).astype(np.int32)
    words = [b.packed[b.read_off[k]:b.read_off[k + 1]] for k in items]
    packed = np.concatenate(words)
    woff = np.zeros(m + 1, np.int64)
    woff[1:] = np.cumsum([len(w) for w in words])
    rlen = np.ascontiguousarray(b.read_len[items])
    mask = np.where(rlen > 30, rlen // 2, 15).astype(np.int32)
    lad, tpl = np.ascontiguousarray(read_ladder[items]), win[items].astype(np.int32)
    fields = dump[items, win[items]]
    out, status = np.zeros((m, 4), np.int32), np.zeros(m, np.int32)

    def second():
        ctx.sw_secondary(packed, woff, rlen, m, lad, tpl, mask, params, out, status)

    def classify():
        ctx.sw_classify(_lib.MEM_HOST, b.packed, b.read_off, b.read_len, n, b.unit_read_off, b.unit_ladder, g, params, tag, h, sc)

    def timed(call, which):
        ctx.reset_timing()
        call()
        return ctx.get_timing(which)[1]

    second()
    classify()
    t2 = sorted(timed(second, _lib.KERNEL_SECOND) for _ in range(repeats))
    t1 = sorted(timed(classify, _lib.KERNEL_SW) for _ in range(repeats))
    cols = np.array([ctx._template_len(b.ladders[l]) for l in range(len(b.ladders))])
    units = np.array([l[3] for l in b.ladders])
    period = np.array([len(l[1]) for l in b.ladders])
    tlen = cols[lad] - (units[lad] - (tpl // 2 + 1)) * period[lad]
    res = {"tool": "tools/second_bench.py", "samples": samples, "units": g, "reads": int(n), "items": int(m),
           "status_counts": {int(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))},
           "score1_and_ref_end1_agree_with_the_dump": int(((out[:, 0] == fields[:, 0]) & (out[:, 1] == fields[:, 2])).sum()),
           "with_second": int((out[:, 2] > 0).sum()), "median_score1_minus_score2": float(np.median(out[:, 0] - out[:, 2])),
           "mean_template_columns": float(tlen.mean()),
           "second_ms_per_call": {"median": t2[len(t2) // 2], "min": t2[0], "max": t2[-1]},
           "sw_ms_per_call": {"median": t1[len(t1) // 2], "min": t1[0], "max": t1[-1]},
           "second_ms_per_million_items": t2[len(t2) // 2] / m * 1e6, "sw_ms_per_million_reads": t1[len(t1) // 2] / n * 1e6,
           "second_share_of_sw": t2[len(t2) // 2] / t1[len(t1) // 2], "repeats": repeats, "library": _lib.version()}
    ctx.close()
    print(json.dumps(res))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fp:
            json.dump(res, fp, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
