#!/usr/bin/env python3
"""Device time of the CIGAR kernel on the headline read set: bench.py's config3 reads (30x, 150 bp, 30 loci) are
classified with the dump, the winning row of every tagged read (highest score, first in db order = fewest units) is
traced by one sw_cigar call, and tredgpu_get_timing's selectors give the time of both steps on the same reads.

    python tools/cigar_bench.py [SAMPLES [REPEATS [out.json]]]      (on the GPU)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 16
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
    # the winner of a tagged read: the highest score among its tagged rows, the first of them in db order
    key = np.where(dump[:, :, 5] > 0, dump[:, :, 0].astype(np.int32), -1)
    win = key.argmax(axis=1)
    items = np.nonzero(tag != _lib.TAG_NONE)[0]
    agree = int(((key[items, win[items]] == sc[items]) & (win[items] // 2 + 1 == h[items])).sum())      # with out_score / out_h
    m = len(items)
    read_ladder = np.repeat(b.unit_ladder, np.diff(b.unit_read_off)).astype(np.int32)
    # the items' reads, packed again in item order (sw_cigar's item k is read k)
    words = [b.packed[b.read_off[k]:b.read_off[k + 1]] for k in items]
    packed = np.concatenate(words)
    woff = np.zeros(m + 1, np.int64)
    woff[1:] = np.cumsum([len(w) for w in words])
    rlen = np.ascontiguousarray(b.read_len[items])
    fields = np.ascontiguousarray(dump[items, win[items], :5])
    cap = 32
    ops, n_ops, status = np.zeros((m, cap), np.uint32), np.zeros(m, np.int32), np.zeros(m, np.int32)

    def cigar():
        ctx.sw_cigar(_lib.MEM_HOST, packed, woff, rlen, m, np.ascontiguousarray(read_ladder[items]), win[items].astype(np.int32),
                     fields, params, cap, ops, n_ops, status)

    def classify():
        ctx.sw_classify(_lib.MEM_HOST, b.packed, b.read_off, b.read_len, n, b.unit_read_off, b.unit_ladder, g, params, tag, h, sc)

    cigar()
    classify()
    ctx.reset_timing()
    for _ in range(repeats):
        cigar()
        classify()
    c_n, c_ms = ctx.get_timing(_lib.KERNEL_CIGAR)
    s_n, s_ms = ctx.get_timing(_lib.KERNEL_SW)
    c_ms, s_ms = c_ms / repeats, s_ms / repeats
    out = {"tool": "tools/cigar_bench.py", "samples": samples, "units": g, "reads": int(n), "traced": int(m), "winner_agrees_with_tag_and_h": agree,
           "status_counts": {int(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))},
           "with_gap": int(((ops & 15) != 0).any(axis=1).sum()), "max_ops": int(n_ops.max()),
           "cigar_launches_per_call": c_n / repeats, "cigar_ms_per_call": c_ms, "sw_ms_per_call": s_ms,
           "cigar_s_per_million_traced": c_ms / m * 1e3, "cigar_share_of_sw": c_ms / s_ms, "repeats": repeats,
           "library": _lib.version()}
    ctx.close()
    print(json.dumps(out))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fp:
            json.dump(out, fp, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
