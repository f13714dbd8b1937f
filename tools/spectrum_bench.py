#!/usr/bin/env python3
"""Device time of the spectrum kernel on the headline read set, beside numpy on one core: bench.py's config3 reads (30x,
150 bp, 30 loci) are classified with the dump, the winning row of every FULL, PREF, POST and REPT read goes through one
sw_cigar call, and the items -- per unit one group per FULL h, one for the partial and one for the in-repeat reads, as
Engine.spectrum forms them; ULD's dodecamer left out -- through one unit_spectrum call.  get_timing's selector gives the
device time (HIP events around the call's two launches): the median of REPEATS calls after a warm-up, and their range; the
clocks are read (rocm-smi, nothing is set) before and after.  The same items then go through a numpy model on one core,
whose tables must equal the kernel's.

    python tools/spectrum_bench.py [SAMPLES [REPEATS [out.json]]]                       (on the GPU)

Then, in child processes:
    one call on a pure tract and on random words (256 groups of 1 024 items of 48 units): what the adds of a whole
    wavefront to ONE bin cost beside adds to 48 different ones
    --parent-tree DIR     `pileup_bench.py 128 15` of a built checkout of the commit before (its own package and library)
                          and of this one, alternated three times: what sharing the operation decoding cost the pileup
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BINS, STRIDE = 4096, 4100


def numpy_spectrum(codes, P, p, S, motif, tpl, fields, ops, n_ops, group, n_groups):
    """out_spectrum and out_item of tredpileup_unit_spectrum for accepted items (codes: uint8 [m][L] base codes of the reads;
    P, p, S, motif: the items' prefix, period and suffix lengths and the code of their repeat)."""
    m, cap = ops.shape
    ln, code = (ops >> 4).astype(np.int64), (ops & 15).astype(np.int64)
    live = np.arange(cap)[None, :] < n_ops[:, None]
    ln = np.where(live, ln, 0)
    on_ref, on_read = np.where(code != 1, ln, 0), np.where(code != 2, ln, 0)
    r0 = fields[:, 1].astype(np.int64)[:, None] + np.cumsum(on_ref, axis=1) - on_ref       # where every operation begins
    q0 = fields[:, 3].astype(np.int64)[:, None] + np.cumsum(on_read, axis=1) - on_read
    h, strand = tpl // 2 + 1, tpl & 1
    T = P + p * h + S
    spec, per_item = np.zeros(n_groups * STRIDE, np.int64), np.zeros((m, 3), np.int64)
    # touched: the span in forward columns, cut to the tract
    rb, re_ = fields[:, 1].astype(np.int64), fields[:, 2].astype(np.int64)
    lo, hi = np.maximum(np.where(strand == 1, T - 1 - re_, rb), P), np.minimum(np.where(strand == 1, T - 1 - rb, re_), P + p * h - 1)
    per_item[:, 2] = np.where(lo <= hi, (hi - P) // p - (lo - P) // p + 1, 0)
    # the units whole inside one M operation
    item = np.repeat(np.arange(m), cap).reshape(m, cap)
    sel = live & (code == 0)
    it, r, q, n = item[sel], r0[sel], q0[sel], ln[sel]
    fa = np.where(strand[it] == 1, T[it] - r - n, r)
    fb = fa + n
    k_lo = (np.maximum(fa, P[it]) - P[it] + p[it] - 1) // p[it]
    k_hi = np.where(fb > P[it], np.minimum(h[it], (fb - P[it]) // p[it]), 0)
    cnt = np.maximum(k_hi - k_lo, 0)
    u_it, u_r, u_q = np.repeat(it, cnt), np.repeat(r, cnt), np.repeat(q, cnt)
    k = np.repeat(k_lo, cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    word, has_n = np.zeros(len(k), np.int64), np.zeros(len(k), bool)
    rev = strand[u_it] == 1
    for i in range(int(p.max()) if m else 0):
        on = i < p[u_it]
        f = P[u_it] + p[u_it] * k + i
        c = np.where(rev, T[u_it] - 1 - f, f)
        x = codes[u_it, np.where(on, u_q + c - u_r, 0)].astype(np.int64)
        has_n |= on & (x > 3)
        word = np.where(on, word * 4 + (np.where(rev, 3 - x, x) & 3), word)
    g = group[u_it]
    np.add.at(spec, g[~has_n] * STRIDE + word[~has_n], 1)
    np.add.at(spec, g * STRIDE + BINS, 1)
    np.add.at(spec, g[has_n] * STRIDE + BINS + 1, 1)
    np.add.at(spec, group * STRIDE + BINS + 2, per_item[:, 2])
    np.add.at(spec, group * STRIDE + BINS + 3, 1)
    per_item[:, 0] = np.bincount(u_it[~has_n], minlength=m)
    per_item[:, 1] = np.bincount(u_it[~has_n & (word == motif[u_it])], minlength=m)
    return spec.reshape(n_groups, STRIDE), per_item


def clocks():
    """What rocm-smi shows of the clocks right now (read only); None where the tool is missing."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=60).stdout
        card = sorted(json.loads(out).items())[0][1]
        return {k: v for k, v in card.items() if "sclk" in k or "mclk" in k or "fclk" in k}
    except Exception:
        return None


def median_range(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def word_case(repeats):
    """Child: device time of one call on a pure tract and on random words (256 groups of 1 024 items of 48 CAG units each,
    12.6 M words: one workgroup per CU, so the adds and not the rows' stores are what is timed)."""
    from tredparse_amd import _lib
    rng = np.random.default_rng(5)
    lad = [("ACGTTGCATGACGTTGCA", "CAG", "TTGCAATTGCAATTGCAA", 50)]
    n_groups, per, units = 256, 1024, 48
    m = n_groups * per
    out = {}
    ctx = _lib.Context(0)
    for name in ("pure", "random"):
        tract = np.tile(np.array([1, 0, 2], np.uint8), (m, units)) if name == "pure" else rng.integers(0, 4, (m, 3 * units)).astype(np.uint8)
        packed, woff, rlen = _lib.pack_codes(tract)
        z = np.zeros(m, np.int32)
        fields = np.zeros((m, 5), np.int16)
        fields[:, 1], fields[:, 2], fields[:, 4] = 18, 18 + 3 * units - 1, 3 * units - 1
        ops = np.full((m, 1), (3 * units) << 4, np.uint32)
        group = np.ascontiguousarray(np.repeat(np.arange(n_groups), per), np.int32)
        spec, per_item, status = np.zeros((n_groups, STRIDE), np.int32), np.zeros((m, 3), np.int32), np.zeros(m, np.int32)
        call = lambda: ctx.unit_spectrum(packed, woff, rlen, m, z, np.full(m, 2 * (units - 1), np.int32), fields, ops, 1,
                                         np.ones(m, np.int32), group, n_groups, np.zeros(n_groups, np.int32), spec, per_item, status,
                                         ladders=lad)
        call()
        assert not status.any() and spec[:, BINS].sum() == m * units and (name != "pure" or spec[:, 1 * 16 + 2].sum() == m * units)
        dev = []
        for _ in range(repeats):
            ctx.reset_timing()
            call()
            dev.append(ctx.get_timing(_lib.KERNEL_PILEUP)[1])
        out[name] = median_range(dev)
    ctx.close()
    print(json.dumps(out))
    return 0


def child(args):
    run = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=900)
    if run.returncode:
        sys.stderr.write(run.stderr[-2000:])
        raise SystemExit("{} failed ({})".format(args[0], run.returncode))
    out = run.stdout
    sys.stderr.write("{}: done\n".format(args[0]))
    return json.loads(out.strip().split("\n")[-1])


def main():
    argv = list(sys.argv[1:])
    if argv[:1] == ["--word-case"]:
        return word_case(int(argv[1]))
    opt = {}
    for flag in ("--parent-tree",):
        if flag in argv:
            k = argv.index(flag)
            opt[flag] = argv[k + 1]
            del argv[k:k + 2]
    samples = int(argv[0]) if len(argv) > 0 else 64
    repeats = int(argv[1]) if len(argv) > 1 else 5
    here = os.path.abspath(__file__)
    from tredparse_amd import synth
    loci = [l for l in synth.load_loci() if l["name"] not in ("FXTAS", "AR")]      # the 30 loci with distinct coordinates
    b = synth.build_batch(20240229, loci, samples, synth.SynthParams(), workers=min(16, len(loci)))   # before the GPU is touched
    from tredparse_amd import _lib
    before = clocks()
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
    period_of = np.array([len(l[1]) for l in b.ladders])
    unit_all = np.searchsorted(b.unit_read_off, np.arange(n), side="right") - 1
    classes = np.isin(tag, (_lib.TAG_FULL, _lib.TAG_PREF, _lib.TAG_POST, _lib.TAG_REPT))
    items = np.nonzero(classes & (period_of[b.unit_ladder[unit_all]] <= _lib.SPECTRUM_MAX_PERIOD))[0]
    m = len(items)
    unit_of = unit_all[items]
    words = [b.packed[b.read_off[k]:b.read_off[k + 1]] for k in items]
    packed = np.concatenate(words)
    woff = np.zeros(m + 1, np.int64)
    woff[1:] = np.cumsum([len(w) for w in words])
    rlen = np.ascontiguousarray(b.read_len[items])
    lad, tpl = np.ascontiguousarray(b.unit_ladder[unit_of].astype(np.int32)), np.ascontiguousarray(win[items].astype(np.int32))
    fields = np.ascontiguousarray(dump[items, win[items], :5])
    cap = 32
    while True:
        ops, n_ops, status = np.zeros((m, cap), np.uint32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        ctx.sw_cigar(_lib.MEM_HOST, packed, woff, rlen, m, lad, tpl, fields, params, cap, ops, n_ops, status)
        if not (status == _lib.CIGAR_OVERFLOW).any():
            break
        cap = int(n_ops.max())
    assert not status.any(), "sw_cigar refused an item"
    # per unit one group per FULL h, one for PREF / POST (-1) and one for REPT (-2), as Engine.spectrum forms them
    t = tag[items]
    cls = np.where(t == _lib.TAG_FULL, tpl // 2 + 1, np.where(t == _lib.TAG_REPT, -2, -1))
    pairs, group = np.unique(np.stack([unit_of, cls], axis=1), axis=0, return_inverse=True)
    group = np.ascontiguousarray(group.reshape(-1).astype(np.int32))
    n_groups = len(pairs)
    group_ladder = np.ascontiguousarray(b.unit_ladder[pairs[:, 0]].astype(np.int32))
    spec, per_item, pstatus = np.zeros((n_groups, STRIDE), np.int32), np.zeros((m, 3), np.int32), np.zeros(m, np.int32)

    def spectrum():
        ctx.unit_spectrum(packed, woff, rlen, m, lad, tpl, fields, ops, cap, n_ops, group, n_groups, group_ladder, spec, per_item, pstatus)

    def timed(call, which):
        ctx.reset_timing()
        t0 = time.perf_counter()
        call()
        return ctx.get_timing(which)[1], (time.perf_counter() - t0) * 1e3

    spectrum()
    assert not pstatus.any(), "unit_spectrum refused an item"
    runs = [timed(spectrum, _lib.KERNEL_PILEUP) for _ in range(repeats)]
    after = clocks()
    dev, wall = median_range([r[0] for r in runs]), median_range([r[1] for r in runs])

    P = np.array([len(l[0]) for l in b.ladders])[lad]
    S = np.array([len(l[2]) for l in b.ladders])[lad]
    p = period_of[lad]
    code_of = lambda w: sum("ACGT".index(c) << (2 * (len(w) - 1 - i)) for i, c in enumerate(w)) if set(w) <= set("ACGT") else -1
    motif = np.array([code_of(l[1].upper()) for l in b.ladders])[lad]           # (-1: a repeat with an N, which no word equals)
    codes = b.codes[items]
    np_runs = []
    for _ in range(max(1, min(repeats, 3))):
        t0 = time.perf_counter()
        table, triples = numpy_spectrum(codes, P, p, S, motif, tpl.astype(np.int64), fields, ops, n_ops, group.astype(np.int64), n_groups)
        np_runs.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(table, spec) and np.array_equal(triples, per_item), "the numpy model and the kernel disagree"
    np_ms = sorted(np_runs)[len(np_runs) // 2]
    by_class = {"full": int((cls > 0).sum()), "partial": int((cls == -1).sum()), "rept": int((cls == -2).sum())}
    res = {"tool": "tools/spectrum_bench.py", "samples": samples, "units": g, "reads": int(n), "items": int(m), "items_by_class": by_class,
           "groups": int(n_groups), "cap": int(cap), "clean_units": int(spec[:, BINS].sum()), "touched_units": int(spec[:, BINS + 2].sum()),
           "motif_share": float(triples[:, 1].sum() / max(1, triples[:, 0].sum())),
           "with_indel": int(((ops & 15) != 0).any(axis=1).sum()),
           "spectrum_device_ms_per_call": dev, "spectrum_call_wall_ms": wall,
           "spectrum_device_ms_per_million_items": dev["median"] / m * 1e6,
           "numpy_wall_ms": np_ms, "numpy_equals_kernel": True, "numpy_wall_over_device": np_ms / dev["median"],
           "numpy_wall_over_call_wall": np_ms / wall["median"], "clocks_before": before, "clocks_after": after,
           "repeats": repeats, "library": _lib.version()}
    ctx.close()
    if "--parent-tree" in opt:                     # the pileup kernels, on the build before and on this one, alternated
        res["pileup_bench_128_15"] = {"parent": [], "this": []}
        for _ in range(3):
            for name, tree in (("parent", os.path.abspath(opt["--parent-tree"])), ("this", ROOT)):
                r = child([os.path.join(tree, "tools", "pileup_bench.py"), "128", "15"])
                res["pileup_bench_128_15"][name].append(r["pileup_device_ms_per_call"])
    res["one_word_vs_random_words"] = child([here, "--word-case", str(repeats)])
    print(json.dumps(res))
    if len(argv) > 2:
        with open(argv[2], "w") as fp:
            json.dump(res, fp, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
