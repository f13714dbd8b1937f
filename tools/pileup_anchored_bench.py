#!/usr/bin/env python3
"""Device time of the anchored pileup on the headline read set, beside numpy on one core: bench.py's config3 reads (30x,
150 bp, 30 loci) are classified with the dump, the winning row of every PREF / POST read goes through one sw_cigar call,
and the items -- one group per unit, its allele the most units a partial read of the unit was tagged with, so that every
one of them is laid down (Engine.consensus(partial=True) with that one allele asked for) -- through one pileup_anchored
call.  get_timing's selector gives the device time: the median of REPEATS calls after a warm-up, and their range.  The same
items then go through the numpy model: every operation expanded to (group, column, channel) triples, cut to the item's
window, shifted and added with np.add.at; its table must equal the kernel's.

    python tools/pileup_anchored_bench.py [SAMPLES [REPEATS [out.json]]]      (on the GPU)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def numpy_pileup_anchored(codes, P, p, S, h, a, strand, anchor, fields, ops, n_ops, group, n_groups, stride):
    """The table of tredpileup_pileup_anchored for accepted items (codes: uint8 [m][L] base codes of the reads; P, p, S, h,
    a, strand, anchor: per item the lengths of prefix, repeat and suffix, its units, its group's, its strand and anchor).
    Returns (table, seconds spent inside np.add.at)."""
    m, cap = ops.shape
    tlen = P + p * h + S
    whole, left = h == a, (anchor == 1) != (strand == 1)
    col_lo = np.where(whole | left, 0, P)
    col_hi = np.where(~whole & left, P + p * h, tlen)
    slot_lo = np.where(whole | left, 0, P + 1)
    slot_hi = np.where(~whole & left, P + p * h, tlen + 1)
    shift = np.where(whole | left, 0, (a - h) * p)
    ln, code = (ops >> 4).astype(np.int64), (ops & 15).astype(np.int64)
    live = np.arange(cap)[None, :] < n_ops[:, None]
    ln = np.where(live, ln, 0)
    on_ref, on_read = np.where(code != 1, ln, 0), np.where(code != 2, ln, 0)
    r0 = fields[:, 1].astype(np.int64)[:, None] + np.cumsum(on_ref, axis=1) - on_ref       # where every operation begins
    q0 = fields[:, 3].astype(np.int64)[:, None] + np.cumsum(on_read, axis=1) - on_read
    table = np.zeros((n_groups * stride, 8), np.int32)
    spent = 0.0
    item = np.repeat(np.arange(m), cap).reshape(m, cap)
    # insertions: one event per operation, before column r0 of the item's strand
    sel = live & (code == 1)
    it = item[sel]
    slot = np.where(strand[it] == 1, tlen[it] - r0[sel], r0[sel])
    keep = (slot >= slot_lo[it]) & (slot < slot_hi[it])
    it, slot, n = it[keep], slot[keep], ln[sel][keep]
    t0 = time.perf_counter()
    np.add.at(table, (group[it] * stride + slot + shift[it], 6), 1)
    np.add.at(table, (group[it] * stride + slot + shift[it], 7), n.astype(np.int32))
    spent += time.perf_counter() - t0
    # M and D: one triple per step
    sel = live & (code != 1)
    n = ln[sel]
    it = np.repeat(item[sel], n)
    step = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    col = np.repeat(r0[sel], n) + step
    is_m = np.repeat(code[sel] == 0, n)
    letter = codes[it, np.where(is_m, np.repeat(q0[sel], n) + step, 0)].astype(np.int64)
    rev = strand[it] == 1
    ch = np.where(is_m, np.where(rev & (letter < 4), 3 - letter, letter), 5)
    col = np.where(rev, tlen[it] - 1 - col, col)
    keep = (col >= col_lo[it]) & (col < col_hi[it])
    it, col, ch = it[keep], col[keep], ch[keep]
    t0 = time.perf_counter()
    np.add.at(table, (group[it] * stride + col + shift[it], ch), 1)
    spent += time.perf_counter() - t0
    return table.reshape(n_groups, stride, 8), spent


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
    items = np.nonzero((tag == _lib.TAG_PREF) | (tag == _lib.TAG_POST))[0]
    m = len(items)
    unit_of = np.searchsorted(b.unit_read_off, items, side="right") - 1
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
    # one group per unit with a partial read: the allele that takes them all
    units, group = np.unique(unit_of, return_inverse=True)
    group = np.ascontiguousarray(group.reshape(-1).astype(np.int32))
    n_groups = len(units)
    group_units = np.zeros(n_groups, np.int32)
    np.maximum.at(group_units, group, (tpl // 2 + 1).astype(np.int32))
    group_ladder = np.ascontiguousarray(b.unit_ladder[units].astype(np.int32))
    anchor = np.ascontiguousarray(np.where(tag[items] == _lib.TAG_PREF, _lib.PILEUP_ANCHOR_BEGIN, _lib.PILEUP_ANCHOR_END).astype(np.int32))
    period = np.array([len(l[1]) for l in b.ladders])
    pre, suf = np.array([len(l[0]) for l in b.ladders]), np.array([len(l[2]) for l in b.ladders])
    stride = int((pre[group_ladder] + period[group_ladder] * group_units + suf[group_ladder]).max()) + 1
    counts, pstatus = np.zeros((n_groups, stride, 8), np.int32), np.zeros(m, np.int32)

    def pileup():
        ctx.pileup_anchored(packed, woff, rlen, m, lad, tpl, fields, ops, cap, n_ops, group, anchor, n_groups, group_ladder,
                            group_units, stride, counts, pstatus)

    def timed(call, which):
        ctx.reset_timing()
        t0 = time.perf_counter()
        call()
        return ctx.get_timing(which)[1], (time.perf_counter() - t0) * 1e3

    pileup()
    assert not pstatus.any(), "pileup_anchored refused an item"
    runs = [timed(pileup, _lib.KERNEL_PILEUP) for _ in range(repeats)]
    dev, wall = sorted(r[0] for r in runs), sorted(r[1] for r in runs)

    codes = b.codes[items]
    hs = tpl // 2 + 1
    np_runs = []
    for _ in range(max(1, min(repeats, 3))):
        t0 = time.perf_counter()
        table, in_add = numpy_pileup_anchored(codes, pre[lad], period[lad], suf[lad], hs, group_units[group].astype(np.int64), tpl & 1,
                                              anchor, fields, ops, n_ops, group.astype(np.int64), n_groups, stride)
        np_runs.append(((time.perf_counter() - t0) * 1e3, in_add * 1e3))
    assert np.array_equal(table, counts), "the numpy model and the kernel disagree"
    np_runs.sort()
    np_ms, add_ms = np_runs[len(np_runs) // 2]
    res = {"tool": "tools/pileup_anchored_bench.py", "samples": samples, "units": g, "reads": int(n), "items": int(m),
           "groups": int(n_groups), "stride": int(stride), "cap": int(cap), "increments": int(counts[:, :, :7].sum()),
           "shorter_than_their_group": int((hs != group_units[group]).sum()), "with_indel": int(((ops & 15) != 0).any(axis=1).sum()),
           "pileup_anchored_device_ms_per_call": {"median": dev[len(dev) // 2], "min": dev[0], "max": dev[-1]},
           "pileup_anchored_call_wall_ms": {"median": wall[len(wall) // 2], "min": wall[0], "max": wall[-1]},
           "pileup_anchored_device_ms_per_million_items": dev[len(dev) // 2] / m * 1e6,
           "numpy_wall_ms": np_ms, "numpy_add_at_ms": add_ms, "numpy_wall_ms_per_million_items": np_ms / m * 1e6,
           "numpy_equals_kernel": True, "numpy_wall_over_device": np_ms / dev[len(dev) // 2],
           "numpy_wall_over_call_wall": np_ms / wall[len(wall) // 2], "repeats": repeats, "library": _lib.version()}
    ctx.close()
    print(json.dumps(res))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fp:
            json.dump(res, fp, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
