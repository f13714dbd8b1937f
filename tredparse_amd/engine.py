"""Batching engine: turns lists of sample x locus units into calls of the C ABI (libtredgpu.so).

The reference calls its kernels one alignment / one locus at a time (bam_parser.py:132-135,
tred.py:165-167); here the host mirrors (bam_parser.BamParser, models.IntegratedCaller, tred.run)
collect units and hand them to one Engine, which packs reads, registers the template ladders and
launches the SW, tally and grid kernels once per batch.  No CPU fallback: constructing an Engine
needs a GPU.
"""
import json
import os

import numpy as np

from . import _lib
from .runtime import REPORTS

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_VALUE = float(np.exp(-10))  # models.py:34


def load_model():
    """Step-size pdfs (6 x 37) and stutter weights (5) from the package data (models.py:42-84)."""
    with open(os.path.join(HERE, "data", "model.json")) as fp:
        m = json.load(fp)
    step = np.array([m["step_size_by_period"][str(p)] for p in range(1, 7)], np.float64)
    return step, np.array(m["stutter_weights"], np.float64)


class Unit(object):
    """Everything the hot path needs for one sample x locus (one runBam, tred.py:153-169)."""

    def __init__(self, tred, readlen, reads, depth, ploidy, global_lens, target_lens, maxinsert=300,
                 fullsearch=False, clip=False, read_pair_ids=None):
        self.tred = tred
        self.readlen = int(readlen)
        self.reads = list(reads)
        self.depth = float(depth)
        self.ploidy = int(ploidy)
        self.global_lens = list(global_lens)
        self.target_lens = list(target_lens)
        self.maxinsert = int(maxinsert)
        self.fullsearch = bool(fullsearch)
        self.clip = bool(clip)
        self.read_pair_ids = read_pair_ids  # only for --norepeatpairs
        self.max_units = -(-self.readlen // len(tred.repeat))          # bam_parser.py:73


JOINT_CAP = 512   # sparse joint entries per unit asked for first (pairs with exp(ml - max) >= e^-10)


class PackedUnits(object):
    """A batch of sample x locus units already in the C ABI's layout (include/tredgpu.h): what
    bam_parser.scan_sample produces, concatenated over samples (from_scans: no read strings, no per-read Python objects),
    or a list of Unit (from_units).  The one form every Engine entry point works on.

      packed / read_off / read_len          the reads, unit after unit
      unit_read_off, ladder_keys[unit]      reads of each unit; its template ladder (prefix, repeat, suffix, max_units)
      params (UNIT_DTYPE)                   grid inputs; pe_off / tl_off index global_lens / target_lens
      pair_id                               per read, for --norepeatpairs (None otherwise)
      text(i)                               read i as text
    """

    @classmethod
    def from_units(cls, units):
        """units: [Unit].  The only place that turns Unit objects into the C ABI's arrays; the reads are packed once."""
        units = list(units)
        clips = set(u.clip for u in units)
        if len(clips) > 1:
            raise ValueError("all units of one batch must share the clip setting")
        b = cls()
        b.clip, b._picks = (clips.pop() if clips else False), None
        b._texts = [r for u in units for r in u.reads]
        b.packed, b.read_off, b.read_len = _lib.pack_reads(b._texts)
        b.n_units, b.n_reads = len(units), len(b._texts)
        b.unit_read_off = np.zeros(b.n_units + 1, np.int32)
        b.unit_read_off[1:] = np.cumsum([len(u.reads) for u in units])
        b.pair_id = None
        if any(u.read_pair_ids is not None for u in units):       # (a unit without ids: -1 for its reads)
            b.pair_id = np.concatenate([np.asarray(u.read_pair_ids if u.read_pair_ids is not None
                                                   else -np.ones(len(u.reads)), np.int32) for u in units])
        b.ladder_keys = [(u.tred.prefix, u.tred.repeat, u.tred.suffix, u.max_units) for u in units]
        b.max_units = max([k[3] for k in b.ladder_keys] + [1])
        g = np.array([len(u.global_lens) for u in units], np.int64)
        t = np.array([len(u.target_lens) for u in units], np.int64)
        b.global_lens = np.asarray([x for u in units for x in u.global_lens], np.int32)
        b.target_lens = np.asarray([x for u in units for x in u.target_lens], np.int32)
        cols = np.array([(len(u.tred.repeat), u.readlen, u.ploidy, u.maxinsert, u.fullsearch, u.tred.repeat_end - u.tred.repeat_start,
                          u.tred.cutoff_risk, u.tred.is_expansion, u.tred.is_recessive) for u in units], np.int32).reshape(-1, 9).T
        b.params = _rows(*cols, np.cumsum(g) - g, g, np.cumsum(t) - t, t, np.array([u.depth for u in units], np.float64))
        return b

    def text(self, i):
        """Read i of the batch as text: the unit's own string (from_units), or what the scan's record decodes to
        (from_scans; the picks' read indices are put together on the first call)."""
        if self._picks is None:
            return self._texts[i]
        if self._texts is None:
            ends, parts = [], []            # per pick with loci: where its reads end in the batch; (scan, their pool indices)
            for scan, ks in self._picks:
                if len(ks):
                    u = scan.unit[np.asarray(ks, np.int64)]
                    parts.append((scan, _ranges(u["read_first"].astype(np.int64), u["n_reads"].astype(np.int64), force=True)))
                    ends.append(len(parts[-1][1]) + (ends[-1] if ends else 0))
            self._texts = (np.asarray(ends, np.int64), parts)
        ends, parts = self._texts
        p = int(np.searchsorted(ends, i, side="right"))
        scan, reads = parts[p]
        return scan.sequence(int(reads[i - (int(ends[p - 1]) if p else 0)]))

    @classmethod
    def from_scans(cls, picks, maxinsert=300, fullsearch=False, clip=False, repeatpairs=True):
        """picks: [(SampleScan, [locus indices])] -- the listed loci of each scan, in that order.  One pass of array
        operations per scan (a unit at a time in Python this cost a driver 0.6-1.2 ms per sample, 30 units each).  The
        batch keeps a reference to picks for text(): the scans live as long as the batch (and a BatchResult of it), and
        the caller must not change the lists afterwards."""
        b = cls()
        b.clip, b.ladder_keys, b._picks, b._texts = bool(clip), [], picks, None
        words, offs, lens, ids, gls, tls, rows, counts = [], [np.zeros(1, np.int64)], [], [], [], [], [], []
        wbase = n_gl = n_tl = 0
        for scan, ks in picks:
            if not len(ks):
                continue
            ks = np.asarray(ks, np.int64)
            u = scan.unit[ks]
            first, n = u["read_first"].astype(np.int64), u["n_reads"].astype(np.int64)
            reads = _ranges(first, n)                         # pool indices of the units' reads, unit after unit
            if isinstance(reads, slice):
                w0, w1 = int(scan.word_off[reads.start]), int(scan.word_off[reads.stop])
                words.append(scan.packed[w0:w1])
                offs.append(scan.word_off[reads.start + 1:reads.stop + 1] - w0 + wbase)
                wbase += w1 - w0
            else:
                lo, hi = scan.word_off[reads], scan.word_off[reads + 1]
                size = hi - lo
                words.append(scan.packed[_ranges(lo, size, force=True)])
                offs.append(np.cumsum(size) + wbase)
                wbase += int(size.sum())
            lens.append(scan.read_len[reads])
            if not (repeatpairs or clip):
                ids.append(scan.name_id[reads])
            g, t = u["n_global"].astype(np.int64), u["n_target"].astype(np.int64)
            gls.append(scan.global_lens[_ranges(u["global_first"].astype(np.int64), g)])
            tls.append(scan.target_lens[_ranges(u["target_first"].astype(np.int64), t)])
            rows.append(_unit_rows(scan, ks, maxinsert, fullsearch, n_gl + np.cumsum(g) - g, n_tl + np.cumsum(t) - t))
            counts.append(n)
            n_gl += int(g.sum())
            n_tl += int(t.sum())
            keys = _ladder_keys(scan)
            b.ladder_keys += [keys[k] for k in ks.tolist()]
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts), dt) if parts else np.zeros(0, dt)
        b.params = cat(rows, _lib.UNIT_DTYPE)
        b.n_units = len(b.params)
        b.unit_read_off = np.zeros(b.n_units + 1, np.int32)
        if counts:
            np.cumsum(np.concatenate(counts), out=b.unit_read_off[1:])
        b.n_reads = int(b.unit_read_off[-1])
        b.packed = cat(words, np.uint32)
        b.read_off = cat(offs, np.int64)
        b.read_len = cat(lens, np.int32)
        b.pair_id = None if (repeatpairs or clip) else cat(ids, np.int32)
        b.global_lens, b.target_lens = cat(gls, np.int32), cat(tls, np.int32)
        b.max_units = max([k[3] for k in b.ladder_keys] + [1])
        return b


def _ranges(first, count, force=False):
    """The concatenation of arange(first[i], first[i] + count[i]) -- as a slice when the ranges follow each other
    without a gap (the common case: a scan's pools hold its loci one after the other)."""
    total = int(count.sum())
    if total == 0:
        return slice(0, 0) if not force else np.zeros(0, np.int64)
    live = count > 0
    f, c = first[live], count[live]
    if not force and (len(f) == 1 or (f[1:] == f[:-1] + c[:-1]).all()):
        return slice(int(f[0]), int(f[0]) + total)
    starts = np.cumsum(c) - c
    return np.repeat(f - starts, c) + np.arange(total, dtype=np.int64)


def _static(scan):
    """Per-locus constants of a scan's locus list as arrays (period, tract span, cut-off, inheritance flags) and its
    template-ladder keys per read length -- the same for every sample of a cohort, so kept on the locus list's first
    Locus object (scans of one repo and list share their Locus objects)."""
    loci = scan.loci
    if not loci:
        return {"period": np.zeros(0, np.int32), "span": np.zeros(0, np.int32), "cutoff_risk": np.zeros(0, np.int32),
                "is_expansion": np.zeros(0, np.int32), "is_recessive": np.zeros(0, np.int32), "ladder": {}}
    key = tuple(id(t) for t in loci)
    hit = _STATIC.get(key)
    if hit is None or hit[0] is not loci[0]:
        st = {"period": np.array([len(t.repeat) for t in loci], np.int32),
              "span": np.array([t.repeat_end - t.repeat_start for t in loci], np.int32),
              "cutoff_risk": np.array([int(t.cutoff_risk) for t in loci], np.int32),
              "is_expansion": np.array([int(t.is_expansion) for t in loci], np.int32),
              "is_recessive": np.array([int(t.is_recessive) for t in loci], np.int32), "ladder": {}}
        if len(_STATIC) > 256:
            _STATIC.clear()
        hit = _STATIC[key] = (loci[0], st)
    return hit[1]


_STATIC = {}


def _ladder_keys(scan):
    """The template-ladder key (prefix, repeat, suffix, max_units) of every locus of a scan at its read length."""
    st = _static(scan)
    keys = st["ladder"].get(scan.readlen)
    if keys is None:
        keys = st["ladder"][scan.readlen] = [(x.prefix, x.repeat, x.suffix, -(-scan.readlen // len(x.repeat))) for x in scan.loci]
    return keys


def _unit_rows(scan, ks, maxinsert, fullsearch, pe_off, tl_off):
    """The grid inputs (UNIT_DTYPE rows) of a scan's loci ks; pe_off / tl_off: where each unit's pair lengths start in the
    call's global_lens / target_lens."""
    st, u = _static(scan), scan.unit[ks]
    return _rows(st["period"][ks], scan.readlen, scan.ploidy[ks], maxinsert, fullsearch, st["span"][ks], st["cutoff_risk"][ks],
                 st["is_expansion"][ks], st["is_recessive"][ks], pe_off, u["n_global"], tl_off, u["n_target"],
                 np.asarray(scan.depth, np.float64)[ks])


def _rows(period, readlen, ploidy, maxinsert, fullsearch, span, cutoff_risk, is_expansion, is_recessive, pe_off, n_global,
          tl_off, n_target, depth):
    """UNIT_DTYPE rows from columns (arrays, one entry per unit, or scalars): the one place that builds them.  span: the
    tract's repeat_end - repeat_start."""
    r = np.zeros(len(period), _lib.UNIT_DTYPE)
    r["period"], r["readlen"], r["ploidy"] = period, readlen, ploidy
    r["maxinsert"], r["fullsearch"] = maxinsert, np.asarray(fullsearch, np.int32)
    r["ref_len"], r["minpe"] = span + 1, span + 2 * 9 + 2          # bam_parser.py:68, :361
    r["cutoff_risk"], r["is_expansion"], r["is_recessive"] = cutoff_risk, is_expansion, is_recessive
    r["pe_off"], r["n_global"] = pe_off, n_global
    r["tl_off"], r["n_target"] = tl_off, n_target
    r["half_depth"] = depth / 2
    return r


def _pad(lens):
    """A length array as the C ABI takes it: never empty (the count is passed on its own)."""
    return lens if len(lens) else np.zeros(1, np.int32)


def _marg_stride(params, hs):
    return max(int(params["maxinsert"].max()) if len(params) else 0, hs) + 2


def _joint_readback(g, period, call):
    """The sparse joint distribution of g units: call(joff, trip, jn, jt) makes the library call into room for
    JOINT_CAP entries per unit; a unit whose flat likelihood surface needs more is asked again with room for every
    entry.  Returns joint -- per unit (triples {h1, h2, exp(ml - max)}, total) -- and joint_units, the batch's entries as
    P_h1h2 prints them (alleles in repeat units, values divided by their unit's total) in one pass over the batch's
    array: (a, b, value, lo, n), laid out by the final capacity; unit i's entries are [lo[i]:lo[i] + n[i]]."""
    cap = np.full(g, JOINT_CAP, np.int64)
    while True:
        joff = np.zeros(g + 1, np.int64)
        joff[1:] = np.cumsum(cap)
        trip = np.zeros((int(joff[-1]), 3), np.float64)
        jn, jt = np.zeros(g, np.int32), np.zeros(g, np.float64)
        call(joff, trip, jn, jt)
        if (jn <= cap).all():
            break
        cap = np.maximum(cap, jn)
    joint = [(trip[joff[i]:joff[i] + jn[i]], float(jt[i])) for i in range(g)]
    per = np.repeat(np.asarray(period, np.int64), cap)
    with np.errstate(divide="ignore", invalid="ignore"):
        units = (trip[:, 0].astype(np.int64) // per, trip[:, 1].astype(np.int64) // per, trip[:, 2] / np.repeat(jt, cap),
                 joff[:-1], jn)
    return joint, units


class _SelectedBatch(object):
    """What a BatchResult's users read of its batch, for units whose reads were packed on the device (genotype_selected)."""
    __slots__ = ("unit_read_off", "n_units", "n_reads", "params", "clip", "ladder_keys", "pair_id", "max_units")


class BatchResult(object):
    """Arrays of one genotyped PackedUnits batch; unit(i) gives the per-unit view the callers format."""
    __slots__ = ("batch", "tag", "h", "score", "full", "pref", "rept", "calls", "marg", "joint", "grid", "grid_off",
                 "joint_units", "repeatpairs", "_emit") + REPORTS

    def __init__(self):
        for name in self.__slots__:           # what a producer does not fill is None (the histograms of the fused calls, the
            setattr(self, name, None)         # dense dump, the reports nobody asked for)

    def unit(self, i):
        b = self.batch
        a, e = int(b.unit_read_off[i]), int(b.unit_read_off[i + 1])
        r = UnitResult()
        r.tags, r.hs, r.scores = self.tag[a:e], self.h[a:e], self.score[a:e]
        r.full = r.pref = r.rept_hist = None      # the histograms {units: count}: only where the batch has them (not the fused calls)
        if self.full is not None:
            r.full, r.pref, r.rept_hist = ({int(k): int(v) for k, v in enumerate(x[i]) if v} for x in (self.full, self.pref, self.rept))
        r.rept = int(self.rept[i].sum())
        r.call = self.calls[i]
        called = self.calls[i]["status"] == 0
        r.grid = self.grid[self.grid_off[i]:self.grid_off[i] + self.calls[i]["n_pairs"]] if called and self.grid is not None else None
        r.joint = self.joint[i] if called and self.joint is not None else None
        r.joint_units = None
        if called and self.joint_units is not None:
            a, b, v, lo, n = self.joint_units
            r.joint_units = (a[lo[i]:lo[i] + n[i]], b[lo[i]:lo[i] + n[i]], v[lo[i]:lo[i] + n[i]])
        r.P_h1, r.P_h2 = self.marg[i, 0], self.marg[i, 1]
        for name in REPORTS:                      # Engine.alignments' / .consensus' / .spectrum's entry of the unit
            x = getattr(self, name)
            setattr(r, name, x[i] if x is not None else None)
        return r


class UnitResult(object):
    """grid: the dense dump {h1, h2, ml1..ml4} per pair (only when asked for); joint: (triples {h1, h2, exp(ml - max)}
    of the pairs >= e^-10, total over all distinct pairs) -- what P_h1h2 is printed from."""
    __slots__ = ("tags", "hs", "scores", "full", "pref", "rept_hist", "rept", "call", "grid", "joint", "P_h1", "P_h2",
                 "joint_units") + REPORTS


class _Winners(object):
    """Engine.winners' result: the batch, and per tagged read of its units (m of them, in batch order) tag, h, the read's
    index in the batch (items), the winning template (win, db order) and its dump row (best), the unit (unit_of); and the
    arguments and outputs of the sw_cigar call over them (packed / read_off / read_len: the tagged reads gathered from the
    batch, item_ladder, fields, ops, n_ops, cap).  Without a tagged read only batch, items, tag, h and unit_of (all empty)
    are set."""
    __slots__ = ("batch", "tag", "h", "items", "win", "best", "unit_of", "packed", "read_off", "read_len", "item_ladder",
                 "fields", "ops", "n_ops", "cap")

    def take(self, sel):
        """The winners `sel` (indices into them, any order, repeats allowed) as an item list of their own, every array
        C-contiguous: packed u32, read_off i64 [n + 1], read_len i32 (the reads' words gathered), item_ladder i32, win i32,
        fields i16 [n][5], ops u32 [n][cap], n_ops i32 -- the order every item-list entry of the context takes them in."""
        sel = np.asarray(sel, np.int64)
        own = lambda x, dt: np.ascontiguousarray(x[sel], dt)
        return _gather_reads(self.packed, self.read_off, self.read_len, sel) + (
            own(self.item_ladder, np.int32), own(self.win, np.int32), own(self.fields, np.int16), own(self.ops, np.uint32),
            own(self.n_ops, np.int32))


# ---- which group of a report a tagged read is counted in: plain arithmetic on (tag, h, unit), no GPU -----------------------
def _wanted(want):
    """The alleles asked for of one unit as every report takes them: whole repeat units >= 1, each once, ascending."""
    return sorted(set(int(x) for x in want if int(x) >= 1))


def _group_ids(groups, keys):
    """int32 per key: its index in groups, -1 for a key that is no group."""
    group_of = {k: i for i, k in enumerate(groups)}
    return np.array([group_of.get(k, -1) for k in keys], np.int32)


def place_consensus(tag, h, unit_of, alleles, partial=False):
    """Engine.consensus' rule over the winners' tag, h and unit_of: (groups, gid, anchor, n).  groups: [(unit, a)] for every
    allele asked for, units then alleles ascending; gid: int32 per winner, its group or -1; anchor: int32 per winner
    (PILEUP_ANCHOR_*); n: the counters per group, int64 -- "full", "partial", "ambiguous", "beyond".
    A FULL read goes to (unit, h) when that was asked for.  partial: of a unit whose longest allele asked for is a_k and
    next longest a_prev (0 when there is none), a PREF / POST read with a_prev < h <= a_k goes to a_k, anchored in its
    flank; one with h <= a_prev is counted `ambiguous` and one with h > a_k `beyond`, both on a_k and laid nowhere.
    Every other read has no group."""
    groups = [(g, a) for g, want in enumerate(alleles) for a in _wanted(want)]
    gid = _group_ids(groups, [(g, a) if t == _lib.TAG_FULL else None for g, a, t in zip(unit_of.tolist(), h.tolist(), tag.tolist())])
    anchor = np.zeros(len(gid), np.int32)
    n = {kind: np.zeros(len(groups), np.int64) for kind in ("partial", "ambiguous", "beyond")}
    n["full"] = np.bincount(gid[gid >= 0], minlength=len(groups)).astype(np.int64)
    if partial:
        longest = {g: k for k, (g, _) in enumerate(groups)}        # (a unit's alleles ascend: its last group is a_k's)
        anchor_of = {_lib.TAG_PREF: _lib.PILEUP_ANCHOR_BEGIN, _lib.TAG_POST: _lib.PILEUP_ANCHOR_END}
        for j, (g, x, t) in enumerate(zip(unit_of.tolist(), h.tolist(), tag.tolist())):
            if t in anchor_of and g in longest:
                k = longest[g]
                a_prev = groups[k - 1][1] if k and groups[k - 1][0] == g else 0
                kind = "beyond" if x > groups[k][1] else "ambiguous" if x <= a_prev else "partial"
                n[kind][k] += 1
                if kind == "partial":
                    gid[j], anchor[j] = k, anchor_of[t]
    return groups, gid, anchor, n


def place_spectrum(tag, h, unit_of, alleles, period):
    """Engine.spectrum's rule: (groups, gid).  groups: [(unit, class)] -- per unit, ascending, `full:a` for every allele
    asked for, ascending, then `partial`, then `rept`; a unit whose period (period[unit]) is above
    _lib.SPECTRUM_MAX_PERIOD has none.  gid: int32 per winner: a FULL read's is (unit, full:h), a PREF or POST read's
    (unit, partial), a REPT read's (unit, rept) -- -1 where that is no group, and for every other read."""
    groups = [(g, name) for g, p in enumerate(period) if p <= _lib.SPECTRUM_MAX_PERIOD
              for name in ["full:{}".format(a) for a in _wanted(alleles[g])] + ["partial", "rept"]]
    names = {_lib.TAG_PREF: "partial", _lib.TAG_POST: "partial", _lib.TAG_REPT: "rept"}
    return groups, _group_ids(groups, [(g, "full:{}".format(x) if t == _lib.TAG_FULL else names.get(t))
                                       for g, x, t in zip(unit_of.tolist(), h.tolist(), tag.tolist())])


class ReadAlignment(object):
    """How one tagged read was laid on the template it was counted for (Engine.alignments): tag, h (repeat units),
    strand (0: the template as written, 1: its reverse complement), target (the template's text) and al, the
    ssw.PyAlignRes of the pair with its CIGAR."""
    __slots__ = ("tag", "h", "strand", "target", "al")

    def __init__(self, tag, h, strand, target, al):
        self.tag, self.h, self.strand, self.target, self.al = tag, h, strand, target, al

    def verbose(self):
        """The reference's verbose block for the pair (bam_parser.py:145-147): `units target`, str(al).strip(), the
        three lines of al.alignment."""
        return "\n".join(["{} {}".format(self.h, self.target), str(self.al).strip()] + list(self.al.alignment)) + "\n"


class Engine(object):
    def __init__(self, device_id=0, ctx=None, long_reads=False):
        """long_reads: switch the context's long-read path on (reads up to 2 048 bp, ladders up to 4 095 columns)."""
        self.ctx = ctx or _lib.Context(device_id)
        self.long_reads = bool(long_reads)
        if self.long_reads:
            self.ctx.set_long_reads(True)
        step, w = load_model()
        self.ctx.set_model(step, w)       # gc=.68, score=1.0 (models.py:106)
        self._ladders = None

    def close(self):
        self.ctx.close()

    # ---- packed batches (the product path) ------------------------------------------------------------
    def _register(self, keys):
        """Ladder index of every key; the context's ladder table only ever grows, so indices stay valid."""
        known = self._ladders or []
        index = {k: i for i, k in enumerate(known)}
        grew = False
        for k in keys:
            if k not in index:
                index[k] = len(known)
                known = known + [k]
                grew = True
        if grew or self._ladders is None:
            self.ctx.set_ladders(known)
            self._ladders = known
        return np.asarray([index[k] for k in keys], np.int32)

    def classify_packed(self, b, dump=None):
        """SW + tagging of a PackedUnits batch: (tag u8[], h i16[], score i16[]) per read.  dump: i16 [reads][templates][6]
        to fill with every (read, template) pair's row, in db order."""
        n = b.n_reads
        tag, h, sc = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int16), np.zeros(max(n, 1), np.int16)
        if n:
            lad = self._register(b.ladder_keys)
            self.ctx.sw_classify(_lib.MEM_HOST, b.packed, b.read_off, b.read_len, n, b.unit_read_off, lad, b.n_units,
                                 _lib.default_sw_params(clip=b.clip), tag, h, sc, dump, dump.shape[1] if dump is not None else 0)
        return tag[:n], h[:n], sc[:n]

    def genotype_packed(self, b, dense=False):
        """The whole path for a PackedUnits batch -> BatchResult (sparse joint distribution included): one fused call
        (tredgpu_genotype_batch_joint: tags, histograms and calls stay on the device between the stages; one wait).
        dense: also the four terms of every (h1, h2) pair (a second grid call with the dump; what --log DEBUG prints) --
        that path goes through the three separate calls, which hand the histograms back."""
        if dense or b.n_units == 0:
            return self._genotype_packed_stepwise(b, dense)
        gl, tl = _pad(b.global_lens), _pad(b.target_lens)
        params = _lib.default_sw_params(clip=b.clip)

        def call(r, lad, hs, ms, joff, trip, jn, jt):
            self.ctx.genotype_batch_joint(b.packed, b.read_off, b.read_len, b.n_reads, b.unit_read_off, lad, b.params, b.n_units,
                                          params, b.pair_id if b.n_reads else None, gl, len(b.global_lens), tl,
                                          len(b.target_lens), r.tag, r.h, r.score, hs, r.rept, r.calls, r.marg, ms, joff, trip,
                                          jn, jt)
        return self._fused(b, call)

    def genotype_selected(self, scans, maxinsert=300, fullsearch=False, clip=False):
        """genotype_packed for samples whose reads the device selected and still holds (feeder._device_scan: SampleScans with
        `.device` = feeder.DeviceReads: the chunk's lease, the sample's first task, its select results): one tredgpu_genotype_selected call -- pack on the device, SW +
        tagging -> histograms -> grid, one wait -- which also brings back the selected reads' lengths, 4-bit sequences and
        names; they are filled into the scans (per-sample views), so that the writers find what scan_sample would have
        left there.  Every locus of every scan is a unit, in order.  Returns the BatchResult (units in scan order)."""
        segs, rows, keys, pools, sels = [], [], [], {}, []
        g_all, t_all, n_gl, n_tl = [], [], 0, 0
        for s in scans:
            dev, t0, sel = s.device.chunk, s.device.first_task, s.device.sel
            n = len(s.names)
            if dev not in pools:
                pools[dev] = (n_gl, n_tl)
                g_all.append(dev.gp)
                t_all.append(dev.tp)
                n_gl, n_tl = n_gl + len(dev.gp), n_tl + len(dev.tp)
            gb, tb = pools[dev]
            tasks = np.arange(t0, t0 + n, dtype=np.int32)
            if segs and segs[-1][0] is dev.inf:
                segs[-1][1].append(tasks)
            else:
                segs.append((dev.inf, [tasks]))
            rows.append(_unit_rows(s, np.arange(n), maxinsert, fullsearch, gb + s.unit["global_first"], tb + s.unit["target_first"]))
            sels.append(sel)
            keys += _ladder_keys(s)
        b = _SelectedBatch()
        b.params, sel = np.concatenate(rows), np.concatenate(sels)
        g = b.n_units = len(b.params)
        uro = np.zeros(g + 1, np.int32)
        uwo, uso, uno = (np.zeros(g + 1, np.int64) for _ in range(3))
        np.cumsum(sel["n_reads"], out=uro[1:])
        np.cumsum(sel["n_words"], out=uwo[1:])
        np.cumsum(sel["seq4_bytes"], out=uso[1:])
        np.cumsum(sel["name_bytes"], out=uno[1:])
        n = int(uro[-1])
        b.unit_read_off, b.n_reads, b.clip, b.ladder_keys, b.pair_id = uro, n, bool(clip), keys, None
        b.max_units = max([k[3] for k in keys] + [1])
        gl = _pad(np.ascontiguousarray(np.concatenate(g_all), np.int32))
        tl = _pad(np.ascontiguousarray(np.concatenate(t_all), np.int32))
        sw = _lib.default_sw_params(clip=clip, max_read_len=max(int(sel["max_len"].max()), 1))
        read_len = np.zeros(max(n, 1), np.int32)
        s4off, nmoff = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        seq4, names = np.zeros(max(int(uso[-1]), 1), np.uint8), np.zeros(max(int(uno[-1]), 1), np.uint8)
        seg_arg = [(inf, np.concatenate(t)) for inf, t in segs]

        def call(r, lad, hs, ms, joff, trip, jn, jt):
            self.ctx.genotype_selected(seg_arg, uro, uwo, uso, uno, lad, b.params, g, sw, gl, n_gl, tl, n_tl, r.tag, r.h, r.score,
                                       hs, r.rept, r.calls, r.marg, ms, joff, trip, jn, jt, read_len, s4off, seq4, nmoff, names)
        r = self._fused(b, call)
        # the reads' arrays, a sample at a time, as scan_sample leaves them (offsets from the sample's first read)
        u0 = 0
        for s in scans:
            m = len(s.names)
            a, e = int(uro[u0]), int(uro[u0 + m])
            s.read_len = read_len[a:e]
            s.seq4_off = s4off[a:e + 1] - s4off[a]
            s.seq4 = seq4[int(s4off[a]):int(s4off[e])] if e > a else np.zeros(0, np.uint8)
            s.name_off = nmoff[a:e + 1] - nmoff[a]
            s.name_blob = names[int(nmoff[a]):int(nmoff[e])].tobytes() if e > a else b""
            s.name_id = np.zeros(e - a, np.int32)          # (read only under --norepeatpairs, which the device path does not take)
            u0 += m
        return r

    def _fused(self, b, call):
        """The BatchResult of a fused call (genotype_packed, genotype_selected) over batch b: its output arrays, the
        batch's ladders registered, call(r, ladder ids, hist_stride, marg_stride, joff, trip, jn, jt) once per attempt of
        the joint read-back, the per-read outputs trimmed to the batch's reads."""
        r = BatchResult()
        r.batch = b
        g, n = b.n_units, b.n_reads
        hs = b.max_units + 2
        ms = _marg_stride(b.params, hs)
        r.tag, r.h, r.score = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int16), np.zeros(max(n, 1), np.int16)
        r.rept = np.zeros((g, hs), np.int32)
        r.calls = np.zeros(g, _lib.CALL_DTYPE)
        r.marg = np.zeros((g, 2, ms), np.float64)
        lad = self._register(b.ladder_keys)
        r.joint, r.joint_units = _joint_readback(g, b.params["period"], lambda *j: call(r, lad, hs, ms, *j))
        r.tag, r.h, r.score = r.tag[:n], r.h[:n], r.score[:n]
        return r

    def _genotype_packed_stepwise(self, b, dense=False, joint=True, refuse_invalid=False):
        """genotype_packed through the three separate calls (SW, tally, grid); joint=False: no joint distribution;
        refuse_invalid: raise straight after the SW call when a read came back TAG_INVALID."""
        r = BatchResult()
        r.batch = b
        r.tag, r.h, r.score = self.classify_packed(b)
        if refuse_invalid:
            _refuse_invalid(r.tag)
        g, n = b.n_units, b.n_reads
        hs = b.max_units + 2
        r.full, r.pref, r.rept = (np.zeros((g, hs), np.int32) for _ in range(3))
        self.ctx.tally(_lib.MEM_HOST, r.tag if n else np.zeros(1, np.uint8), r.h if n else np.zeros(1, np.int16), n,
                       b.unit_read_off, g, b.pair_id if n else None, hs, r.full, r.pref, r.rept)
        hist = (b.params, hs, r.full, r.pref, r.rept, b.global_lens, b.target_lens)
        r.calls, r.marg, r.joint, r.joint_units = self._grid_arrays(*hist, joint=joint)
        if dense and g:
            r.grid, r.grid_off = self._dense_dump(*hist, r.calls)
        return r

    def _grid_arrays(self, up, hs, full, pref, rept, gl, tl, joint=True):
        """The grid of units `up` from their histograms: (calls, marginals, joint, joint_units) -- with joint=False one
        likelihood_grid call and no joint distribution (None, None)."""
        g = len(up)
        ms = _marg_stride(up, hs)
        calls = np.zeros(g, _lib.CALL_DTYPE)
        marg = np.zeros((g, 2, ms), np.float64)
        grid = (_lib.MEM_HOST, up, g, hs, full, pref, rept, _pad(gl), len(gl), _pad(tl), len(tl), calls)
        if not joint:
            self.ctx.likelihood_grid(*grid, None, None, marg, ms)
            return calls, marg, None, None
        return (calls, marg) + _joint_readback(g, up["period"], lambda *j: self.ctx.likelihood_grid_joint(*grid, marg, ms, *j))

    def _dense_dump(self, up, hs, full, pref, rept, gl, tl, calls):
        """The four terms of every (h1, h2) pair of the units' grids ({h1, h2, ml1..ml4} per pair, unit i's pairs from
        grid_off[i]): a second likelihood_grid call, with the dump."""
        g = len(up)
        grid_off = np.zeros(g + 1, np.int64)
        grid_off[1:] = np.cumsum(np.maximum(calls["n_pairs"], 1))
        grid = np.zeros((int(grid_off[-1]), 6), np.float64)
        self.ctx.likelihood_grid(_lib.MEM_HOST, up, g, hs, full, pref, rept, _pad(gl), len(gl), _pad(tl), len(tl),
                                 np.zeros(g, _lib.CALL_DTYPE), grid_off, grid, None, 0)
        return grid, grid_off

    # ---- lists of Unit: packed once (PackedUnits.from_units), then the packed path ------------------------------
    def classify(self, units, want_dump=False):
        """SW + tagging of units (a list of Unit, or a PackedUnits): (tag u8[], h i16[], score i16[], the units' read
        offsets, dump or None) -- classify_packed, with every (read, template) pair's row when want_dump."""
        b = _batch(units)
        n = b.n_reads
        nt = max([2 * k[3] for k in b.ladder_keys] + [1])
        dump = np.zeros((max(n, 1), nt, 6), np.int16) if want_dump else None
        tag, h, sc = self.classify_packed(b, dump)
        _refuse_invalid(tag)
        return tag, h, sc, b.unit_read_off, (dump[:n] if want_dump else None)

    # ---- the alignment behind every tagged read -------------------------------------------------------
    def winners(self, units):
        """What alignments and consensus share: classify with the dump, then per tagged read (HANG included) the winning
        dump row -- the highest score, then the fewest units, then the first row in db order (bam_parser.py:174), which is
        the pair out_tag / out_h stand for -- and ONE sw_cigar call for all winners, their packed words gathered from the
        batch.  Returns a _Winners: hand it to both when both are wanted, so that these steps run once."""
        b = _batch(units)
        tag, h, sc, uro, dump = self.classify(b, want_dump=True)
        items = np.nonzero(tag != _lib.TAG_NONE)[0]
        m = len(items)
        w = _Winners()
        unit_of = (np.searchsorted(uro, items, side="right") - 1).astype(np.int64)
        w.batch, w.items, w.tag, w.h, w.unit_of = b, items, tag[items], h[items], unit_of
        if m == 0:                            # (no tagged read: nothing was asked of sw_cigar)
            return w
        # rows in db order are u=1 fwd, u=1 rc, u=2 fwd, ...: the first row with the highest score has the fewest units
        rows = dump[items]
        key = np.where(rows[:, :, 5] > 0, rows[:, :, 0].astype(np.int32), -1)
        win = key.argmax(axis=1).astype(np.int32)
        best = rows[np.arange(m), win]
        assert (best[:, 0] == sc[items]).all() and (best[:, 5] == tag[items]).all() and (win // 2 + 1 == h[items]).all(), \
            "the winning dump row is not the pair the read was tagged for"
        w.packed, w.read_off, w.read_len = _gather_reads(b.packed, b.read_off, b.read_len, items)
        fields = np.ascontiguousarray(best[:, :5], np.int16)
        item_ladder = np.ascontiguousarray(self._register(b.ladder_keys)[unit_of])
        cap = 32
        while True:
            ops, n_ops, status = np.zeros((m, cap), np.uint32), np.zeros(m, np.int32), np.zeros(m, np.int32)
            self.ctx.sw_cigar(_lib.MEM_HOST, w.packed, w.read_off, w.read_len, m, item_ladder, win, fields,
                              _lib.default_sw_params(clip=b.clip), cap, ops, n_ops, status, ladders=self._ladders)
            if not (status == _lib.CIGAR_OVERFLOW).any():
                break
            cap = int(n_ops.max())            # (a CIGAR of more than 32 operations: once more with the room it needs)
        _refuse_item("sw_cigar", status, _lib.CIGAR_OK, items, unit_of, uro)
        w.win, w.best = win, best
        w.item_ladder, w.fields, w.ops, w.n_ops, w.cap = item_ladder, fields, ops, n_ops, cap
        return w

    def alignments(self, units, winners=None):
        """Per unit: {read index in the unit: ReadAlignment} for every tagged read (HANG included): the pair the read was
        tagged for and its CIGAR (winners: what self.winners(units) returned, when the caller already has it).  Only
        these reads are turned into text."""
        from .bam_parser import rc
        from .ssw import PyAlignRes
        w = self.winners(units) if winners is None else winners
        b = w.batch
        out = [{} for _ in range(b.n_units)]
        targets = {}
        for j in range(len(w.items)):
            g, t, i = int(w.unit_of[j]), int(w.win[j]), int(w.items[j])
            if (g, t) not in targets:
                prefix, repeat, suffix, _ = b.ladder_keys[g]
                text = prefix + repeat * (t // 2 + 1) + suffix
                targets[(g, t)] = rc(text) if t % 2 else text
            al = PyAlignRes(w.best[j], b.text(i), targets[(g, t)], w.ops[j, :w.n_ops[j]])
            out[g][i - int(b.unit_read_off[g])] = ReadAlignment(int(w.tag[j]), int(w.h[j]), t % 2, targets[(g, t)], al)
        return out

    # ---- what is in the tract of an allele --------------------------------------------------------------
    def _grouped(self, name, w, gid, tail):
        """ONE call of the context's item-list entry `name` (pileup, pileup_anchored, unit_spectrum) over the winners that
        have a group (gid >= 0), in their order: the items taken out of w, their groups, tail(sel) -- the entry's arguments
        between item_group and out_status --, a status per item; an item the entry refuses raises.  No winner with a group:
        no call.  Returns sel, the winners sent."""
        sel = np.nonzero(gid >= 0)[0]
        if len(sel):
            packed, read_off, read_len, item_ladder, win, fields, ops, n_ops = w.take(sel)
            status = np.zeros(len(sel), np.int32)
            getattr(self.ctx, name)(packed, read_off, read_len, len(sel), item_ladder, win, fields, ops, w.cap, n_ops,
                                    np.ascontiguousarray(gid[sel], np.int32), *tail(sel), status, ladders=self._ladders)
            _refuse_item(name, status, _lib.PILEUP_OK, w.items[sel], w.unit_of[sel], w.batch.unit_read_off)
        return sel

    def _group_ladders(self, b, groups):
        """The registered ladder of every group's unit (int32 [n_groups])."""
        return np.ascontiguousarray(self._register(b.ladder_keys)[[g for g, _ in groups]], np.int32)

    def consensus(self, units, alleles, winners=None, partial=False):
        """Per unit: {a: consensus.AlleleConsensus} for every a >= 1 of alleles[unit] (repeat units): the reads of the
        unit tagged FULL with h == a, laid on prefix + repeat * a + suffix by the alignments of self.winners (winners:
        what it returned, when the caller already has it) and counted column by column in ONE pileup call for all units
        and alleles -- one group per (unit, a).  Only FULL reads count: a partial (PREF / POST) or repeat-only read is
        tagged with the longest template it fits, not with an allele, so it cannot be placed on an allele's template.
        An allele no FULL read was counted for -- an expansion longer than the reads, say -- comes back with reads = 0,
        its template in lower case and empty lists.

        partial=True lays the PREF / POST reads down too, in ONE pileup_anchored call with the FULL reads: of a unit whose
        longest allele asked for is a_k and next longest a_prev (0 when there is none), a partial read with
        a_prev < h <= a_k can only come from a_k and is laid on it from the side of its flank (AlleleConsensus.partial);
        one with h <= a_prev fits any allele asked for and is counted as `ambiguous`, one with h > a_k as `beyond`, both on
        a_k and laid nowhere.  REPT and HANG reads are never placed.  (The rule: place_consensus.)"""
        from .consensus import AlleleConsensus
        w = self.winners(units) if winners is None else winners
        b = w.batch
        groups, gid, anchor, n = place_consensus(w.tag, w.h, w.unit_of, alleles, partial)
        out = [{} for _ in range(b.n_units)]
        if not groups:
            return out
        ng = len(groups)
        texts = [b.ladder_keys[g][0] + b.ladder_keys[g][1] * a + b.ladder_keys[g][2] for g, a in groups]
        if partial:             # the groups have their shape from the alleles asked for, which may lie beyond the ladder
            stride = max(len(T) for T in texts) + 1
            tail = lambda sel: (np.ascontiguousarray(anchor[sel]), ng, self._group_ladders(b, groups),
                                np.ascontiguousarray([a for _, a in groups], np.int32), stride, counts)
        else:                   # ... from the ladder's templates: of the table the call is given, not the batch's own
            stride = max(self.ctx._template_len(l) for l in self._ladders) + 1
            tail = lambda sel: (ng, stride, counts)
        counts = np.zeros((ng, stride, _lib.PILEUP_CHANNELS), np.int32)
        self._grouped("pileup_anchored" if partial else "pileup", w, gid, tail)
        for k, ((g, a), T) in enumerate(zip(groups, texts)):
            # (a template beyond the stride is beyond the ladder: nothing was counted on it)
            table = counts[k] if len(T) < stride else np.zeros((len(T) + 1, _lib.PILEUP_CHANNELS), np.int32)
            out[g][a] = AlleleConsensus(a, n["full"][k], table, T, len(b.ladder_keys[g][0]), len(b.ladder_keys[g][1]),
                                        partial=n["partial"][k], ambiguous=n["ambiguous"][k], beyond=n["beyond"][k])
        return out

    # ---- which repeat units the reads of a locus show -------------------------------------------------
    def spectrum(self, units, alleles, winners=None):
        """Per unit a spectrum.RepeatSpectrum: the repeat-unit words of the unit's tagged reads, cut by the alignments of
        self.winners (winners: what it returned, when the caller already has it) and counted in ONE unit_spectrum call
        for all units.  The classes of a unit: `full:a` for every a >= 1 of alleles[unit] (reads tagged FULL with h == a),
        `partial` (all PREF and POST reads, wherever consensus(partial=True) would lay them) and `rept` (all REPT reads);
        HANG reads are in none.  A unit whose period has no table (above _lib.SPECTRUM_MAX_PERIOD) comes back
        `unsupported` and none of its reads are sent.  (The rule: place_spectrum.)"""
        from .spectrum import RepeatSpectrum
        w = self.winners(units) if winners is None else winners
        b = w.batch
        period = [len(k[1]) for k in b.ladder_keys]
        groups, gid = place_spectrum(w.tag, w.h, w.unit_of, alleles, period)
        ng = len(groups)
        spec = np.zeros((ng, _lib.SPECTRUM_STRIDE), np.int32)
        per_item = np.zeros((len(gid), 3), np.int32)                # (the items sent fill its head)
        sel = self._grouped("unit_spectrum", w, gid, lambda sel: (ng, self._group_ladders(b, groups), spec, per_item[:len(sel)]))
        by_group = np.argsort(gid[sel], kind="stable")
        cut = np.searchsorted(gid[sel][by_group], np.arange(ng + 1))
        tables = [None if p > _lib.SPECTRUM_MAX_PERIOD else {} for p in period]
        for k, (g, name) in enumerate(groups):
            tables[g][name] = (spec[k], per_item[by_group[cut[k]:cut[k + 1]]])
        return [RepeatSpectrum(b.ladder_keys[g][1], tables[g]) for g in range(b.n_units)]

    # ---- a child against its parents ------------------------------------------------------------------
    def trio(self, children, fathers, mothers, ploidy, period=None, mu=_lib.TRIO_MU, rho=_lib.TRIO_RHO, beta=_lib.TRIO_BETA):
        """Per item -- one (trio, locus) -- a trio.TrioResult: the child's call given what its parents could have passed on,
        its posterior, the odds that an allele changed on the way (denovo) and that the larger allele is the father's
        (paternal), in ONE Context.trio call for all items (the model: DESIGN.md 4, "Trio evaluation").  children, fathers,
        mothers: per item a trio.PairList or a UnitResult with its dense grid (genotype_packed(b, dense=True); period: the
        loci's periods then, one or per item); a parent that is None, was not called or has no pair says nothing.  ploidy:
        the CHILD's, one or per item -- a ploidy-1 child ignores the father.  mu, rho, beta: the transmission model, whose
        defaults are a choice, not a measurement.  Runs after the samples, not per read: no member of runtime.REPORTS.  An
        item the unit refuses (TRIO_BAD_ITEM, TRIO_TOO_LONG) raises; a child without a pair comes back TRIO_EMPTY_CHILD."""
        from .trio import PairList, TrioResult, member_list, pack_members
        n = len(children)
        if not (len(fathers) == len(mothers) == n):
            raise ValueError("children, fathers and mothers must be of one length")
        per = np.broadcast_to(np.asarray(0 if period is None else period, np.int64), (n,))
        lists = [[member_list(x, int(p) or None) for x, p in zip(role, per)] for role in (children, fathers, mothers)]
        kids = [k if k is not None else PairList([], [], []) for k in lists[0]]
        (child, _), (father, f_inf), (mother, m_inf) = (pack_members(x) for x in [kids] + lists[1:])
        status, call, values = np.zeros(n, np.int32), np.zeros((n, 3), np.int32), np.zeros((n, 4), np.float64)
        J = np.zeros(int(child[0][-1]), np.float64)
        if n:
            self.ctx.trio(n, child, father, mother, np.ascontiguousarray(np.broadcast_to(np.asarray(ploidy, np.int32), (n,))),
                          f_inf, m_inf, status, call, values, J, mu=mu, rho=rho, beta=beta)
        refused = np.where((status == _lib.TRIO_BAD_ITEM) | (status == _lib.TRIO_TOO_LONG), status, _lib.TRIO_OK)
        _refuse_item("trio", refused, _lib.TRIO_OK, np.zeros(n, np.int64), np.arange(n), np.zeros(n, np.int64))
        return [TrioResult(status[i], call[i], values[i], J[child[0][i]:child[0][i + 1]], kids[i]) for i in range(n)]

    # ---- all samples of a locus ----------------------------------------------------------------------
    def cohort(self, lists_per_locus, ploidy_per_locus, period=None, iters=_lib.COHORT_ITERS, alpha=_lib.COHORT_ALPHA,
               tol=_lib.COHORT_TOL):
        """Per locus a cohort.CohortResult: the allele frequencies of the locus by EM over the (h1, h2) surfaces of all its
        samples, and per sample the call under those frequencies as a Hardy-Weinberg prior, its posterior over its pairs
        and logZ, in ONE Context.cohort call for all loci (the model: DESIGN.md 4, "Cohort frequencies").
        lists_per_locus: per locus, per sample a trio.PairList or a UnitResult with its dense grid (genotype_packed(b,
        dense=True); period: the loci's periods then, one or per locus); a sample that is None, was not called or has no
        pair takes no part.  ploidy_per_locus: per locus one ploidy or one per sample.  iters, alpha: the EM's iterations,
        all of which run, and the pseudo-chromosomes; tol: what `converged` reports against -- a choice, not a measurement.
        Runs after the samples, not per read: no member of runtime.REPORTS.  A locus the unit refuses (COHORT_BAD_ITEM,
        COHORT_TOO_LONG) raises; one without a participating sample comes back COHORT_EMPTY."""
        from .cohort import cohort_outputs, pack_cohort, results_of
        from .trio import member_list
        n = len(lists_per_locus)
        per = np.broadcast_to(np.asarray(0 if period is None else period, np.int64), (n,))
        lists = [[member_list(x, int(p) or None) for x in locus] for locus, p in zip(lists_per_locus, per)]
        item_off, samples, ploidy, allele_off, members = pack_cohort(lists, ploidy_per_locus)
        out = cohort_outputs(n, len(members), int(samples[0][-1]), int(allele_off[-1]), int(iters))
        if n:
            self.ctx.cohort(n, item_off, samples, ploidy, allele_off, *out, iters=iters, alpha=alpha)
        status = out[0]
        refused = np.where((status == _lib.COHORT_BAD_ITEM) | (status == _lib.COHORT_TOO_LONG), status, _lib.COHORT_OK)
        _refuse_item("cohort", refused, _lib.COHORT_OK, np.zeros(n, np.int64), np.arange(n), np.zeros(n, np.int64))
        return results_of(n, item_off, samples, ploidy, allele_off, members, out, tol)

    # ---- where the repeats are ----------------------------------------------------------------------
    def scan_repeats(self, segments, min_copies=None, periods=None, interruptions=None):
        """The perfect tandem repeats of `segments` (bytes-like letter sequences) on this engine's context, as (seg, start,
        length, period) arrays in ascending (seg, start, period) order: prepare.scan_repeats, which batches the segments
        into Context.scan calls and joins the runs of a segment longer than one call (the definition: DESIGN.md 4,
        "Tandem-repeat scan").  min_copies: per period 1 .. 6, _lib.SCAN_MIN_COPIES by default -- a choice, not a
        measurement; periods: the periods to report, all by default.  interruptions: None for the perfect repeats;
        (seed_copies, max_gap), or True for _lib.TRACT_SEED_COPIES and _lib.TRACT_MAX_GAP_DEFAULT (a choice too), for the
        interrupted tracts of Context.scan_tracts ("Interrupted tracts"): the return gains seeds and mismatch."""
        from .prepare import scan_repeats
        return scan_repeats(self.ctx, segments, min_copies=min_copies, periods=periods, interruptions=interruptions)

    # ---- the whole path ------------------------------------------------------------------------------
    def genotype(self, units, want_grid=True):
        """SW + tagging -> histograms -> likelihood grid for a batch of units (a list of Unit, or a PackedUnits); returns
        [UnitResult], with the histograms.  want_grid=False: no joint distribution."""
        b = _batch(units)
        r = self._genotype_packed_stepwise(b, joint=want_grid, refuse_invalid=True)
        return [r.unit(i) for i in range(b.n_units)]

    def grid_from_counts(self, unit, full, pref, rept):
        """Likelihood grid of one unit from explicit histograms {units: count} (IntegratedCaller.call)."""
        b = PackedUnits.from_units([unit])
        hs = max(list(full) + list(pref) + [unit.max_units]) + 2
        f, p, r = (np.zeros((1, hs), np.int32) for _ in range(3))
        for row, counts in ((f, full), (p, pref)):
            for k, v in counts.items():
                row[0, k] = v
        r[0, 0] = rept
        hist = (b.params, hs, f, p, r, b.global_lens, b.target_lens)
        calls, marg, _, _ = self._grid_arrays(*hist, joint=False)
        dump, goff = self._dense_dump(*hist, calls)
        res = UnitResult()
        res.tags = res.hs = res.scores = res.joint = None
        res.full, res.pref, res.rept_hist, res.rept = dict(full), dict(pref), {}, rept
        res.call = calls[0]
        res.grid = dump[goff[0]:goff[0] + calls[0]["n_pairs"]] if calls[0]["status"] == 0 else None
        res.P_h1, res.P_h2 = marg[0, 0], marg[0, 1]
        return res


def _batch(units):
    return units if isinstance(units, PackedUnits) else PackedUnits.from_units(units)


def _refuse_invalid(tag):
    if (tag == _lib.TAG_INVALID).any():
        raise _lib.TredGpuError("a read exceeds TREDGPU_MAX_READ_LEN")


def _refuse_item(name, status, ok, items, unit_of, unit_read_off):
    """Raises for the first item of a side call (items: the reads' indices in the batch) whose status is not `ok`."""
    bad = np.nonzero(status != ok)[0]
    if len(bad):
        k = int(bad[0])
        raise _lib.TredGpuError("{}: status {} for read {} of unit {}".format(name, int(status[k]), int(items[k] - unit_read_off[unit_of[k]]),
                                                                          int(unit_of[k])))


def _gather_reads(packed, read_off, read_len, reads):
    """(packed, read_off, read_len) of the reads `reads` (indices) of a packed pool: their words, gathered by index."""
    lo = read_off[reads]
    size = read_off[reads + 1] - lo
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum(size, out=off[1:])
    return (np.ascontiguousarray(packed[_ranges(lo, size, force=True)], np.uint32), off,
            np.ascontiguousarray(read_len[reads], np.int32))
