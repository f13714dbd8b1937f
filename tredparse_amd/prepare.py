"""Loci of your own from a reference FASTA: `python -m tredparse_amd.prepare locus` cuts the flanks of one locus and writes
its site file, `python -m tredparse_amd.prepare scan` finds the tandem repeats of a FASTA on the GPU -- the perfect ones, or
with --interruptions those that substitutions interrupt -- and writes them as a catalogue (and, on request, as site files).

The site files are the reference's schema (its sites/README.md; meta.TREDsRepo(sites=...) loads them, tred.py --sites DIR
points at them).  The reference's own tool asks its questions on the terminal, needs pyfaidx and writes "repeat": "CAG"
whatever motif was entered; this one takes options, reads the FASTA itself and checks that the tract is where it is said to be.

The scan is include/tredscan.h (Context.scan): the maximal runs of every period 1 .. 6 with at least min_copies whole copies
and a primitive motif.  The min_copies defaults (_lib.SCAN_MIN_COPIES: 10, 6, 5, 4, 4, 4) are a choice, not a measurement.
Genotyping at catalogue scale -- thousands of scanned loci in one tred.py run, alternative regions for user loci, cut-offs
derived from data -- is out of scope: a scanned site carries placeholder cut-offs.

`scan --interruptions` is include/tredtract.h (Context.scan_tracts): perfect runs of seed_copies copies of one motif in one
phase are joined across at most max_gap substituted letters, so (CGG)9 AGG (CGG)9 AGG (CGG)10 is one row of 30 copies with
2 mismatches, not three.  Its defaults (_lib.TRACT_SEED_COPIES: 5, 3, 3, 3, 3, 3; _lib.TRACT_MAX_GAP_DEFAULT: 1 .. 6, one
unit) are a choice, not a measurement either.  A lone unit behind an interruption is not absorbed, and indels end a tract.
"""
import argparse
import json
import mmap
import os
import re
import sys

import numpy as np

from . import _lib, meta

FLANK = 18
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")
_STRIP = b"\r\n"
CATALOG_COLUMNS = ("contig", "start", "end", "period", "motif", "copies", "partial", "canonical", "prefix", "suffix")
TRACT_COLUMNS = CATALOG_COLUMNS + ("seeds", "mismatches", "purity")     # the catalogue of scan --interruptions
# every column of a site file (the reference's sites/PIEZO1.json); what the tool cannot know stays ""
SITE_COLUMNS = ("allele_freq", "cutoff_prerisk", "cutoff_risk", "gene_location", "gene_name", "gene_part", "id", "inheritance",
                "motif", "mutation_nature", "normal", "omim_id", "prefix", "prerisk", "repeat", "repeat_location",
                "repeat_location.hg19", "risk", "src", "suffix", "symptom", "title", "url", "variant_type")


class PrepareError(ValueError):
    """A refusal of the tool: the message is for the user."""


# ---- FASTA -----------------------------------------------------------------------------------------------------------------
class Fasta(object):
    """Random access to an uncompressed FASTA through an mmap.  `<path>.fai` is read where it exists (samtools faidx's five
    columns), else the file is indexed here: any line width, a short last line, \\r\\n line ends."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as fp:
            magic = fp.read(2)
        if path.endswith((".gz", ".bgz")) or magic == b"\x1f\x8b":
            raise PrepareError("{}: a compressed FASTA cannot be read in place; decompress it first (gunzip -k)".format(path))
        self._fp = open(path, "rb")
        self._mm = mmap.mmap(self._fp.fileno(), 0, access=mmap.ACCESS_READ) if os.path.getsize(path) else b""
        self.index = {}                     # name -> (length, offset, linebases, linewidth)
        self.names = []
        fai = path + ".fai"
        rows = self._read_fai(fai) if os.path.exists(fai) else self._build_index()
        for name, row in rows:
            if name in self.index:
                raise PrepareError("{}: contig `{}` twice".format(path, name))
            self.index[name] = row
            self.names.append(name)

    def close(self):
        if self._mm:
            self._mm.close()
        self._fp.close()

    @staticmethod
    def _read_fai(fai):
        rows = []
        with open(fai) as fp:
            for line in fp:
                f = line.rstrip("\n").split("\t")
                if len(f) < 5:
                    raise PrepareError("{}: not a .fai line: `{}`".format(fai, line.strip()))
                rows.append((f[0], tuple(int(x) for x in f[1:5])))
        return rows

    def _build_index(self):
        mm, size = self._mm, len(self._mm)
        rows = []
        at = 0 if size and mm[0:1] == b">" else mm.find(b"\n>") + 1 if size else 0
        if size and mm[at:at + 1] != b">":
            raise PrepareError("{}: no `>` line".format(self.path))
        while at < size:
            eol = mm.find(b"\n", at)
            eol = size if eol < 0 else eol
            name = (mm[at + 1:eol].split() or [b""])[0].decode()
            offset = min(eol + 1, size)
            nxt = mm.find(b"\n>", offset - 1)
            end = size if nxt < 0 else nxt + 1
            stop = end
            while stop > offset and mm[stop - 1:stop] in (b"\n", b"\r", b" ", b"\t"):
                stop -= 1
            first = mm.find(b"\n", offset, end)                 # (the first line with its end, as samtools faidx counts it)
            linewidth = (first + 1 if first >= 0 else stop) - offset
            linebases = len(mm[offset:offset + linewidth].rstrip(_STRIP))
            length = 0
            if stop > offset:
                full, rest = divmod(stop - offset, linewidth)
                length = full * linebases + min(rest, linebases)
                ends = np.flatnonzero(np.frombuffer(mm, np.uint8, stop - offset, offset) == 10)
                if len(ends) != (length + linebases - 1) // linebases - 1 or ((ends + 1) % linewidth).any():
                    raise PrepareError("{}: the lines of contig `{}` differ in width".format(self.path, name))
            rows.append((name, (length, offset, max(linebases, 1), max(linewidth, 1))))
            at = end
        return rows

    def length(self, contig):
        if contig not in self.index:
            raise PrepareError("{}: no contig `{}`".format(self.path, contig))
        return self.index[contig][0]

    def fetch(self, contig, start=0, end=None):
        """Letters [start, end) of the contig, 0-based, as upper-case bytes."""
        length = self.length(contig)
        _, offset, linebases, linewidth = self.index[contig]
        end = length if end is None else end
        if not 0 <= start <= end <= length:
            raise PrepareError("{}:{}-{} is outside the contig (1 .. {})".format(contig, start + 1, end, length))
        if start == end:
            return b""
        at = lambda i: offset + i // linebases * linewidth + i % linebases
        return self._mm[at(start):at(end - 1) + 1].translate(None, _STRIP).upper()


# ---- the scan, batched -----------------------------------------------------------------------------------------------------
def parse_periods(text):
    """'1-6', '2,3', '3' -> the set of periods."""
    out = set()
    for part in str(text).split(","):
        lo, _, hi = part.partition("-")
        out.update(range(int(lo), int(hi or lo) + 1))
    if not out or min(out) < 1 or max(out) > _lib.SCAN_MAX_PERIOD:
        raise PrepareError("periods are 1 .. {}: `{}`".format(_lib.SCAN_MAX_PERIOD, text))
    return out


def _min_copies(min_copies, periods):
    mc = list(_lib.SCAN_MIN_COPIES if min_copies is None else min_copies)
    if len(mc) != _lib.SCAN_MAX_PERIOD or any(int(m) != m or (m < 2 and m != 0) for m in mc):
        raise PrepareError("min_copies: {} counts of 2 and above (0: the period is off)".format(_lib.SCAN_MAX_PERIOD))
    if periods is not None:
        mc = [m if p in periods else 0 for p, m in enumerate(mc, 1)]
    if not any(mc):
        raise PrepareError("every period is switched off")
    return [int(m) for m in mc]


def _tract_params(mc, interruptions):
    """(seed_copies, max_gap) of scan_repeats' `interruptions` (True: the defaults), checked against include/tredtract.h's
    rules for the periods that are on."""
    sc, mg = (_lib.TRACT_SEED_COPIES, _lib.TRACT_MAX_GAP_DEFAULT) if interruptions is True else interruptions
    sc, mg = list(sc), list(mg)
    if len(sc) != _lib.SCAN_MAX_PERIOD or len(mg) != _lib.SCAN_MAX_PERIOD or any(int(x) != x for x in sc + mg):
        raise PrepareError("seed_copies and max_gap: {} whole numbers each".format(_lib.SCAN_MAX_PERIOD))
    for p, (m, c, g) in enumerate(zip(mc, sc, mg), 1):
        if m == 0:
            continue
        if not 2 <= c <= m:
            raise PrepareError("period {}: 2 <= seed_copies <= min_copies does not hold (seed_copies {}, min_copies {})".format(p, c, m))
        if not 0 <= g <= _lib.TRACT_MAX_GAP:
            raise PrepareError("period {}: 0 <= max_gap <= {} does not hold (max_gap {})".format(p, _lib.TRACT_MAX_GAP, g))
        if not c * p > g + 2 * p - 2:
            raise PrepareError("period {}: seed_copies * p > max_gap + 2 p - 2 does not hold ({} * {} <= {} + {}): longer seeds or "
                               "a smaller gap".format(p, c, p, g, 2 * p - 2))
    return [int(c) for c in sc], [int(g) for g in mg]


def _scan_tracts(ctx, segments, mc, interruptions, max_letters, cap):
    """scan_repeats' tract path: the segments batched into Context.scan_tracts calls of at most max_letters letters."""
    sc, mg = _tract_params(mc, interruptions)
    bufs = [letters if isinstance(letters, np.ndarray) else np.frombuffer(letters, np.uint8) for letters in segments]
    for k, buf in enumerate(bufs):
        if len(buf) > max_letters:
            raise PrepareError("segment {} has {} letters, more than the {} of one call: tracts are not joined across a cut "
                               "(scan it in regions, or without --interruptions)".format(k, len(buf), max_letters))
    found = []
    i = 0
    while i < len(bufs):
        j, letters = i, 0
        while j < len(bufs) and (j == i or letters + len(bufs[j]) <= max_letters):
            letters += len(bufs[j])
            j += 1
        buf = bufs[i] if j == i + 1 else np.concatenate(bufs[i:j])
        off = np.concatenate(([0], np.cumsum([len(b) for b in bufs[i:j]]))).astype(np.int64)
        out = ctx.scan_tracts(buf, off, mc, sc, mg, cap)
        if out[6] > len(out[0]):
            out = ctx.scan_tracts(buf, off, mc, sc, mg, out[6])
        found.append(np.stack([out[0].astype(np.int64) + i] + [x.astype(np.int64) for x in out[1:6]], axis=1).reshape(-1, 6))
        i = j
    rows = np.concatenate(found) if found else np.zeros((0, 6), np.int64)
    return (rows[:, 0].astype(np.int32), rows[:, 1].copy()) + tuple(rows[:, k].astype(np.int32) for k in range(2, 6))


def scan_repeats(ctx, segments, min_copies=None, periods=None, max_letters=_lib.SCAN_MAX_LETTERS, cap=1 << 16, interruptions=None):
    """The tandem repeats of `segments` (bytes-like letter sequences) by Context.scan, as (seg int32, start int64, length
    int32, period int32) in ascending (seg, start, period) order -- what one call on all segments would give, whatever
    their sizes.  Segments are batched into calls of at most max_letters letters.  A longer segment is cut into pieces that
    overlap by the longest run that just qualifies (max of min_copies p, and no less than the longest period): a run that
    crosses a cut qualifies in the piece on either side, two pieces of one run share at least p letters -- which two
    different runs of period p never do -- and are joined by that.  A call whose records exceed `cap` is repeated with
    room for all of them.
    interruptions: None for the above; (seed_copies, max_gap), or True for the defaults (a choice, not a measurement), for
    the interrupted tracts of Context.scan_tracts (include/tredtract.h): the return gains seeds and mismatch (int32), the
    segments are batched in the same way, and a segment longer than max_letters is refused -- tracts are not joined
    across a cut."""
    mc = _min_copies(min_copies, periods)
    if interruptions is not None:
        return _scan_tracts(ctx, segments, mc, interruptions, max_letters, cap)
    overlap = max([m * p for p, m in enumerate(mc, 1)] + [_lib.SCAN_MAX_PERIOD])
    if max_letters < 2 * overlap + 2:
        raise PrepareError("max_letters {} is too small for runs of {} letters".format(max_letters, overlap))
    pieces = []                             # (segment, where the piece begins in it, its letters)
    for k, letters in enumerate(segments):
        buf = letters if isinstance(letters, np.ndarray) else np.frombuffer(letters, np.uint8)
        if len(buf) <= max_letters:
            pieces.append((k, 0, buf))
            continue
        at = 0
        while True:
            pieces.append((k, at, buf[at:at + max_letters]))
            if at + max_letters >= len(buf):
                break
            at += max_letters - overlap
    found = []                              # rows (seg, start, end, period), starts within the segment
    i = 0
    while i < len(pieces):
        j, letters = i, 0
        while j < len(pieces) and (j == i or letters + len(pieces[j][2]) <= max_letters):
            letters += len(pieces[j][2])
            j += 1
        batch = pieces[i:j]
        buf = batch[0][2] if len(batch) == 1 else np.concatenate([b[2] for b in batch])
        off = np.concatenate(([0], np.cumsum([len(b[2]) for b in batch]))).astype(np.int64)
        seg, start, length, period, total = ctx.scan(buf, off, mc, cap)
        if total > len(seg):
            seg, start, length, period, total = ctx.scan(buf, off, mc, total)
        owner = np.asarray([b[0] for b in batch], np.int64)[seg]
        begin = np.asarray([b[1] for b in batch], np.int64)[seg] + start
        found.append(np.stack([owner, begin, begin + length, period.astype(np.int64)], axis=1).reshape(-1, 4))
        i = j
    rows = np.concatenate(found) if found else np.zeros((0, 4), np.int64)
    if len(pieces) > len(segments) and len(rows):
        # pieces of one run: the same segment and period, at least `period` letters in common
        rows = rows[np.lexsort((rows[:, 1], rows[:, 3], rows[:, 0]))]
        merged = [list(rows[0])]
        for s, a, b, p in rows[1:]:
            last = merged[-1]
            if s == last[0] and p == last[3] and a <= last[2] - p:
                last[2] = max(last[2], b)
            else:
                merged.append([s, a, b, p])
        rows = np.asarray(merged, np.int64)
    rows = rows[np.lexsort((rows[:, 3], rows[:, 1], rows[:, 0]))]
    return rows[:, 0].astype(np.int32), rows[:, 1].copy(), (rows[:, 2] - rows[:, 1]).astype(np.int32), rows[:, 3].astype(np.int32)


# ---- site files -----------------------------------------------------------------------------------------------------------
def canonical_motif(motif):
    """The smallest rotation of the motif over both strands."""
    m = motif.upper()
    rc = m.encode().translate(_COMPLEMENT)[::-1].decode()
    return min(x[k:] + x[:k] for x in (m, rc) for k in range(len(m)))


def builtin_names():
    with open(meta._DATA) as fp:
        return [row["name"] for row in json.load(fp)["loci"]]


def site_row(contig, start, motif, copies, prefix, suffix, cutoff_prerisk=None, cutoff_risk=None, inheritance="AD",
             mutation_nature="increase"):
    """One site in the reference's schema.  start: 1-based.  Cut-offs that are not given are copies + 1: placeholders."""
    row = dict.fromkeys(SITE_COLUMNS, "")
    row.update(id="{}_{}_{}".format(contig, start, motif), prefix=prefix, suffix=suffix, repeat=motif, motif=motif,
               repeat_location="{}:{}-{}".format(contig, start, start + len(motif) * copies - 1),
               cutoff_prerisk=copies + 1 if cutoff_prerisk is None else cutoff_prerisk,
               cutoff_risk=copies + 1 if cutoff_risk is None else cutoff_risk,
               inheritance=inheritance, mutation_nature=mutation_nature, variant_type="short tandem repeats")
    return row


def write_site(outdir, name, row):
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, name + ".json")
    with open(path, "w") as fp:
        fp.write(json.dumps({name: row}, sort_keys=True, indent=2) + "\n")
    return path


def build_locus(fasta, name, motif, location, copies=None, flank=FLANK, force=False, **columns):
    """The site of one locus: motif x copies at location ('chr4:3074877', 1-based start) of the FASTA, with `flank` letters
    on either side.  copies None: the whole copies of the motif found there.  Returns (row, copies)."""
    motif = motif.upper()
    if not motif or set(motif) - set("ACGT"):
        raise PrepareError("motif `{}`: letters A, C, G, T".format(motif))
    if name in builtin_names():
        raise PrepareError("`{}` is a locus of the built-in table: choose another name".format(name))
    m = re.match(r"^([^:]+):(\d+)$", location.replace(",", ""))
    if not m or int(m.group(2)) < 1:
        raise PrepareError("location `{}`: contig:start, 1-based".format(location))
    contig, start = m.group(1), int(m.group(2))
    length, p = fasta.length(contig), len(motif)
    if start > length:
        raise PrepareError("{} is beyond the end of {} ({} letters)".format(location, contig, length))
    if copies is None:
        copies = 0
        while start - 1 + (copies + 1) * p <= length and fasta.fetch(contig, start - 1 + copies * p, start - 1 + (copies + 1) * p) == motif.encode():
            copies += 1
        if copies == 0:
            raise PrepareError("{} does not show `{}` at {}".format(fasta.path, motif, location))
    if copies < 1:
        raise PrepareError("copies must be 1 or more")
    end = start + p * copies - 1            # 1-based, inclusive
    if start - 1 < flank or end + flank > length:
        raise PrepareError("{}:{}-{} is closer than {} letters to an end of the contig (1 .. {})".format(contig, start, end, flank, length))
    tract = fasta.fetch(contig, start - 1, end).decode()
    if tract != motif * copies and not force:
        raise PrepareError("{}:{}-{} reads {} in {}, not {} x {} (--force writes the site all the same)".format(
            contig, start, end, tract if len(tract) <= 60 else tract[:57] + "...", fasta.path, motif, copies))
    prefix = fasta.fetch(contig, start - 1 - flank, start - 1).decode()
    suffix = fasta.fetch(contig, end, end + flank).decode()
    return site_row(contig, start, motif, copies, prefix, suffix, **columns), copies


# ---- the catalogue ---------------------------------------------------------------------------------------------------------
def parse_regions(fasta, regions):
    """['chr4:100-2000', 'chrX'] -> [(contig, start 0-based, end)]; None: every contig."""
    if not regions:
        return [(name, 0, fasta.length(name)) for name in fasta.names]
    out = []
    for text in regions:
        m = re.match(r"^([^:]+)(?::(\d+)-(\d+))?$", text.replace(",", ""))
        if not m:
            raise PrepareError("region `{}`: contig or contig:start-end".format(text))
        length = fasta.length(m.group(1))
        a, b = (int(m.group(2)) - 1, int(m.group(3))) if m.group(2) else (0, length)
        if not 0 <= a <= b <= length:
            raise PrepareError("region `{}` is outside the contig (1 .. {})".format(text, length))
        out.append((m.group(1), a, b))
    return out


def catalog_rows(fasta, regions, records, flank=FLANK):
    """The records of scan_repeats over parse_regions' regions as the rows of the catalogue (CATALOG_COLUMNS): 1-based
    start, end of the whole copies; the flanks are the contig's, '' where one would leave it.  Records of the tract path
    (six arrays) give TRACT_COLUMNS: end, copies and partial from the tract's length, the motif the letters at its start
    (the first seed's, in phase), then seeds, mismatches and purity = 1 - mismatches / length."""
    rows = []
    for seg, start, length, period, *tract in zip(*records):
        contig, a, _ = regions[seg]
        g, p = a + int(start), int(period)                  # 0-based in the contig
        copies, partial = divmod(int(length), p)
        end = g + copies * p
        motif = fasta.fetch(contig, g, g + p).decode()
        prefix = suffix = ""
        if g >= flank and end + flank <= fasta.length(contig):
            prefix, suffix = fasta.fetch(contig, g - flank, g).decode(), fasta.fetch(contig, end, end + flank).decode()
        row = (contig, g + 1, end, p, motif, copies, partial, canonical_motif(motif), prefix, suffix)
        if tract:
            row += (int(tract[0]), int(tract[1]), "%.4f" % (1 - int(tract[1]) / int(length)))
        rows.append(row)
    return rows


def catalog_text(rows, columns=CATALOG_COLUMNS):
    return "".join("\t".join(str(x) for x in row) + "\n" for row in [("#" + columns[0],) + columns[1:]] + list(rows))


def write_catalog_sites(rows, outdir, max_sites):
    """One site file per row that has its flanks, named <contig>_<start>_<motif>; placeholder cut-offs."""
    usable = [r for r in rows if r[8] and r[9]]
    if len(usable) > max_sites:
        raise PrepareError("{} sites are more than --max-sites {}: narrow the regions, raise --min-copies or the limit".format(
            len(usable), max_sites))
    return [write_site(outdir, "{}_{}_{}".format(r[0], r[1], r[4]), site_row(r[0], r[1], r[4], r[5], r[8], r[9])) for r in usable]


# ---- command line ----------------------------------------------------------------------------------------------------------
def set_argparse():
    p = argparse.ArgumentParser(prog="python -m tredparse_amd.prepare", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="command")
    sub.required = True
    a = sub.add_parser("locus", help="write the site file of one locus", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    a.add_argument("--fasta", required=True, help="the reference FASTA (uncompressed; <fasta>.fai is used where it exists)")
    a.add_argument("--name", required=True, help="the locus name (not one of the built-in table)")
    a.add_argument("--motif", required=True, help="the repeat unit on the forward strand, e.g. CAG")
    a.add_argument("--location", required=True, help="contig:start of the tract, 1-based, e.g. chr4:3074877")
    a.add_argument("--copies", type=int, default=None, help="whole copies in the reference; counted from the FASTA when omitted")
    a.add_argument("--flank", type=int, default=FLANK, help="letters of prefix and suffix")
    a.add_argument("--cutoff-prerisk", dest="cutoff_prerisk", type=int, default=None, help="copies from which an allele is pre-risk (placeholder when omitted: copies + 1)")
    a.add_argument("--cutoff-risk", dest="cutoff_risk", type=int, default=None, help="copies from which an allele is at risk (placeholder when omitted: copies + 1)")
    a.add_argument("--inheritance", choices=("AD", "AR", "XLD", "XLR"), default="AD", help="a placeholder unless given")
    a.add_argument("--mutation-nature", dest="mutation_nature", choices=("increase", "decrease"), default="increase", help="a placeholder unless given")
    a.add_argument("--force", action="store_true", help="write the site although the FASTA does not show motif x copies there")
    a.add_argument("--outdir", default="sites", help="directory of the site file")
    s = sub.add_parser("scan", help="find the tandem repeats of a FASTA on the GPU", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    s.add_argument("--fasta", required=True, help="the reference FASTA (uncompressed; <fasta>.fai is used where it exists)")
    s.add_argument("--regions", nargs="+", default=None, help="contig or contig:start-end (1-based); every contig when omitted")
    s.add_argument("--periods", default="1-6", help="periods to report, e.g. 1-6 or 2,3")
    s.add_argument("--min-copies", dest="min_copies", default=",".join(str(m) for m in _lib.SCAN_MIN_COPIES),
                   help="whole copies a run of period 1,2,..,6 needs; the defaults are a choice, not a measurement")
    s.add_argument("--interruptions", action="store_true",
                   help="join perfect runs of one motif and phase across substituted letters (include/tredtract.h); the catalogue "
                        "gains the columns seeds, mismatches and purity")
    s.add_argument("--seed-copies", dest="seed_copies", default=None, metavar=",".join(str(c) for c in _lib.TRACT_SEED_COPIES),
                   help="whole copies a perfect run of period 1,2,..,6 needs to take part; implies --interruptions; the defaults "
                        "are a choice, not a measurement")
    s.add_argument("--max-gap", dest="max_gap", default=None, metavar=",".join(str(g) for g in _lib.TRACT_MAX_GAP_DEFAULT),
                   help="letters between two runs that are joined, per period; implies --interruptions; the defaults (one unit) "
                        "are a choice, not a measurement")
    s.add_argument("--flank", type=int, default=FLANK, help="letters of prefix and suffix")
    s.add_argument("--out", required=True, help="the catalogue is written to <out>.tsv")
    s.add_argument("--write-sites", dest="write_sites", default=None, metavar="DIR", help="also write one site file per record with flanks")
    s.add_argument("--max-sites", dest="max_sites", type=int, default=1000, help="refuse to write more site files than this")
    s.add_argument("--gpu", type=int, default=0, help="device")
    return p


def run_locus(args):
    fasta = Fasta(args.fasta)
    try:
        row, copies = build_locus(fasta, args.name, args.motif, args.location, copies=args.copies, flank=args.flank, force=args.force,
                                  cutoff_prerisk=args.cutoff_prerisk, cutoff_risk=args.cutoff_risk, inheritance=args.inheritance,
                                  mutation_nature=args.mutation_nature)
    finally:
        fasta.close()
    path = write_site(args.outdir, args.name, row)
    print("|".join((row["prefix"], (row["repeat"] * copies).lower(), row["suffix"])), file=sys.stderr)
    print("{}: {} x {} at {}".format(path, row["repeat"], copies, row["repeat_location"]), file=sys.stderr)
    if args.cutoff_prerisk is None or args.cutoff_risk is None:
        print("warning: cut-offs of {} copies are placeholders (reference copies + 1); inheritance `{}` and mutation nature `{}` "
              "are the defaults unless you gave them: edit {} before you read a risk label off it".format(
                  copies + 1, row["inheritance"], row["mutation_nature"], path), file=sys.stderr)
    return path


def run_scan(args, ctx=None):
    fasta = Fasta(args.fasta)
    try:
        regions = parse_regions(fasta, args.regions)
        try:
            mc = [int(x) for x in args.min_copies.split(",")]
        except ValueError:
            raise PrepareError("--min-copies: six counts, e.g. 10,6,5,4,4,4")
        periods = parse_periods(args.periods)
        on = _min_copies(mc, periods)
        interruptions = None
        if args.interruptions or args.seed_copies is not None or args.max_gap is not None:
            try:
                interruptions = tuple(list(default) if text is None else [int(x) for x in text.split(",")] for text, default in
                                      ((args.seed_copies, _lib.TRACT_SEED_COPIES), (args.max_gap, _lib.TRACT_MAX_GAP_DEFAULT)))
            except ValueError:
                raise PrepareError("--seed-copies and --max-gap: six counts each, e.g. 5,3,3,3,3,3 and 1,2,3,4,5,6")
            _tract_params(on, interruptions)               # (refused before a context is made)
        own = ctx is None
        ctx = _lib.Context(args.gpu) if own else ctx
        try:
            records = scan_repeats(ctx, [fasta.fetch(c, a, b) for c, a, b in regions], mc, periods, interruptions=interruptions)
        finally:
            if own:
                ctx.close()
        rows = catalog_rows(fasta, regions, records, flank=args.flank)
    finally:
        fasta.close()
    with open(args.out + ".tsv", "w") as fp:
        fp.write(catalog_text(rows, CATALOG_COLUMNS if interruptions is None else TRACT_COLUMNS))
    print("{}.tsv: {} {}".format(args.out, len(rows), "repeats" if interruptions is None else "tracts"), file=sys.stderr)
    if args.write_sites:
        paths = write_catalog_sites(rows, args.write_sites, args.max_sites)
        print("{}: {} site files with placeholder cut-offs (reference copies + 1, AD, increase)".format(args.write_sites, len(paths)),
              file=sys.stderr)
    return rows


def main(argv=None):
    args = set_argparse().parse_args(argv)
    try:
        (run_locus if args.command == "locus" else run_scan)(args)
    except PrepareError as e:
        print("prepare: {}".format(e), file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
