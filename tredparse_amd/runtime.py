"""What the pieces of a driver process share (tred.py the CLI and run_many, feeder.py the GPU-inflate pipeline, emit.py
the native writer): the stage timers, the named form of run()'s argument tuple and the record of one genotyped sample."""
import json
import os
import threading
import time
from collections import namedtuple

from .bam_parser import scan_sample


# seconds accumulated over run_many calls: the driver thread's waits for scans, its GPU calls and its formatting; and
# the writer thread's time in the sink (JSON / VCF text and files)
TIMING = {"scan_wait": 0.0, "gpu": 0.0, "format": 0.0, "write": 0.0, "inflate": 0.0, "inflate_blocks": 0, "inflate_failed": 0,
          "inflate_hits": 0, "inflate_misses": 0, "inflate_gpu": 0.0, "walk_regions": 0, "walk_declined": 0,
          "walk_blocks_fetched": 0, "walk_alt_regions": 0, "walk_alt_declined": 0, "walk_call": 0.0, "walk_fetch": 0.0, "pack": 0.0,
          "merged_chunks": 0, "select_samples": 0, "select_declined": 0, "gpu_calls": 0}
_TIMING_LOCK = threading.Lock()


def timing_add(**kw):
    """TIMING[key] += value for every keyword, under a lock: the scan pool, the feeder and the writer thread all
    report here while the driver thread does too (a lost update would show up in bench.py's driver_seconds)."""
    with _TIMING_LOCK:
        for k, v in kw.items():
            TIMING[k] += v


# A driver's timeline, for tuning: with TRED_TIMELINE=<directory> in the environment every mark(event) is kept with its wall-clock
# time and the process writes <directory>/timeline_<pid>.json when it ends (tools/cli_rate.py --timeline reads them).  Off: one
# dictionary look-up per mark.
_TIMELINE = [] if os.environ.get("TRED_TIMELINE") else None


def mark(event, **kw):
    if _TIMELINE is not None:
        _TIMELINE.append((time.time(), event, kw))


def timeline_dump():
    if _TIMELINE:
        try:
            with open(os.path.join(os.environ["TRED_TIMELINE"], "timeline_{}.json".format(os.getpid())), "w") as fp:
                json.dump(_TIMELINE, fp)
        except OSError:
            pass


REPORTS = ("alignments", "consensus", "spectrum")     # the per-read reports, in the order their files are written
_TAIL = ("alignments", "consensus", "consensus_partial", "spectrum")        # members 10-13 of a run() argument tuple


def _options(arg):
    """The reference's run() argument tuple, named.  Members 10-13, where the tuple has them (option_tail), are --alignments,
    --consensus, --consensus-partial and --spectrum; `reports`: the REPORTS among them that are on, in that order;
    `count_repeatpairs`: what the kernels, the tally and the device's selection go by -- `repeatpairs`, or --useclippedreads."""
    samplekey, bam, repo, names, maxinsert, fullsearch, clip, alts, repeatpairs, log = arg[:10]
    o = dict(samplekey=samplekey, bam=bam, repo=repo, names=list(names), maxinsert=maxinsert,
             fullsearch=fullsearch, clip=clip, alts=alts, repeatpairs=repeatpairs, log=log)
    for at, name in enumerate(_TAIL, 10):
        o[name] = bool(arg[at]) if len(arg) > at else False
    o["reports"] = [name for name in REPORTS if o[name]]
    o["count_repeatpairs"] = bool(repeatpairs or clip)
    return o


# what the samples of one GPU batch must share: the kernel-side options and the reports computed with the batch
BatchKey = namedtuple("BatchKey", "maxinsert fullsearch clip count_repeatpairs debug reports consensus_partial")


def batch_key(o):
    return BatchKey(o["maxinsert"], o["fullsearch"], o["clip"], o["count_repeatpairs"], o["log"] == "DEBUG", tuple(o["reports"]),
                    o["consensus_partial"])


# the units of one sample in one BatchResult: `result`, the sample's first unit in it, the locus indices of its units there
Piece = namedtuple("Piece", "result first loci")


class Sample(object):
    """One sample between its scan and its files (tred.genotype_scans fills it, tred.format_sample and the Emitter read it):
    arg, the run() argument tuple; o, _options(arg); scan, the SampleScan that was genotyped (the host's after a fall-back from the
    device's selection); loci, scan.live_loci(); pieces, [Piece] -- one unless the retries cut the batch into single units."""
    __slots__ = ("arg", "o", "scan", "loci", "pieces")

    def __init__(self, arg, scan):
        self.arg, self.o = arg, _options(arg)
        self.take(scan)

    def take(self, scan):                  # (the sample's scan from here on: what was genotyped from an earlier one is forgotten)
        self.scan, self.loci, self.pieces = scan, scan.live_loci(), []

    def units(self):
        """{locus index: UnitResult} of the genotyped units."""
        return {k: p.result.unit(p.first + j) for p in self.pieces for j, k in enumerate(p.loci)}


def option_tail(alignments=False, consensus=False, consensus_partial=False, spectrum=False):
    """What follows the reference's ten members in a run() argument tuple for these flags, as _options reads it: nothing
    when none is set."""
    tail = (bool(alignments), bool(consensus), bool(consensus_partial), bool(spectrum))        # (in _TAIL's order)
    return tail if any(tail) else ()


def collect_sample(arg, long_reads=False):
    """Host half of a sample (thread-safe, no GPU): the native scan of its BAM (long_reads: see scan_sample)."""
    o = _options(arg)
    return scan_sample(o["bam"], o["repo"], o["names"], clip=o["clip"], alts=o["alts"], long_reads=long_reads)
