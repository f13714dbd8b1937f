"""Cohort allele frequencies by EM and population-aware calls: the host side of include/tredcohort.h.

tredreport.py counts every sample's arg-max alleles as if they were certain; they are least certain where the table matters
most, at the long and rare end.  The model ("Cohort frequencies") estimates the allele frequencies of a locus
from the (h1, h2) surfaces of all its samples by EM, feeds them back to every sample as a Hardy-Weinberg prior and reports
posterior-weighted case, pre-risk and carrier counts; the evaluation runs on the GPU (csrc/cohort.hip, Engine.cohort).  Here:

    pack_cohort         [[trio.PairList-or-None per sample] per locus] -> the nested CSR of Context.cohort
    CohortResult        what comes back per locus
    run_cohort          the file pass: the `<key>.json` files of a run -> `<out>.json` and `<out>.calls.tsv`
    python -m tredparse_amd.cohort work/*.json --out work/cohort      the file pass from the command line

The pair lists are trio.PairList's, from a dense grid or from a file's `P_h1h2`.  The file pass inherits the limit of the
files: `P_h1h2` omits the pairs below e^-10 of the mode, so an allele that unlikely in every sample is not in the support.
Engine.cohort on dense grids has every pair.  The defaults of iters, alpha and tol are a choice, not a measurement: they are
options at every layer; exactly `iters` iterations run, and `converged` is a report (the last change below tol), not a control."""
import argparse
import json
import logging
import os
import sys

import numpy as np

from . import _lib
from .models import calc_label
from .trio import _file_list, pack_members


def pack_cohort(lists_per_locus, ploidy_per_locus):
    """The nested CSR of a cohort: item_off int64 [n_loci + 1] (the samples of a locus), samples = (off int64
    [n_samples + 1], a, b, lw) over all samples of all loci, ploidy int32 [n_samples], allele_off int64 [n_loci + 1] (room for
    the support of a locus: twice its pairs, 1 025 at the most) and the flat list of the members (None: takes no part).
    ploidy_per_locus: per locus one ploidy or one per sample."""
    if len(lists_per_locus) != len(ploidy_per_locus):
        raise ValueError("lists and ploidies must be of one length")
    members = [m if m is not None and len(m) else None for locus in lists_per_locus for m in locus]
    item_off = np.zeros(len(lists_per_locus) + 1, np.int64)
    item_off[1:] = np.cumsum([len(locus) for locus in lists_per_locus])
    ploidy = [np.broadcast_to(np.asarray(p, np.int32), (len(locus),)) for locus, p in zip(lists_per_locus, ploidy_per_locus)]
    ploidy = np.ascontiguousarray(np.concatenate(ploidy + [np.zeros(0, np.int32)]), np.int32)
    samples, _ = pack_members(members)
    pairs = samples[0][item_off]                                    # the pairs before each locus
    allele_off = np.zeros(len(lists_per_locus) + 1, np.int64)
    allele_off[1:] = np.cumsum(np.minimum(2 * np.diff(pairs), _lib.COHORT_MAX_ALLELE + 1))
    return item_off, samples, ploidy, allele_off, members


class CohortResult(object):
    """One locus: status (_lib.COHORT_*), alleles (the support, ascending), freq (f after the last iteration), count (the
    expected allele counts of the final E-step), C (chromosomes of the participating samples), n_samples (those samples),
    trace [iters][2] (sum of logZ under f_{t-1}, largest change of f), delta (the last change), converged (delta < tol),
    loglik (sum of logZ under the final f) and per sample of the locus -- None where it takes no part -- pairs (its
    PairList), index, call (a, b), post, logZ, r (its posterior over its pairs); ploidy per sample."""
    __slots__ = ("status", "alleles", "freq", "count", "C", "n_samples", "trace", "delta", "converged", "loglik", "pairs", "ploidy",
                 "index", "call", "post", "logZ", "r")

    def __init__(self, status, alleles, freq, count, trace, tol, pairs, ploidy, calls, values, r):
        self.status, self.alleles, self.freq, self.count, self.trace = int(status), alleles, freq, count, trace
        self.pairs, self.ploidy = pairs, [int(p) for p in ploidy]
        ok = self.status == _lib.COHORT_OK
        part = [ok and p is not None for p in pairs]
        self.n_samples = sum(part)
        self.C = sum(pl for pl, x in zip(self.ploidy, part) if x)
        self.delta = float(trace[-1, 1]) if ok else None
        self.converged = bool(self.delta < tol) if ok else False
        self.index = [int(c[0]) if x else None for c, x in zip(calls, part)]
        self.call = [(int(c[1]), int(c[2])) if x else None for c, x in zip(calls, part)]
        self.logZ = [float(v[0]) if x else None for v, x in zip(values, part)]
        self.post = [float(v[1]) if x else None for v, x in zip(values, part)]
        self.r = [rs if x else None for rs, x in zip(r, part)]
        self.loglik = float(np.cumsum([z for z in self.logZ if z is not None] or [0.0])[-1]) if ok else None

    def weight(self, s, select):
        """sum of r over the pairs (a, b) of sample s for which select(a, b) holds, 0.0 for a sample that takes no part."""
        if self.r[s] is None:
            return 0.0
        p = self.pairs[s]
        keep = np.array([bool(select(a, b)) for a, b in zip(p.a.tolist(), p.b.tolist())], bool)
        return float(self.r[s][keep].sum())


def is_carrier(tred, a, b):
    """tredreport's carrier rule for one pair: not labelled risk, and the longer allele past the disease cut-off (for
    contraction loci: at or below it)."""
    if calc_label(tred, [a, b]) == "risk":
        return False
    return b >= tred.cutoff_risk if tred.is_expansion else 0 < b <= tred.cutoff_risk


def results_of(n_items, item_off, samples, ploidy, allele_off, members, out, tol):
    """[CohortResult] of the outputs of one Context.cohort call (pack_cohort's arrays beside them)."""
    status, n_alleles, alleles, freq, count, trace, calls, values, r = out
    off = samples[0]
    res = []
    for i in range(n_items):
        lo, hi, j0 = int(item_off[i]), int(item_off[i + 1]), int(allele_off[i])
        j1 = j0 + int(n_alleles[i])
        res.append(CohortResult(status[i], alleles[j0:j1], freq[j0:j1], count[j0:j1], trace[i], tol, members[lo:hi], ploidy[lo:hi],
                                calls[lo:hi], values[lo:hi], [r[off[s]:off[s + 1]] for s in range(lo, hi)]))
    return res


def cohort_outputs(n_items, n_samples, n_pairs, room, iters):
    """The zeroed output arrays of Context.cohort, in its order."""
    return (np.zeros(n_items, np.int32), np.zeros(n_items, np.int32), np.zeros(room, np.int32), np.zeros(room, np.float64),
            np.zeros(room, np.float64), np.zeros((n_items, iters, 2), np.float64), np.zeros((n_samples, 3), np.int32),
            np.zeros((n_samples, 2), np.float64), np.zeros(n_pairs, np.float64))


# ---- the file pass ----------------------------------------------------------------------------------------------------
def _fmt(call):
    return "{}|{}".format(*call)


def run_cohort(paths, out, engine, repo, loci=None, iters=_lib.COHORT_ITERS, alpha=_lib.COHORT_ALPHA, tol=_lib.COHORT_TOL):
    """The file pass: the samples of the `<key>.json` files `paths`, in that order, at every locus of `loci` (default: all of
    repo) that one of the files has -- pair lists from `T.P_h1h2`, a sample's ploidy by the rule of the scan (inferredGender
    Male at an X-linked locus: 1, else the locus' own), a sample with no call at a locus takes no part there, ONE
    engine.cohort call for all loci.  Writes `<out>.json` (sorted keys, indent 4) and `<out>.calls.tsv` and returns the two
    paths."""
    docs = []
    for path in paths:
        with open(path) as fp:
            doc = json.load(fp)
        docs.append((doc.get("samplekey") or os.path.basename(path).rsplit(".json", 1)[0], doc["tredCalls"]))
    names = [n for n in (loci if loci is not None else repo.names) if any(n + ".1" in c for _, c in docs)]
    lists, ploidy = [], []
    for name in names:
        tred = repo[name]
        lists.append([_file_list(c, name) for _, c in docs])
        ploidy.append([1 if (c.get("inferredGender") == "Male" and tred.is_xlinked) else tred.ploidy for _, c in docs])
    results = engine.cohort(lists, ploidy, iters=iters, alpha=alpha, tol=tol) if names else []
    per_locus, rows = {}, []
    for name, r in zip(names, results):
        tred = repo[name]
        hard = {}
        for _, c in docs:
            for x in (c.get(name + ".1", -1), c.get(name + ".2", -1)):
                if isinstance(x, int) and x != -1:
                    hard[x] = hard.get(x, 0) + 1
        p_risk = [r.weight(s, lambda a, b: calc_label(tred, [a, b]) == "risk") for s in range(len(docs))]
        p_prerisk = [r.weight(s, lambda a, b: calc_label(tred, [a, b]) == "prerisk") for s in range(len(docs))]
        diploid = [s for s in range(len(docs)) if r.r[s] is not None and r.ploidy[s] == 2]
        per_locus[name] = {
            "status": _lib.COHORT_STATUS_NAMES[r.status], "alleles": [int(x) for x in r.alleles], "freq": [float(x) for x in r.freq],
            "count": [float(x) for x in r.count], "chromosomes": r.C, "n_samples": r.n_samples, "loglik": r.loglik,
            "delta": r.delta, "converged": r.converged, "exp_risk": float(sum(p_risk)), "exp_prerisk": float(sum(p_prerisk)),
            "exp_carrier": float(sum(r.weight(s, lambda a, b: is_carrier(tred, a, b)) for s in range(len(docs)))),
            "het_obs": float(sum(r.weight(s, lambda a, b: a != b) for s in diploid)),
            "het_exp": float(len(diploid) * (1.0 - float(np.sum(np.asarray(r.freq, np.float64) ** 2)))),
            "hard_freq": {str(k): hard[k] for k in sorted(hard)}}
        for s, (key, c) in enumerate(docs):
            if r.call[s] is None:
                continue
            rows.append([key, name, _fmt((c[name + ".1"], c[name + ".2"])), _fmt(r.call[s]), "{:.6g}".format(r.post[s]),
                         "{:.6g}".format(p_risk[s]), "{:.6g}".format(p_prerisk[s]), calc_label(tred, list(r.call[s]))])
    doc = {"params": {"iters": iters, "alpha": alpha, "tol": tol}, "samples": [key for key, _ in docs], "loci": per_locus}
    with open(out + ".json", "w") as fw:
        fw.write(json.dumps(doc, sort_keys=True, indent=4, separators=(",", ": ")) + "\n")
    with open(out + ".calls.tsv", "w") as fw:
        fw.write("\t".join(("SampleKey", "locus", "single", "call", "post", "P_risk", "P_prerisk", "label")) + "\n")
        for row in rows:
            fw.write("\t".join(row) + "\n")
    return [out + ".json", out + ".calls.tsv"]


def add_model_options(p, prefix=""):
    """--iters / --alpha / --tol (tred.py: --cohort-iters ...) of a parser."""
    for name, kind, default, text in (("iters", int, _lib.COHORT_ITERS, "EM iterations, all of them run (1 .. 4096)"),
                                      ("alpha", float, _lib.COHORT_ALPHA, "pseudo-chromosomes spread evenly over the alleles (> 0)"),
                                      ("tol", float, _lib.COHORT_TOL, "`converged` reports whether the last change of a frequency is below it")):
        p.add_argument("--{}{}".format(prefix, name), dest="cohort_" + name, type=kind, default=default,
                       help=text + "; a choice, not a measurement")


def main(argv=None):
    from .meta import BUILDS, TREDsRepo
    p = argparse.ArgumentParser(prog="python -m tredparse_amd.cohort", description="Cohort allele frequencies by EM and "
                                "population-aware calls from the <key>.json files of a run: <out>.json and <out>.calls.tsv",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("files", nargs="+", help="the samples' <key>.json files")
    p.add_argument("--out", default="cohort", help="prefix of the two files written")
    add_model_options(p)
    p.add_argument("--gpu", type=int, default=0, help="device index")
    p.add_argument("--tred", action="append", default=None, help="locus to evaluate (repeatable); all if omitted")
    p.add_argument("--ref", choices=BUILDS, default="hg38", help="genome build the BAMs were aligned to")
    p.add_argument("--haploid", action="append", help="contig that was treated as haploid (repeatable)")
    args = p.parse_args(argv)
    logging.basicConfig()
    from .engine import Engine
    repo = TREDsRepo(ref=args.ref)
    repo.set_ploidy(args.haploid)
    engine = Engine(args.gpu)
    try:
        for path in run_cohort(args.files, args.out, engine, repo, loci=args.tred, iters=args.cohort_iters, alpha=args.cohort_alpha,
                               tol=args.cohort_tol):
            print(path)
    finally:
        engine.close()


if __name__ == "__main__":
    main(sys.argv[1:])
