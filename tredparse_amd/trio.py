"""Trio-aware calls and de novo expansion odds: the host side of include/tredtrio.h.

Every sample is called alone; a family sequenced as a trio asks whether the child's long allele is inherited or newly
expanded, and from which parent.  The model ("Trio evaluation") couples the (h1, h2) surfaces of a child and
its parents through a transmission kernel; the evaluation runs on the GPU (csrc/trio.hip, Engine.trio).  Here:

    PairList            a member's surface as a list of allele pairs {a, b, lw}, built from a dense grid dump or from the
                        sparse `P_h1h2` of a `<key>.json` -- the one builder, with its two sources
    read_ped            the pedigree file
    TrioResult          what comes back per (trio, locus)
    run_pedigree        the file pass: the members' `<key>.json` of a working directory -> `<childkey>.trio.json`
    python -m tredparse_amd.trio family.ped --workdir work     the file pass from the command line

The file pass inherits the limit of the files: `P_h1h2` omits the pairs below e^-10 of the mode, so a parental allele that
unlikely is not there to be transmitted.  Engine.trio on dense grids has every pair.  The defaults of mu, rho and beta are a
choice, not a measurement: they are options at every layer."""
import argparse
import json
import logging
import os
import sys
from math import exp

import numpy as np

from . import _lib
from .models import calc_label

logger = logging.getLogger(__name__)
SMALL_VALUE = exp(-10)          # models.py:34: what `P_h1h2` keeps


class PairList(object):
    """The allele pairs of one member at one locus: a <= b in repeat units (int32) and lw, the log weight of the pair minus
    the list's largest (float64, <= 0)."""
    __slots__ = ("a", "b", "lw")

    def __init__(self, a, b, lw):
        self.a, self.b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
        self.lw = np.ascontiguousarray(lw, np.float64)
        if not len(self.a) == len(self.b) == len(self.lw):
            raise ValueError("a, b and lw of a pair list must be of one length")

    def __len__(self):
        return len(self.a)

    @classmethod
    def _build(cls, a, b, ml):
        ml = np.asarray(ml, np.float64)
        return cls(a, b, ml - ml.max() if len(ml) else ml)

    @classmethod
    def from_grid(cls, grid, period):
        """From a dense dump {h1, h2, ml1..ml4} (UnitResult.grid; h in bp): the first occurrence of every distinct
        (h1 // period, h2 // period) in enumeration order -- the grid can list a pair twice --, ml = ((ml1 + ml2) + ml3) + ml4."""
        grid = np.asarray(grid, np.float64).reshape(-1, 6)
        a, b = grid[:, 0].astype(np.int64) // period, grid[:, 1].astype(np.int64) // period
        _, first = np.unique(a * (int(b.max()) + 1 if len(b) else 1) + b, return_index=True)
        first.sort()
        ml = ((grid[:, 2] + grid[:, 3]) + grid[:, 4]) + grid[:, 5]
        return cls._build(a[first], b[first], ml[first])

    @classmethod
    def from_json(cls, dist):
        """From a `P_h1h2` dictionary {"a,b": v} of a `<key>.json` ("" or empty: no pair): the keys in ascending (a, b)
        order, lw = log v - max log v."""
        keys = sorted(tuple(int(x) for x in k.split(",")) for k in (dist or {}))
        return cls._build([k[0] for k in keys], [k[1] for k in keys], np.log([float(dist["%d,%d" % k]) for k in keys]))


def member_list(x, period=None):
    """A member of Engine.trio as a PairList, None for one that says nothing: None itself, a UnitResult whose call status is
    not 0, an empty list.  A UnitResult needs its dense grid (genotype_packed(dense=True)) and the locus' period."""
    if x is None:
        return None
    if not isinstance(x, PairList):
        if int(x.call["status"]) != 0:
            return None
        if x.grid is None or period is None:
            raise ValueError("a UnitResult goes into a trio with its dense grid (genotype_packed(b, dense=True)) and the period")
        x = PairList.from_grid(x.grid, int(period))
    return x if len(x) else None


def pack_members(members):
    """CSR (off int64 [n + 1], a, b, lw) of a list of PairList-or-None, and int32 [n]: 1 where there is a list."""
    off = np.zeros(len(members) + 1, np.int64)
    off[1:] = np.cumsum([0 if m is None else len(m) for m in members])
    cat = lambda name, dt: np.ascontiguousarray(np.concatenate([getattr(m, name) for m in members if m is not None] + [np.zeros(0, dt)]), dt)
    return (off, cat("a", np.int32), cat("b", np.int32), cat("lw", np.float64)), np.array([m is not None for m in members], np.int32)


class TrioResult(object):
    """One (trio, locus): status (_lib.TRIO_*), index (of the call in the child's list), call (a, b) in repeat units,
    post (the call's posterior), denovo and paternal (None when the status is DEGENERATE), Jmax, S, J (per pair of the
    child's list) and pairs, that list.  A child without a pair (EMPTY_CHILD) has call (-1, -1) and None elsewhere."""
    __slots__ = ("status", "index", "call", "post", "denovo", "paternal", "Jmax", "S", "J", "pairs")

    def __init__(self, status, call, values, J, pairs):
        self.status, self.J, self.pairs = int(status), J, pairs
        self.index, self.call = int(call[0]), (int(call[1]), int(call[2]))
        self.Jmax, self.S = float(values[0]), float(values[1])
        self.post = self.denovo = self.paternal = None
        if self.status == _lib.TRIO_EMPTY_CHILD:
            self.call = (-1, -1)
        if self.status in (_lib.TRIO_OK, _lib.TRIO_DEGENERATE):
            self.post = 1.0 / self.S
        if self.status == _lib.TRIO_OK:
            self.denovo, self.paternal = float(values[2]), float(values[3])

    def P_h1h2(self):
        """The trio-aware joint distribution as the single-sample `P_h1h2` is printed (models.py:304-317): the pairs with
        exp(J - Jmax) >= e^-10, over the sum of all; "" without a call."""
        if self.status not in (_lib.TRIO_OK, _lib.TRIO_DEGENERATE):
            return ""
        v = np.exp(self.J - self.Jmax)
        keep = np.nonzero(v >= SMALL_VALUE)[0]
        return {"%d,%d" % (a, b): float(p) for a, b, p in zip(self.pairs.a[keep].tolist(), self.pairs.b[keep].tolist(), v[keep] / self.S)}

    def label(self, tred):
        """The risk label of the trio-aware call, by the rule of the single-sample label."""
        return calc_label(tred, list(self.call))

    def to_dict(self, tred=None, single=None):
        """What `<childkey>.trio.json` holds per locus (label with tred, single with the file's own call)."""
        out = {"call": list(self.call), "post": self.post, "denovo": self.denovo, "paternal": self.paternal,
               "P_h1h2": self.P_h1h2(), "status": _lib.TRIO_STATUS_NAMES[self.status]}
        if tred is not None:
            out["label"] = self.label(tred)
        if single is not None:
            out["single"] = list(single)
        return out


# ---- the pedigree file ------------------------------------------------------------------------------------------------
class Person(object):
    """One line of a PED file: family, key (the sample key), father, mother (keys, None for `0`), sex (1 male, 2 female,
    anything else unknown), phenotype."""
    __slots__ = ("family", "key", "father", "mother", "sex", "phenotype")

    def __init__(self, family, key, father, mother, sex, phenotype):
        self.family, self.key, self.sex, self.phenotype = family, key, sex, phenotype
        self.father, self.mother = (None if x == "0" else x for x in (father, mother))


def read_ped(lines):
    """[Person] of a PED file (a path, or its lines): six whitespace-separated columns, `#` comments and blank lines
    skipped.  The second column is the sample key, `0` a missing parent; a child with one parent (a duo) is allowed.
    ValueError for another column count, a key listed twice and a child listed as its own parent."""
    if isinstance(lines, str):
        with open(lines) as fp:
            lines = fp.read().splitlines()
    people, seen = [], set()
    for no, line in enumerate(lines, 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        cells = line.split()
        if len(cells) != 6:
            raise ValueError("PED line {}: {} columns, not 6".format(no, len(cells)))
        p = Person(*cells)
        if p.key in (p.father, p.mother):
            raise ValueError("PED line {}: `{}` is listed as its own parent".format(no, p.key))
        if p.key in seen:
            raise ValueError("PED line {}: `{}` is listed twice".format(no, p.key))
        seen.add(p.key)
        people.append(p)
    return people


# ---- the file pass ----------------------------------------------------------------------------------------------------
_PED_SEX = {"1": "Male", "2": "Female"}


def _load_calls(key, workdir):
    """tredCalls of `<key>.json`, None (with a warning) where the file is not there."""
    path = os.path.join(workdir, key + ".json")
    if not os.path.exists(path):
        logger.warning("pedigree member `%s` has no %s: it says nothing", key, path)
        return None
    with open(path) as fp:
        return json.load(fp)["tredCalls"]


def _file_list(calls, name):
    """The member's PairList at locus `name` from its file, None where it has no call there."""
    if calls is None or calls.get(name + ".1", -1) == -1:
        return None
    return member_list(PairList.from_json(calls.get(name + ".P_h1h2")))


def run_pedigree(ped, workdir, engine, repo, loci=None, mu=_lib.TRIO_MU, rho=_lib.TRIO_RHO, beta=_lib.TRIO_BETA):
    """The file pass: every child of the pedigree (a member with at least one parent named) against its parents, at every
    locus of `loci` (default: all of repo) its own `<key>.json` in workdir has -- pair lists from `T.P_h1h2`, the child's
    ploidy by the rule of the scan (inferredGender Male at an X-linked locus: 1, else the locus' own), ONE engine.trio call
    for the whole pedigree, one `<childkey>.trio.json` per child (sorted keys, indent 4).  Returns the paths written."""
    people = read_ped(ped)
    calls = {}
    for p in people:
        if p.father or p.mother:
            for key in (p.key, p.father, p.mother):
                if key is not None and key not in calls:
                    calls[key] = _load_calls(key, workdir)
    for p in people:
        c = calls.get(p.key)
        if c is not None and p.sex in _PED_SEX and c.get("inferredGender") in _PED_SEX.values() and _PED_SEX[p.sex] != c["inferredGender"]:
            logger.warning("`%s`: the pedigree says %s, the reads say %s", p.key, _PED_SEX[p.sex], c["inferredGender"])
    names = list(loci if loci is not None else repo.names)
    items, children, fathers, mothers, ploidy = [], [], [], [], []
    for p in people:
        c = calls.get(p.key)
        if not (p.father or p.mother) or c is None:
            continue
        for name in names:
            if name + ".1" not in c:
                continue
            tred = repo[name]
            items.append((p, name))
            children.append(_file_list(c, name) or PairList([], [], []))
            fathers.append(_file_list(calls.get(p.father), name))
            mothers.append(_file_list(calls.get(p.mother), name))
            ploidy.append(1 if (c.get("inferredGender") == "Male" and tred.is_xlinked) else tred.ploidy)
    results = engine.trio(children, fathers, mothers, ploidy, mu=mu, rho=rho, beta=beta) if items else []
    per_child = {}
    for (p, name), r in zip(items, results):
        c = calls[p.key]
        per_child.setdefault(p.key, {})[name] = r.to_dict(repo[name], single=(c[name + ".1"], c[name + ".2"]))
    written = []
    for p in people:
        if p.key not in per_child:
            continue
        doc = {"samplekey": p.key, "father": p.father, "mother": p.mother, "params": {"mu": mu, "rho": rho, "beta": beta},
               "loci": per_child[p.key]}
        path = os.path.join(workdir, p.key + ".trio.json")
        with open(path, "w") as fw:
            fw.write(json.dumps(doc, sort_keys=True, indent=4, separators=(",", ": ")) + "\n")
        written.append(path)
    return written


def add_model_options(p, prefix=""):
    """--mu / --rho / --beta (tred.py: --trio-mu ...) of a parser."""
    for name, default, text in (("mu", _lib.TRIO_MU, "probability that a transmission changes the allele (0 < mu < 1)"),
                                ("rho", _lib.TRIO_RHO, "geometric ratio of the size of a change (0 < rho < 1)"),
                                ("beta", _lib.TRIO_BETA, "share of the changes that are expansions (0 <= beta <= 1)")):
        p.add_argument("--{}{}".format(prefix, name), dest="trio_" + name, type=float, default=default,
                       help=text + "; a choice, not a measurement")


def main(argv=None):
    from .meta import BUILDS, TREDsRepo
    p = argparse.ArgumentParser(prog="python -m tredparse_amd.trio", description="Trio-aware calls and de novo expansion odds "
                                "from the <key>.json files of a working directory: one <childkey>.trio.json per child",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("pedigree", help="PED file: family, sample key, father, mother, sex, phenotype; 0 for a missing parent")
    p.add_argument("--workdir", default=os.getcwd(), help="directory of the <key>.json files and of the outputs")
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
        for path in run_pedigree(args.pedigree, args.workdir, engine, repo, loci=args.tred, mu=args.trio_mu, rho=args.trio_rho,
                                 beta=args.trio_beta):
            print(path)
    finally:
        engine.close()


if __name__ == "__main__":
    main(sys.argv[1:])
