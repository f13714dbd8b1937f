"""GPU: Engine.spectrum -- the repeat-unit words of a locus' reads, the in-repeat ones included.  t001 / HD against
tests/spectrum_model.py on Engine.winners' own arrays and against the text of the reference's own report; CCG planted in
an allele of 120 units and found by the reads from inside the tract; the long-read path; a period without a table; the
shared step handed over."""
import collections
import json
import os
import random

import numpy as np
import pytest

from tredparse_amd import _lib, tred as tredmod
from tredparse_amd.engine import Engine, PackedUnits
from tredparse_amd.meta import TREDsRepo

from . import pileup_model as pm
from . import spectrum_model as sm
from .test_consensus_gpu import GOLD, NAME, PREFIX, SUFFIX, _t001_units, _unit, engine, hd, long_bam  # noqa: F401
from .test_long_reads_e2e_gpu import LONG_SAMPLES

pytestmark = pytest.mark.gpu
CLASS_OF = {_lib.TAG_PREF: "partial", _lib.TAG_POST: "partial", _lib.TAG_REPT: "rept"}


def model_classes(w, alleles):
    """Per unit {class: dict} by the model, from the arrays Engine.winners returned: the read's text, the winning
    template, its fields and the operations of sw_cigar."""
    b = w.batch
    out = []
    for g in range(b.n_units):
        names = ["full:{}".format(a) for a in sorted(set(int(x) for x in alleles[g] if int(x) >= 1))] + ["partial", "rept"]
        out.append({n: dict(reads=0, units=0, with_n=0, touched=0, words=collections.Counter(), interrupted_reads=0) for n in names})
    for j in range(len(w.items)):
        g, t = int(w.unit_of[j]), int(w.tag[j])
        name = "full:{}".format(int(w.h[j])) if t == _lib.TAG_FULL else CLASS_OF.get(t)
        if name not in out[g]:
            continue
        prefix, repeat, suffix, _ = b.ladder_keys[g]
        words, touched = sm.item_units(len(prefix), len(repeat), len(suffix), int(w.win[j]), b.text(int(w.items[j])),
                                       [int(v) for v in w.fields[j]], [int(v) for v in w.ops[j, :w.n_ops[j]]])
        free = [x for x in words if "N" not in x]
        c = out[g][name]
        c["reads"] += 1
        c["units"] += len(free)
        c["with_n"] += len(words) - len(free)
        c["touched"] += touched
        c["words"].update(free)
        c["interrupted_reads"] += any(x != repeat for x in free)
    return out


def same(got, want, repeat):
    """A RepeatSpectrum against model_classes' entry of its unit."""
    assert sorted(got.classes) == sorted(want) and got.motif == repeat and got.period == len(repeat) and not got.unsupported
    for name, c in want.items():
        x = got.classes[name]
        assert (x.reads, x.units, x.with_n, x.touched, x.interrupted_reads) == (c["reads"], c["units"], c["with_n"], c["touched"],
                                                                               c["interrupted_reads"]), name
        assert x.words == dict(c["words"]) and list(x.words.items()) == sorted(c["words"].items(), key=lambda kv: (-kv[1], kv[0]))
        assert x.purity == (None if c["units"] == 0 else c["words"][repeat] / c["units"])


def test_t001_hd_equals_the_model_and_the_golden_reports_text(engine):
    units = _t001_units()
    engine.ctx.reset_timing()
    res = engine.spectrum(units, [[15, 41, 41, 0, -1]])
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1 and engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1
    assert len(res) == 1 and sorted(res[0].classes) == ["full:15", "full:41", "partial", "rept"]
    w = engine.winners(units)
    same(res[0], model_classes(w, [[15, 41]])[0], "CAG")
    # the FULL reads of the report, from its text alone
    with open(os.path.join(GOLD, "alignments_t001_HD.txt")) as fp:
        blocks = pm.parse_blocks(fp.read())
    words, touched = collections.Counter(), 0
    for b in blocks:
        if b["tag"] == "FULL":
            ws, t = sm.from_lines(len(PREFIX), 3, len(SUFFIX), b["units"], b["strand"], b["fields"][1], b["lines"][0], b["lines"][2])
            words.update(ws)
            touched += t
    full = res[0].classes["full:15"]
    assert full.reads == 4 and full.words == dict(words) and full.touched == touched == 60 and full.with_n == 0
    assert res[0].classes["full:41"].reads == 0 and res[0].classes["full:41"].purity is None
    part = sum(b["tag"] in ("PREF", "POST") for b in blocks)
    assert res[0].classes["partial"].reads == part == 21 and res[0].classes["partial"].units > 300
    # the shared step handed over: no second CIGAR call, the same result
    engine.ctx.reset_timing()
    again = engine.spectrum(units, [[15, 41]], winners=w)
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1 and engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0
    assert again[0].to_dict() == res[0].to_dict()
    assert json.loads(json.dumps(res[0].to_dict(), sort_keys=True)) == res[0].to_dict()


# ---- CCG planted in every tenth unit of an allele of 120 units ----------------------------------------------------------
def _tract(a, every=None):
    return "".join("CCG" if every and (k + 1) % every == 0 else "CAG" for k in range(a))


def _cut_reads(a120, L=150):
    """150 bp reads, each with its reverse complement: spanning reads of the 15-unit allele, reads cut from both flanks
    of the 120-unit allele, and reads from inside its tract -- beginning on a unit boundary and one and two letters
    behind one, every planted unit at least four units away from the ends of a read."""
    rnd = random.Random(7)
    flank = lambda: "".join(rnd.choice("ACGT") for _ in range(60))
    short = flank() + PREFIX + "CAG" * 15 + SUFFIX + flank()
    long_ = flank() + PREFIX + a120 + SUFFIX + flank()
    out, inside = [], []
    for x in (20, 30):
        out.append(short[x:x + L])
    for x in (45, 52):                                        # from the prefix into the tract; from the tract into the suffix
        out.append(long_[x:x + L])
        out.append(long_[len(long_) - x - L:len(long_) - x])
    t0 = 60 + len(PREFIX)
    for unit, phase in ((4, 0), (14, 1), (25, 2), (34, 0), (45, 1), (64, 2)):
        inside.append(long_[t0 + 3 * unit + phase:t0 + 3 * unit + phase + L])
    both = lambda rs: [s for r in rs for s in (r, pm.revcomp(r))]
    return both(out), both(inside)


def test_ccg_in_every_tenth_unit_of_an_allele_no_read_spans(engine, hd):
    outer, inside = _cut_reads(_tract(120, every=10))
    assert len(inside) == 12 and all(len(r) == 150 for r in outer + inside)
    planted = sum("CCG" in r or "CGG" in r for r in inside)
    assert planted == 12
    units = [_unit(hd, outer + inside)]
    w = engine.winners(units)
    res = engine.spectrum(units, [[15, 120]], winners=w)[0]
    want = model_classes(w, [[15, 120]])[0]
    same(res, want, "CAG")
    rept = res.classes["rept"]
    assert rept.reads == 12, (w.tag.tolist(), w.h.tolist())            # a tagging surprise shows here
    assert set(rept.words) == {"CAG", "CCG"} and rept.words["CCG"] == want["rept"]["words"]["CCG"] >= 4 * 12
    assert rept.words["CAG"] == want["rept"]["words"]["CAG"] and rept.purity < 1 and rept.interrupted_reads == planted
    assert res.classes["full:15"].reads == 4 and res.classes["full:15"].purity == 1.0
    assert res.classes["full:120"].reads == 0 and res.classes["partial"].reads == 8
    assert res.classes["partial"].words.get("CCG", 0) >= 8             # every flank read reaches the 10th unit from its end
    # the same reads cut from a pure tract
    outer, inside = _cut_reads(_tract(120))
    clean = engine.spectrum([_unit(hd, outer + inside)], [[15, 120]])[0]
    for name in ("full:15", "partial", "rept"):
        c = clean.classes[name]
        assert c.purity == 1.0 and c.words == {"CAG": c.units} and c.interrupted_reads == 0 and c.units > 0, name
    assert clean.classes["rept"].reads == 12


# ---- the long path ------------------------------------------------------------------------------------------------------
def test_long_reads_spectrum_equals_the_model(long_bam):
    golden = json.load(open(os.path.join(GOLD, "alignments_" + NAME + ".json")))["loci"]
    e = Engine(0, long_reads=True)
    try:
        repo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
        scan = tredmod.collect_sample((NAME, long_bam, repo, LONG_SAMPLES[NAME][0], 300, False, False, True, True, "INFO"),
                                      long_reads=True)
        ks = [k for k, n in enumerate(scan.names) if n in golden]
        units = PackedUnits.from_scans([(scan, ks)])
        w = e.winners(units)
        alleles = [sorted({int(h) for h, t, u in zip(w.h, w.tag, w.unit_of) if t == _lib.TAG_FULL and u == g}) for g in range(len(ks))]
        e.ctx.reset_timing()
        res = e.spectrum(units, alleles, winners=w)
        assert e.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1 and e.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0
        want = model_classes(w, alleles)
        n_units = 0
        for k, r, m in zip(ks, res, want):
            same(r, m, scan.loci[k].repeat)
            n_units += sum(c.units for c in r.classes.values())
        assert n_units > 0 and int(w.read_len.max()) > 480            # something was counted, and on the long path
    finally:
        e.close()


# ---- a period without a table, next to one with ---------------------------------------------------------------------------
def test_a_dodecamer_comes_back_unsupported_and_nothing_of_it_is_sent(engine, hd):
    uld = TREDsRepo(ref="hg38")["ULD"]
    assert len(uld.repeat) == 12
    rnd = random.Random(3)
    flank = "".join(rnd.choice("ACGT") for _ in range(40))
    text = flank + uld.prefix + uld.repeat * 3 + uld.suffix + flank
    reads = [text[20:170], pm.revcomp(text[20:170])]
    from tredparse_amd.engine import Unit
    u = Unit(uld, 150, reads, 30.0, 2, (), ())
    assert (engine.classify([u])[0] != _lib.TAG_NONE).any()             # its reads are tagged: they are held back, not missing
    engine.ctx.reset_timing()
    res = engine.spectrum([u], [[3]])
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 0            # no call at all
    assert res[0].unsupported and res[0].to_dict() == {"motif": uld.repeat, "period": 12, "unsupported": True}
    outer, inside = _cut_reads(_tract(120))
    engine.ctx.reset_timing()
    res = engine.spectrum([u, _unit(hd, outer + inside), u], [[3], [15], [3]])
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
    assert res[0].unsupported and res[2].unsupported and not res[1].unsupported
    assert sum(c.reads for c in res[1].classes.values()) == len(outer + inside)     # every item sent is the HD unit's
    assert res[1].classes["rept"].purity == 1.0
