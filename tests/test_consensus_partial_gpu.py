"""GPU: Engine.consensus(partial=True) and tred.py --consensus-partial -- the reads anchored in one flank laid on the
longest allele asked for, so that an allele longer than the reads is covered.  t001 / HD's allele 41 against the table
derived from the text of the reference's own report, interruptions planted in alleles no read spans found from the side
that reaches them, the long-read path against tests/pileup_anchored_model.py, and the command line."""
import json
import os
import random

import numpy as np
import pytest

from tredparse_amd import _lib, tred as tredmod
from tredparse_amd.engine import Engine, PackedUnits

from . import pileup_anchored_model as am
from . import pileup_model as pm
from .test_consensus_gpu import GOLD, NAME, PREFIX, SUFFIX, T001, _run, _t001_units, _unit, engine, hd, long_bam  # noqa: F401
from .test_long_reads_e2e_gpu import LONG_SAMPLES
from .test_pileup_anchored_model import t001_partial_table

pytestmark = pytest.mark.gpu
P, p, S = 18, 3, 18
T41 = PREFIX + "CAG" * 41 + SUFFIX


def _model(al, locus, alleles):
    """{a: (table, reads, partial, ambiguous, beyond)} of one unit from its alignments (Engine.alignments), by the model."""
    prefix, repeat, suffix = locus
    Pl, pl, Sl = len(prefix), len(repeat), len(suffix)
    out = {a: [pm.table(Pl + pl * a + Sl), 0, 0, 0, 0] for a in alleles}
    for x in al.values():
        kind, a = am.place(_lib.TAG_NAMES[x.tag], x.h, alleles)
        if kind is None:
            continue
        out[a][{"whole": 1, "partial": 2, "ambiguous": 3, "beyond": 4}[kind]] += 1
        if kind in ("whole", "partial"):
            f = [x.al.score, x.al.ref_begin, x.al.ref_end, x.al.query_begin, x.al.query_end]
            am.add_item_anchored(out[a][0], Pl, pl, Sl, x.h, a, x.strand, am.ANCHOR_OF_TAG[_lib.TAG_NAMES[x.tag]], x.al.query_seq,
                                 f, x.al._cigar_string)
    return out


def _same(x, T, want, Pl, pl):
    table, reads, partial, ambiguous, beyond = want
    assert (x.reads, x.partial, x.ambiguous, x.beyond) == (reads, partial, ambiguous, beyond)
    assert x.counts.dtype == np.int32 and x.counts.shape == (len(T) + 1, 8) and x.counts.tolist() == table
    c = pm.consensus_of(table, T, Pl, pl, x.h)
    assert (x.consensus, [int(v) for v in x.depth], x.interruptions, x.insertions) == (c["consensus"], c["depth"],
                                                                                    c["interruptions"], c["insertions"])


# ---- (e) t001 / HD ----------------------------------------------------------------------------------------------------
def test_t001_hd_allele_41_is_covered_by_its_partial_reads(engine):
    text, _, n = t001_partial_table()
    units = _t001_units()
    old = engine.consensus(units, [[15, 41]])
    engine.ctx.reset_timing()
    res = engine.consensus(units, [[15, 41]], partial=True)
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1 and engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1
    assert len(res) == 1 and sorted(res[0]) == [15, 41]
    y = res[0][41]
    assert (y.h, y.reads, y.partial, y.ambiguous, y.beyond) == (41, 0, 7, 14, 0) == (41, 0, n["partial"], n["ambiguous"], n["beyond"])
    assert y.counts.shape == (len(T41) + 1, 8) and y.counts.tolist() == text
    assert y.consensus == T41 and (int(y.depth.min()), int(y.depth.max())) == (3, 6)
    assert y.interruptions == [] and y.insertions == []
    # the shorter allele is what it was: its FULL reads, and no partial read can be told to be its own
    x, was = res[0][15], old[0][15]
    assert (x.reads, x.partial, x.ambiguous, x.beyond) == (4, 0, 0, 0) and np.array_equal(x.counts, was.counts)
    assert x.to_dict() == was.to_dict() and x.to_dict(partial=True) == dict(was.to_dict(), partial=0, ambiguous=0, beyond=0)
    # without the argument the result is the old one
    again = engine.consensus(units, [[15, 41]])
    assert again[0][41].consensus == T41.lower() and again[0][41].reads == 0 and not again[0][41].counts.any()
    assert again[0][41].to_dict() == old[0][41].to_dict() and again[0][15].to_dict() == was.to_dict()
    # the shared step handed over
    w = engine.winners(units)
    engine.ctx.reset_timing()
    both = engine.consensus(units, [[15, 41]], winners=w, partial=True)
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1 and engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0
    assert both[0][41].counts.tolist() == text


# ---- (f) an interruption in an allele no read spans ----------------------------------------------------------------------
LEFT, RIGHT = (0, 7, 14), (0, 7, 14, 20)        # flank letters in front of the prefix / behind the suffix of the 150 bp reads
# what bam_parser.py:123-182 says of the reads of _flank_reads (the oracle's classify, run on the CPU when this was written):
# a left read and its reverse complement, cut by cut, then the right ones
TAGS = [_lib.TAG_PREF, _lib.TAG_POST] * 3 + [_lib.TAG_POST, _lib.TAG_PREF] * 4
HS = [44, 44, 41, 41, 39, 39, 44, 44, 42, 42, 40, 40, 38, 38]


def _planted(a, at):
    units = ["CAG"] * a
    for k in at:
        units[k - 1] = "CAA"
    return PREFIX + "".join(units) + SUFFIX


def _flank_reads(text, seed=5, L=150):
    """150 bp reads cut from 40 random letters + text + 40 random letters: from x letters before the prefix on, and up
    to y letters behind the suffix, each with its reverse complement."""
    rnd = random.Random(seed)
    G = "".join(rnd.choice("ACGT") for _ in range(40)) + text + "".join(rnd.choice("ACGT") for _ in range(40))
    out = []
    for x in LEFT:
        s = G[40 - x:40 - x + L]
        out += [s, pm.revcomp(s)]
    for y in RIGHT:
        s = G[len(G) - 40 + y - L:len(G) - 40 + y]
        out += [s, pm.revcomp(s)]
    return out


def _flank_case(engine, hd, a, at):
    text = _planted(a, at)
    reads = _flank_reads(text)
    assert len(reads) == 14 and all(len(r) == 150 for r in reads)
    units = [_unit(hd, reads)]
    tag, h, _, _, _ = engine.classify(units)
    assert tag.tolist() == TAGS and h.tolist() == HS, (tag, h)          # a tagging surprise shows here
    x = engine.consensus(units, [[a]], partial=True)[0][a]
    want = _model(engine.alignments(units)[0], (PREFIX, "CAG", SUFFIX), [a])[a]
    _same(x, PREFIX + "CAG" * a + SUFFIX, want, P, p)
    assert (x.reads, x.partial, x.ambiguous, x.beyond) == (0, 14, 0, 0) and x.insertions == []
    assert engine.consensus(units, [[a]])[0][a].consensus == (PREFIX + "CAG" * a + SUFFIX).lower()
    return text, x


def test_planted_interruptions_are_found_from_the_side_that_reaches_them(engine, hd):
    text, x = _flank_case(engine, hd, 60, (3, 30, 58))
    assert x.consensus == text                                           # every column is reached from one side at least
    hit = lambda unit, n: {"unit": unit, "offset": 2, "ref": "G", "alt": "A", "support": n, "depth": n}
    # unit 3: the six reads from the left; unit 58: the eight from the right; unit 30: all of them
    assert x.interruptions == [hit(3, 6), hit(30, 14), hit(58, 8)]
    assert int(x.depth[P - 1]) == 6 and int(x.depth[len(text) - S]) == 8


def test_the_middle_nobody_reaches_stays_lower_case(engine, hd):
    a = 120
    text, x = _flank_case(engine, hd, a, (3, 118))
    hit = lambda unit, n: {"unit": unit, "offset": 2, "ref": "G", "alt": "A", "support": n, "depth": n}
    assert x.interruptions == [hit(3, 6), hit(118, 8)]
    # the left reads end in unit 44 at the latest, the right ones begin in unit a - 44 + 1 at the earliest
    lo, hi = P + p * 44, P + p * (a - 44)
    assert not x.depth[lo:hi].any() and x.consensus[lo:hi] == ("CAG" * a)[:hi - lo].lower() and not x.counts[lo + 1:hi].any()
    assert x.depth[lo - 1] > 0 and x.depth[hi] > 0 and x.consensus[:lo] == text[:lo] and x.consensus[hi:] == text[hi:]


# ---- (h) the long path ---------------------------------------------------------------------------------------------------
def test_long_reads_partial_consensus_equals_the_model(long_bam):
    golden = json.load(open(os.path.join(GOLD, "alignments_" + NAME + ".json")))["loci"]
    from tredparse_amd.meta import TREDsRepo
    e = Engine(0, long_reads=True)
    try:
        repo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
        scan = tredmod.collect_sample((NAME, long_bam, repo, LONG_SAMPLES[NAME][0], 300, False, False, True, True, "INFO"),
                                      long_reads=True)
        ks = [k for k, n in enumerate(scan.names) if n in golden]
        units = PackedUnits.from_scans([(scan, ks)])
        w = e.winners(units)
        al = e.alignments(units, winners=w)
        # the alleles the FULL reads show, or, of a locus no read spans, the longest a partial read was tagged with
        alleles = [sorted({x.h for x in a.values() if x.tag == _lib.TAG_FULL}) or
                   [max(x.h for x in a.values() if x.tag in (_lib.TAG_PREF, _lib.TAG_POST))] for a in al]
        e.ctx.reset_timing()
        res = e.consensus(units, alleles, winners=w, partial=True)
        assert e.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
        placed = unspanned = 0
        for k, a, r, want in zip(ks, al, res, alleles):
            t = scan.loci[k]
            model = _model(a, (t.prefix, t.repeat, t.suffix), want)
            assert sorted(r) == want
            for h in want:
                _same(r[h], t.prefix + t.repeat * h + t.suffix, model[h], len(t.prefix), len(t.repeat))
                placed += r[h].partial
                unspanned += r[h].reads == 0 and r[h].partial > 0 and r[h].depth.any()
        assert placed >= 2 and unspanned >= 1          # (HD: two reads between its alleles; SCA10: no FULL read at all)
    finally:
        e.close()


# ---- (g) the command line ------------------------------------------------------------------------------------------------
def test_cli_consensus_partial(engine, tmp_path, capsys, monkeypatch):
    text, _, n = t001_partial_table()
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    engine.ctx.reset_timing()
    plain = _run(tmp_path / "plain", capsys, "--consensus")
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
    one = _run(tmp_path / "one", capsys, "--consensus-partial")
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 2 and engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 2
    two = _run(tmp_path / "two", capsys, "--consensus-partial")
    assert one == two == plain
    assert sorted(os.listdir(tmp_path / "one")) == ["t001.consensus.json", "t001.json", "t001.tred.vcf.gz"]
    got_text = (tmp_path / "one" / "t001.consensus.json").read_bytes()
    assert got_text == (tmp_path / "two" / "t001.consensus.json").read_bytes()
    assert (tmp_path / "one" / "t001.json").read_bytes() == (tmp_path / "plain" / "t001.json").read_bytes()
    got = json.loads(got_text)
    old = json.loads((tmp_path / "plain" / "t001.consensus.json").read_text())
    assert got_text == (json.dumps(got, sort_keys=True, indent=1) + "\n").encode()
    assert list(got) == ["HD"] and [x["h"] for x in got["HD"]["alleles"]] == [15, 41]
    assert "partial" not in old["HD"]["alleles"][0] and "ambiguous" not in old["HD"]["alleles"][1]
    assert got["HD"]["alleles"][0] == dict(old["HD"]["alleles"][0], partial=0, ambiguous=0, beyond=0)
    want = pm.consensus_of(text, T41, P, p, 41)
    assert want["consensus"] == T41 and min(want["depth"]) == 3
    assert got["HD"]["alleles"][1] == dict(want, h=41, reads=0, partial=n["partial"], ambiguous=n["ambiguous"], beyond=0)
    # with --alignments: one CIGAR call and one pileup call, and both files what they are alone
    engine.ctx.reset_timing()
    _run(tmp_path / "both", capsys, "--consensus-partial", "--alignments")
    assert engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1 and engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
    assert (tmp_path / "both" / "t001.consensus.json").read_bytes() == got_text
    with open(os.path.join(GOLD, "alignments_t001_HD.txt"), "rb") as fp:
        assert (tmp_path / "both" / "t001.alignments.txt").read_bytes() == fp.read()
    # --consensus beside it changes nothing
    _run(tmp_path / "either", capsys, "--consensus", "--consensus-partial")
    assert (tmp_path / "either" / "t001.consensus.json").read_bytes() == got_text
