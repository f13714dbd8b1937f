"""GPU: Engine.consensus and tred.py --consensus -- the reads that span an allele, laid on its template and read column
by column.  t001 / HD against the pileup derived from the text of the reference's own report
(tests/golden/alignments_t001_HD.txt), planted interruptions (CAA in a CAG tract) found where they were planted, mixed
evidence on both sides of `more than half`, the long-read path against tests/pileup_model.py, and the command line."""
import json
import os
import random

import numpy as np
import pytest

from tredparse_amd import _lib, synth, synth_bam, tred as tredmod
from tredparse_amd.engine import Engine, PackedUnits, Unit
from tredparse_amd.meta import TREDsRepo

from . import pileup_model as pm
from .test_long_reads_e2e_gpu import LONG_SAMPLES

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PREFIX, SUFFIX = "GAGTCCCTCAAGTCCTTC", "CAACAGCCGCCACCGCCG"
T001 = ("t001", os.path.join(GOLD, "bam", "t001.bam"))


@pytest.fixture(scope="module")
def engine(ctx):
    return Engine(ctx=ctx)            # on the session's context (tests/conftest.py: it loads PyTorch's HIP runtime first)


@pytest.fixture(scope="module")
def hd():
    t = TREDsRepo(ref="hg38")["HD"]
    assert (t.prefix, t.repeat, t.suffix) == (PREFIX, "CAG", SUFFIX)
    return t


@pytest.fixture(scope="module")
def t001_want():
    """What the golden report says of allele 15 of t001 / HD: the pileup of its four FULL blocks, from their text."""
    with open(os.path.join(GOLD, "alignments_t001_HD.txt")) as fp:
        blocks = [b for b in pm.parse_blocks(fp.read()) if b["tag"] == "FULL"]
    assert len(blocks) == 4 and all(b["h"] == 15 for b in blocks)
    T = PREFIX + "CAG" * 15 + SUFFIX
    table = pm.table(len(T))
    for b in blocks:
        assert (pm.revcomp(b["target"]) if b["strand"] else b["target"]) == T
        pm.from_lines(table, len(T), b["strand"], b["fields"][1], b["lines"][0], b["lines"][2])
    return T, table, pm.consensus_of(table, T, len(PREFIX), 3, 15)


def _same(x, T, table, want, reads):
    assert x.reads == reads and x.counts.dtype == np.int32 and x.counts.shape == (len(T) + 1, 8)
    assert x.counts.tolist() == table
    assert (x.consensus, [int(v) for v in x.depth], x.interruptions, x.insertions) == (want["consensus"], want["depth"],
                                                                                    want["interruptions"], want["insertions"])


def _t001_units():
    from tredparse_amd.runtime import collect_sample
    scan = collect_sample(T001 + (TREDsRepo(ref="hg38"), ["HD"], 300, False, False, True, True, "INFO"))
    return PackedUnits.from_scans([(scan, [0])])


def test_t001_hd_equals_the_pileup_of_the_golden_reports_text(engine, t001_want):
    T, table, want = t001_want
    units = _t001_units()
    engine.ctx.reset_timing()
    res = engine.consensus(units, [[15, 41, 41, 0, -1]])
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1 and engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1
    assert len(res) == 1 and sorted(res[0]) == [15, 41]
    x = res[0][15]
    assert x.h == 15 and want["depth"][len(PREFIX)] == 4
    _same(x, T, table, want, 4)
    # an allele nobody spans: the template in lower case and nothing else
    y = res[0][41]
    T41 = PREFIX + "CAG" * 41 + SUFFIX
    assert (y.h, y.reads, y.consensus, y.interruptions, y.insertions) == (41, 0, T41.lower(), [], [])
    assert not y.counts.any() and not y.depth.any() and y.counts.shape == (len(T41) + 1, 8)
    # alignments returns what it did, with or without the shared step handed over
    w = engine.winners(units)
    a, b = engine.alignments(units), engine.alignments(units, winners=w)
    assert sorted(a[0]) == sorted(b[0]) and all(a[0][k].verbose() == b[0][k].verbose() for k in a[0])
    again = engine.consensus(units, [[15]], winners=w)
    assert again[0][15].counts.tolist() == table


def _planted(a, unit):
    units = ["CAG"] * a
    units[unit - 1] = "CAA"
    return PREFIX + "".join(units) + SUFFIX


def _cut(text, ks, seed=5):
    """Reads cut from 40 random letters + text + 40 random letters: the spans G[40 - 5k : len - 40 + 6k], both strands."""
    rnd = random.Random(seed)
    G = "".join(rnd.choice("ACGT") for _ in range(40)) + text + "".join(rnd.choice("ACGT") for _ in range(40))
    out = []
    for k in ks:
        s = G[40 - 5 * k:len(G) - 40 + 6 * k]
        out += [s, pm.revcomp(s)]
    return out


def _unit(hd, reads):
    return Unit(hd, 150, reads, 30.0, 2, (), ())


@pytest.mark.parametrize("a,unit", [(10, 5), (10, 1), (10, 10), (15, 8)])
def test_a_planted_interruption_is_found_where_it_was_planted(engine, hd, a, unit):
    text = _planted(a, unit)
    reads = _cut(text, range(6))
    assert len(reads) == 12 and sorted(set(map(len, reads))) == [len(text) + 11 * k for k in range(6)]
    units = [_unit(hd, reads)]
    tag, h, sc, _, _ = engine.classify(units)
    assert (tag == _lib.TAG_FULL).all() and (h == a).all() and (sc == len(text) - 6).all(), (tag, h, sc)   # a tagging surprise shows here
    x = engine.consensus(units, [[a]])[0][a]
    assert x.reads == 12 and x.consensus == text and (x.depth == 12).all()
    assert x.interruptions == [{"unit": unit, "offset": 2, "ref": "G", "alt": "A", "support": 12, "depth": 12}]
    assert x.insertions == []


def test_mixed_evidence_on_both_sides_of_more_than_half(engine, hd):
    a, clean = 10, PREFIX + "CAG" * 10 + SUFFIX
    text = _planted(a, 5)
    x = engine.consensus([_unit(hd, _cut(text, range(6)) + _cut(clean, range(2), seed=6))], [[a]])[0][a]
    assert x.reads == 16 and x.consensus == text and x.insertions == []
    assert x.interruptions == [{"unit": 5, "offset": 2, "ref": "G", "alt": "A", "support": 12, "depth": 16}]
    x = engine.consensus([_unit(hd, _cut(text, range(4)) + _cut(clean, range(4), seed=6))], [[a]])[0][a]
    col = len(PREFIX) + 4 * 3 + 2
    assert x.reads == 16 and x.counts[col, :6].tolist() == [8, 0, 8, 0, 0, 0]
    assert x.interruptions == [] and x.consensus == clean            # 8 of 16 is not more than half; the tie goes to the template's G


def test_several_units_and_alleles_share_one_call(engine, hd):
    u10, u15 = _unit(hd, _cut(_planted(10, 5), range(6))), _unit(hd, _cut(_planted(15, 8), range(6)) + _cut(_planted(10, 1), range(3)))
    engine.ctx.reset_timing()
    res = engine.consensus([u10, u15, _unit(hd, [])], [[10], [10, 15], [7]])
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
    assert [sorted(r) for r in res] == [[10], [10, 15], [7]]
    assert [i["unit"] for i in res[0][10].interruptions] == [5] and res[0][10].reads == 12
    assert [i["unit"] for i in res[1][10].interruptions] == [1] and res[1][10].reads == 6
    assert [i["unit"] for i in res[1][15].interruptions] == [8] and res[1][15].reads == 12
    assert res[2][7].reads == 0 and res[2][7].consensus == (PREFIX + "CAG" * 7 + SUFFIX).lower()


# ---- the long path ----------------------------------------------------------------------------------------------------
NAME = "synlong600"


@pytest.fixture(scope="module")
def long_bam(tmp_path_factory):
    """The sample, regenerated from its seed as tests/test_long_reads_e2e_gpu.py does."""
    gold = json.load(open(os.path.join(GOLD, "run_long.json")))["samples"][NAME]
    names, kw, alt_rate = LONG_SAMPLES[NAME]
    loci = [l for l in synth.load_loci() if l["name"] in names]
    recs, _ = synth_bam.simulate_sample(gold["seed"], loci, synth.SynthParams(**kw), alt_rate=alt_rate)
    path = str(tmp_path_factory.mktemp(NAME) / (NAME + ".bam"))
    synth_bam.write_bam(path, recs, sample=NAME, level=1)
    return path


def test_long_reads_consensus_equals_the_model(long_bam):
    golden = json.load(open(os.path.join(GOLD, "alignments_" + NAME + ".json")))["loci"]
    e = Engine(0, long_reads=True)
    try:
        repo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
        scan = tredmod.collect_sample((NAME, long_bam, repo, LONG_SAMPLES[NAME][0], 300, False, False, True, True, "INFO"),
                                      long_reads=True)
        ks = [k for k, n in enumerate(scan.names) if n in golden]
        units = PackedUnits.from_scans([(scan, ks)])
        w = e.winners(units)
        al = e.alignments(units, winners=w)
        alleles = [sorted({x.h for x in a.values() if x.tag == _lib.TAG_FULL}) + [299] for a in al]
        e.ctx.reset_timing()
        res = e.consensus(units, alleles, winners=w)
        assert e.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
        spanned = 0
        for k, a, r, want in zip(ks, al, res, alleles):
            assert sorted(r) == want
            for h in want:
                t = scan.loci[k]
                T = t.prefix + t.repeat * h + t.suffix
                table, n = pm.table(len(T)), 0
                for x in a.values():
                    if x.tag == _lib.TAG_FULL and x.h == h:
                        f = [x.al.score, x.al.ref_begin, x.al.ref_end, x.al.query_begin, x.al.query_end]
                        pm.add_item(table, len(T), x.strand, x.al.query_seq, f, x.al._cigar_string)
                        n += 1
                _same(r[h], T, table, pm.consensus_of(table, T, len(t.prefix), len(t.repeat), h), n)
                spanned += n
                assert n or r[h].consensus == T.lower()
        assert spanned >= 4
    finally:
        e.close()


# ---- the command line -------------------------------------------------------------------------------------------------
def _run(work, capsys, *flags):
    tredmod.main([T001[1], "--tred", "HD", "--workdir", str(work)] + list(flags))
    return capsys.readouterr().out


def test_cli_writes_the_consensus_of_the_called_alleles(engine, t001_want, tmp_path, capsys, monkeypatch):
    T, table, want = t001_want
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    engine.ctx.reset_timing()
    plain = _run(tmp_path / "plain", capsys)
    assert sorted(os.listdir(tmp_path / "plain")) == ["t001.json", "t001.tred.vcf.gz"]
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 0 and engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0
    one = _run(tmp_path / "one", capsys, "--consensus")
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
    two = _run(tmp_path / "two", capsys, "--consensus")
    assert one == two == plain
    assert sorted(os.listdir(tmp_path / "one")) == ["t001.consensus.json", "t001.json", "t001.tred.vcf.gz"]
    text = (tmp_path / "one" / "t001.consensus.json").read_bytes()
    assert text == (tmp_path / "two" / "t001.consensus.json").read_bytes()
    assert (tmp_path / "one" / "t001.json").read_bytes() == (tmp_path / "plain" / "t001.json").read_bytes()
    calls = json.loads((tmp_path / "one" / "t001.json").read_text())["tredCalls"]
    assert (calls["HD.1"], calls["HD.2"]) == (15, 41)
    got = json.loads(text)
    assert list(got) == ["HD"] and list(got["HD"]) == ["alleles"] and [x["h"] for x in got["HD"]["alleles"]] == [15, 41]
    assert got["HD"]["alleles"][0] == dict(want, h=15, reads=4)
    T41 = PREFIX + "CAG" * 41 + SUFFIX
    assert got["HD"]["alleles"][1] == {"h": 41, "reads": 0, "consensus": T41.lower(), "depth": [0] * len(T41), "interruptions": [],
                                       "insertions": []}
    assert text == (json.dumps(got, sort_keys=True, indent=1) + "\n").encode()
    # suppressed with the other outputs
    _run(tmp_path / "none", capsys, "--consensus", "--no-output")
    assert not [n for n in os.listdir(tmp_path / "none") if n.startswith("t001")]


def test_cli_consensus_with_alignments_runs_the_shared_steps_once(engine, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    engine.ctx.reset_timing()
    _run(tmp_path / "both", capsys, "--consensus", "--alignments")
    assert engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1 and engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1
    assert sorted(os.listdir(tmp_path / "both")) == ["t001.alignments.txt", "t001.consensus.json", "t001.json", "t001.tred.vcf.gz"]
    with open(os.path.join(GOLD, "alignments_t001_HD.txt"), "rb") as fp:
        assert (tmp_path / "both" / "t001.alignments.txt").read_bytes() == fp.read()
    _run(tmp_path / "alone", capsys, "--consensus")
    assert (tmp_path / "both" / "t001.consensus.json").read_bytes() == (tmp_path / "alone" / "t001.consensus.json").read_bytes()
