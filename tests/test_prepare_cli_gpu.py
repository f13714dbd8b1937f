"""GPU: python -m tredparse_amd.prepare end to end.  (a) `scan` on a synthetic FASTA of four contigs with planted tracts of
every period: catalog.tsv is the model's (tests/scan_model.py), flanks included.  (b) A locus of one's own: HD's tract rebuilt
at its hg38 place in a synthetic chr4, cut out by `locus`, found by `scan`, and genotyped by tred.py --sites under another
name with the calls HD itself gets.  (c) Without --sites, in a directory without sites/, tred.py offers the built-in names."""
import json
import os

import pytest

from tredparse_amd import _lib, prepare
from tredparse_amd import tred as tredmod
from tredparse_amd.engine import Engine

from . import scan_model as sm
from .test_prepare_host import ModelContext, rand, write_fasta

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T001 = os.path.join(HERE, "golden", "bam", "t001.bam")
MOTIFS = {1: "T", 2: "AC", 3: "CAG", 4: "GATA", 5: "AACCT", 6: "AAGGCT"}


@pytest.fixture()
def own_context(ctx, monkeypatch):
    """The command line makes a context of its own and closes it: here it gets the session's, which stays open."""
    monkeypatch.setattr(prepare._lib, "Context", lambda device=0: ctx)
    monkeypatch.setattr(ctx, "close", lambda: None)
    return ctx


def test_scan_catalog_equals_the_model(own_context, tmp_path, capsys):
    contigs, planted = [], []
    for k, n in enumerate((120000, 60000, 20000, 37)):
        seq = bytearray(rand(40 + k, n).encode())
        for p in range(1, 7):
            if n < 5000:
                break
            at = p * n // 7
            if k == 0:                                                             # (the first contig begins on a tile's edge:
                at = at // _lib.SCAN_TILE * _lib.SCAN_TILE - 3 * p                 #  its tracts lie across one)
            tract = (MOTIFS[p] * 14)[:13 * p + p // 2]
            seq[at:at + len(tract)] = tract.encode() if k != 1 else tract.lower().encode()
            planted.append(("chr%d" % (k + 1), p, MOTIFS[p]))
        if k == 2:
            seq[-30:] = b"GATA" * 7 + b"GA"                                        # a tract at the contig's end: no flanks
            seq[5000:5400] = b"N" * 400
        contigs.append(("chr%d" % (k + 1), seq.decode()))
    path = write_fasta(tmp_path / "syn.fa", contigs, 70)
    assert prepare.main(["scan", "--fasta", path, "--out", str(tmp_path / "gpu")]) == 0
    assert "repeats" in capsys.readouterr().err
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "model")])
    prepare.run_scan(args, ctx=ModelContext())
    text = (tmp_path / "gpu.tsv").read_text()
    assert text == (tmp_path / "model.tsv").read_text()
    rows = [line.split("\t") for line in text.splitlines()[1:]]
    for contig, p, motif in planted:                                               # what was planted is listed, with its flanks
        hits = [r for r in rows if r[0] == contig and int(r[3]) == p and sm.canonical(r[4]) == sm.canonical(motif) and int(r[5]) >= 13]
        assert len(hits) >= 1 and all(len(r[8]) == len(r[9]) == 18 for r in hits), (contig, p)
    last = [r for r in rows if r[0] == "chr3"][-1]
    assert last[3:7] == ["4", "GATA", "7", "2"] and last[8:] == ["", ""] and int(last[2]) == 20000 - 2
    # regions and periods: the rows of the model on those regions
    extra = ["--regions", "chr1:4000-90000", "chr3", "--periods", "2-4", "--min-copies", "10,8,5,5,4,4"]
    assert prepare.main(["scan", "--fasta", path, "--out", str(tmp_path / "gpu2")] + extra) == 0
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "model2")] + extra)
    prepare.run_scan(args, ctx=ModelContext())
    assert (tmp_path / "gpu2.tsv").read_text() == (tmp_path / "model2.tsv").read_text() and len((tmp_path / "gpu2.tsv").read_text().splitlines()) > 4


def test_a_locus_of_ones_own_end_to_end(own_context, tmp_path, capsys, monkeypatch):
    with open(prepare.meta._DATA) as fp:
        hd = next(row for row in json.load(fp)["loci"] if row["name"] == "HD")
    assert (hd["repeat"], hd["repeat_location"]) == ("CAG", "chr4:3074877-3074933")
    chr4 = "N" * 3074858 + hd["prefix"] + "CAG" * 19 + hd["suffix"] + rand(50, 100)
    fasta = write_fasta(tmp_path / "chr4.fa", [("chr4", chr4)], 60)
    sites = str(tmp_path / "custom")
    assert prepare.main(["locus", "--fasta", fasta, "--name", "MYHD", "--motif", "CAG", "--location", "chr4:3074877", "--outdir", sites,
                         "--cutoff-prerisk", str(hd["cutoff_prerisk"]), "--cutoff-risk", str(hd["cutoff_risk"]),
                         "--inheritance", hd["inheritance"], "--mutation-nature", hd["mutation_nature"]]) == 0
    assert "CAG x 19" in capsys.readouterr().err                                   # counted: --copies was not given
    with open(os.path.join(sites, "MYHD.json")) as fp:
        row = json.load(fp)["MYHD"]
    for column in ("prefix", "suffix", "repeat", "repeat_location", "cutoff_prerisk", "cutoff_risk", "inheritance", "mutation_nature"):
        assert row[column] == hd[column], column

    # the scan finds the tract: 59 letters, 19 copies and CA of the twentieth
    assert prepare.main(["scan", "--fasta", fasta, "--out", str(tmp_path / "cat"), "--periods", "3"]) == 0
    capsys.readouterr()
    rows = [line.split("\t") for line in (tmp_path / "cat.tsv").read_text().splitlines()[1:]]
    assert ["chr4", "3074877", "3074933", "3", "CAG", "19", "2", "AGC", hd["prefix"], hd["suffix"]] in rows

    # tred.py --sites: MYHD is called as HD is
    engine = Engine(ctx=own_context)
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    monkeypatch.chdir(tmp_path)
    tredmod.main([T001, "--tred", "HD", "--noalts", "--quiet-json", "--workdir", str(tmp_path / "hd")])
    tredmod.main([T001, "--tred", "MYHD", "--sites", sites, "--noalts", "--quiet-json", "--workdir", str(tmp_path / "myhd")])
    capsys.readouterr()
    calls = {}
    for name, work in (("HD", "hd"), ("MYHD", "myhd")):
        with open(str(tmp_path / work / "t001.json")) as fp:
            calls[name] = json.load(fp)["tredCalls"]
    assert calls["HD"]["HD.1"] >= 0 and calls["HD"]["HD.FR"] != "" and calls["HD"]["HD.FDP"] > 0     # (the sample has reads there)
    for field in ("1", "2", "CI", "PP", "label", "FR", "PR", "RR", "DP", "FDP", "PDP", "RDP", "PEDP"):
        assert calls["MYHD"]["MYHD." + field] == calls["HD"]["HD." + field], field
    assert not any(k.startswith("HD.") for k in calls["MYHD"])


def test_without_sites_the_names_are_the_built_in_ones(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    assert not os.path.exists("sites")
    choices = next(a.choices for a in tredmod.set_argparse([T001])._actions if a.dest == "tred")
    assert choices == sorted(prepare.builtin_names()) and len(choices) == 32
    with pytest.raises(SystemExit):
        tredmod.main([T001, "--tred", "MYHD", "--noalts"])
    assert "MYHD" in capsys.readouterr().err
