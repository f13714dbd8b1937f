"""GPU: python -m tredparse_amd.prepare scan --interruptions end to end, on a small FASTA with an FMR1-shaped and an
SCA1-shaped tract in random flanks: catalog.tsv is the model's (tests/tract_model.py), and the site file of the FMR1-shaped
tract has its 30 copies and its flanks."""
import json
import os

import pytest

from tredparse_amd import _lib, prepare
from tredparse_amd.meta import TREDsRepo

from . import tract_model as tm
from .test_prepare_host import rand, write_fasta
from .test_prepare_tracts_host import TractContext

pytestmark = pytest.mark.gpu


@pytest.fixture()
def own_context(ctx, monkeypatch):
    """The command line makes a context of its own and closes it: here it gets the session's, which stays open."""
    monkeypatch.setattr(prepare._lib, "Context", lambda device=0: ctx)
    monkeypatch.setattr(ctx, "close", lambda: None)
    return ctx


def test_interrupted_tracts_catalog_and_site(own_context, tmp_path, capsys):
    tile = _lib.SCAN_TILE
    left, right = rand(60, 2 * tile - 40) + "TTGACA", "TCATGA" + rand(61, 5000)     # the tract lies across a tile's edge
    chr1 = left + tm.FMR1 + right
    chr2 = rand(62, 3000) + "T" + tm.SCA1.lower() + "T" + rand(63, 700) + "nnnn" + tm.FMR1[:60] + "A" + rand(64, 300)
    path = write_fasta(tmp_path / "syn.fa", [("chr1", chr1), ("empty", ""), ("chr2", chr2)], 70)
    sites = str(tmp_path / "sites")
    assert prepare.main(["scan", "--fasta", path, "--out", str(tmp_path / "gpu"), "--interruptions", "--write-sites", sites]) == 0
    assert "tracts" in capsys.readouterr().err
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "model"), "--interruptions"])
    prepare.run_scan(args, ctx=TractContext())
    text = (tmp_path / "gpu.tsv").read_text()
    assert text == (tmp_path / "model.tsv").read_text()
    assert text.splitlines()[0].split("\t")[-3:] == ["seeds", "mismatches", "purity"]
    rows = [line.split("\t") for line in text.splitlines()[1:]]
    at = len(left) + 1
    assert ["chr1", str(at), str(at + 89), "3", "CGG", "30", "0", "CCG", left[-18:], right[:18], "3", "2", "0.9778"] in rows
    assert [r[5:7] + r[10:] for r in rows if r[0] == "chr2" and r[4] == "CAG"] == [["12", "2", "1", "0", "1.0000"], ["15", "0", "1", "0", "1.0000"]]
    assert [r[5] for r in rows if r[0] == "chr2" and r[4] == "CGG"] == ["19"] and [r[10:12] for r in rows if r[0] == "chr2" and r[4] == "CGG"] == [["2", "1"]]
    name = "chr1_{}_CGG".format(at)
    with open(os.path.join(sites, name + ".json")) as fp:
        row = json.load(fp)[name]
    assert (row["repeat"], row["prefix"], row["suffix"], row["repeat_location"]) == ("CGG", left[-18:], right[:18], "chr1:{}-{}".format(at, at + 89))
    locus = TREDsRepo(sites=sites)[name]
    assert locus.ref_copy == 30 and (locus.repeat_start, locus.repeat_end) == (at, at + 89)
    # the perfect scan of the same FASTA lists the pieces: 9, 9 and 10 copies
    assert prepare.main(["scan", "--fasta", path, "--out", str(tmp_path / "perfect"), "--regions", "chr1", "--periods", "3"]) == 0
    perfect = [line.split("\t") for line in (tmp_path / "perfect.tsv").read_text().splitlines()[1:]]
    assert [r[5] for r in perfect] == ["9", "9", "10"] and all(len(r) == 10 for r in perfect)
    # a longer gap joins the SCA1-shaped tract: the model's rows again
    extra = ["--regions", "chr2:2900-3200", "--periods", "3", "--seed-copies", "5,3,4,3,3,3", "--max-gap", "1,2,7,4,5,6"]
    assert prepare.main(["scan", "--fasta", path, "--out", str(tmp_path / "gpu2")] + extra) == 0
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "model2")] + extra)
    prepare.run_scan(args, ctx=TractContext())
    assert (tmp_path / "gpu2.tsv").read_text() == (tmp_path / "model2.tsv").read_text()
    joined = [line.split("\t") for line in (tmp_path / "gpu2.tsv").read_text().splitlines()[1:]]
    assert [r[1:7] + r[10:] for r in joined] == [["3002", "3091", "3", "CAG", "30", "0", "2", "2", "0.9778"]]
