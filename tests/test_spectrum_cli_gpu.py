"""GPU: tred.py --spectrum -- <samplekey>.spectrum.json is what Engine.spectrum's result serialises to, run after run; the
files of --alignments and --consensus-partial beside it are what they are without it; without the flag nothing is
launched and nothing is written."""
import json
import os

import pytest

from tredparse_amd import _lib

from .test_consensus_gpu import GOLD, _run, _t001_units, engine  # noqa: F401

pytestmark = pytest.mark.gpu


def test_cli_spectrum(engine, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    engine.ctx.reset_timing()
    _run(tmp_path / "plain", capsys)
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 0 and engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0
    assert sorted(os.listdir(tmp_path / "plain")) == ["t001.json", "t001.tred.vcf.gz"]
    one = _run(tmp_path / "one", capsys, "--spectrum")
    assert engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 1 and engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1
    two = _run(tmp_path / "two", capsys, "--spectrum")
    assert one == two
    assert sorted(os.listdir(tmp_path / "one")) == ["t001.json", "t001.spectrum.json", "t001.tred.vcf.gz"]
    text = (tmp_path / "one" / "t001.spectrum.json").read_bytes()
    assert text == (tmp_path / "two" / "t001.spectrum.json").read_bytes()
    assert (tmp_path / "one" / "t001.json").read_bytes() == (tmp_path / "plain" / "t001.json").read_bytes()
    # the file is the engine's result for the called alleles, serialised
    want = engine.spectrum(_t001_units(), [[15, 41]])[0].to_dict()
    assert text == (json.dumps({"HD": want}, sort_keys=True, indent=1) + "\n").encode()
    got = json.loads(text)
    assert sorted(got["HD"]["classes"]) == ["full:15", "full:41", "partial", "rept"] and got["HD"]["motif"] == "CAG"
    assert got["HD"]["classes"]["full:15"]["reads"] == 4 and got["HD"]["classes"]["partial"]["reads"] == 21


def test_cli_spectrum_beside_the_other_reports(engine, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    _run(tmp_path / "alone", capsys, "--spectrum")
    _run(tmp_path / "without", capsys, "--alignments", "--consensus-partial")
    engine.ctx.reset_timing()
    _run(tmp_path / "with", capsys, "--alignments", "--consensus-partial", "--spectrum")
    # one CIGAR call for all three; the anchored pileup and the spectrum are a call each of the same unit
    assert engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1 and engine.ctx.get_timing(_lib.KERNEL_PILEUP)[0] == 2
    assert sorted(os.listdir(tmp_path / "with")) == ["t001.alignments.txt", "t001.consensus.json", "t001.json", "t001.spectrum.json",
                                                    "t001.tred.vcf.gz"]
    for name in ("t001.alignments.txt", "t001.consensus.json", "t001.json"):
        assert (tmp_path / "with" / name).read_bytes() == (tmp_path / "without" / name).read_bytes(), name
    assert (tmp_path / "with" / "t001.spectrum.json").read_bytes() == (tmp_path / "alone" / "t001.spectrum.json").read_bytes()
    with open(os.path.join(GOLD, "alignments_t001_HD.txt"), "rb") as fp:
        assert (tmp_path / "with" / "t001.alignments.txt").read_bytes() == fp.read()
    assert "t001.spectrum.json" not in os.listdir(tmp_path / "without")
