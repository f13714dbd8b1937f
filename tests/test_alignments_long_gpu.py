"""GPU: the alignments of long reads through the product path -- Engine(long_reads=True).alignments and tred.py
--long-reads --alignments on the 600 bp sample synlong600 -- against the reference's alignments of the same pairs
(tests/golden/alignments_synlong600.json, tools/gen_golden_cigar_long.py)."""
import hashlib
import json
import os

import pytest

from tredparse_amd import _lib, synth, synth_bam, tred as tredmod
from tredparse_amd.engine import Engine, PackedUnits

from .test_long_reads_e2e_gpu import LONG_SAMPLES

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "synlong600"


@pytest.fixture(scope="module")
def long_engine(ctx):
    e = Engine(0, long_reads=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    """The sample, regenerated from its seed as tests/test_long_reads_e2e_gpu.py does."""
    gold = json.load(open(os.path.join(GOLD, "run_long.json")))["samples"][NAME]
    names, kw, alt_rate = LONG_SAMPLES[NAME]
    loci = [l for l in synth.load_loci() if l["name"] in names]
    recs, _ = synth_bam.simulate_sample(gold["seed"], loci, synth.SynthParams(**kw), alt_rate=alt_rate)
    path = str(tmp_path_factory.mktemp(NAME) / (NAME + ".bam"))
    synth_bam.write_bam(path, recs, sample=NAME, level=1)
    return path


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLD, "alignments_synlong600.json")))["loci"]


def test_engine_alignments_of_long_reads_are_the_references(long_engine, bam, golden):
    from tredparse_amd.meta import TREDsRepo
    repo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
    scan = tredmod.collect_sample((NAME, bam, repo, LONG_SAMPLES[NAME][0], 300, False, False, True, True, "INFO"), long_reads=True)
    assert scan.readlen == 600 and not scan.dropped
    ks = [k for k, n in enumerate(scan.names) if n in golden]
    assert len(ks) == len(golden) == 2
    long_engine.ctx.reset_timing()
    res = long_engine.alignments(PackedUnits.from_scans([(scan, ks)]))
    assert long_engine.ctx.get_timing(_lib.KERNEL_CIGAR_LONG)[0] == 1          # ONE long call for all winners
    for k, al in zip(ks, res):
        rows = golden[scan.names[k]]
        a, _ = scan.reads_of(k)
        at = 0
        for i in sorted(al):                       # the `details` reads are a subsequence of the tagged reads, in BAM order
            x = al[i]
            if at < len(rows) and (scan.name(a + i), _lib.TAG_NAMES[x.tag], x.h) == (rows[at]["id"], rows[at]["tag"], rows[at]["h"]):
                r = rows[at]
                assert "-+"[x.strand == 0] == r["strand"], r["id"]
                assert [x.al.score, x.al.ref_begin, x.al.ref_end, x.al.query_begin, x.al.query_end] == r["fields"], r["id"]
                assert x.al.cigar_string == r["cigar_string"], r["id"]
                assert hashlib.sha256(x.verbose().encode()).hexdigest() == r["block_sha256"], r["id"]
                at += 1
        assert at == len(rows) >= 4, (scan.names[k], at, len(rows))


def _run(bam, work, capsys, *flags):
    tredmod.main([bam, "--tred", "HD", "--workdir", str(work), "--long-reads"] + list(flags))
    return capsys.readouterr().out


def test_cli_writes_the_report_of_a_long_read_sample(long_engine, bam, golden, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: long_engine)
    plain = _run(bam, tmp_path / "plain", capsys)
    flagged = _run(bam, tmp_path / "flagged", capsys, "--alignments")
    assert sorted(os.listdir(tmp_path / "plain")) == [NAME + ".json", NAME + ".tred.vcf.gz"]
    assert sorted(os.listdir(tmp_path / "flagged")) == [NAME + ".alignments.txt", NAME + ".json", NAME + ".tred.vcf.gz"]
    assert (tmp_path / "flagged" / (NAME + ".json")).read_bytes() == (tmp_path / "plain" / (NAME + ".json")).read_bytes()
    assert flagged == plain
    text = (tmp_path / "flagged" / (NAME + ".alignments.txt")).read_text()
    assert text.endswith("\n\n")
    entries = text[:-2].split("\n\n")
    rows = golden["HD"]
    assert len(entries) == len(rows) >= 4
    for entry, r in zip(entries, rows):
        header, block = entry.split("\n", 1)
        assert header == ">HD {} h={} {} {}".format(r["tag"], r["h"], r["strand"], r["id"])
        assert hashlib.sha256((block + "\n").encode()).hexdigest() == r["block_sha256"], r["id"]
