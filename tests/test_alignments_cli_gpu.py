"""GPU: tred.py --alignments writes <samplekey>.alignments.txt -- for every `details` read the reference's verbose
block of the pair it was counted for (tests/golden/alignments_t001_HD.txt: the reference's own texts, put together by
tools/gen_golden_cigar.py) -- and changes nothing else the command writes."""
import gzip
import os

import pytest

from tredparse_amd import tred as tredmod

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def engine(ctx):
    from tredparse_amd.engine import Engine
    return Engine(ctx=ctx)            # on the session's context (tests/conftest.py: it loads PyTorch's HIP runtime first)


def _run(work, capsys, *flags):
    tredmod.main([os.path.join(GOLD, "bam", "t001.bam"), "--tred", "HD", "--workdir", str(work)] + list(flags))
    return capsys.readouterr().out


def test_alignments_report_is_the_references_text_and_nothing_else_changes(engine, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    plain = _run(tmp_path / "plain", capsys)
    flagged = _run(tmp_path / "flagged", capsys, "--alignments")
    assert sorted(os.listdir(tmp_path / "plain")) == ["t001.json", "t001.tred.vcf.gz"]
    assert sorted(os.listdir(tmp_path / "flagged")) == ["t001.alignments.txt", "t001.json", "t001.tred.vcf.gz"]
    with open(os.path.join(GOLD, "alignments_t001_HD.txt"), "rb") as fp:
        want = fp.read()
    assert (tmp_path / "flagged" / "t001.alignments.txt").read_bytes() == want and want.count(b">HD ") > 0
    assert (tmp_path / "flagged" / "t001.json").read_bytes() == (tmp_path / "plain" / "t001.json").read_bytes()
    vcf = [gzip.open(tmp_path / d / "t001.tred.vcf.gz", "rb").read() for d in ("plain", "flagged")]
    assert vcf[0] == vcf[1] and b"HD" in vcf[0]
    assert flagged == plain and '"samplekey": "t001"' in plain


def test_engine_alignments_agree_with_the_tags_the_reads_were_counted_for(engine):
    """Engine.alignments on the locus' unit: one entry per tagged read, whose winner is the (tag, h) pair of classify,
    and whose operations consume exactly the aligned bases."""
    from tredparse_amd import _lib
    from tredparse_amd.runtime import collect_sample
    from tredparse_amd.engine import PackedUnits
    from tredparse_amd.tred import TREDsRepo
    repo = TREDsRepo(ref="hg38")
    scan = collect_sample(("t001", os.path.join(GOLD, "bam", "t001.bam"), repo, ["HD"], 300, False, False, True, True, "INFO"))
    units = PackedUnits.from_scans([(scan, [0])])
    tag, h, _, _, _ = engine.classify(units)
    engine.ctx.reset_timing()
    al = engine.alignments(units)[0]
    assert engine.ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 1                      # ONE sw_cigar call for all winners
    assert sorted(al) == list(map(int, (tag != _lib.TAG_NONE).nonzero()[0])) and len(al) > 10
    for i, x in al.items():
        assert (x.tag, x.h) == (int(tag[i]), int(h[i]))
        ops = list(x.al.iter_cigar)
        assert sum(n for n, op in ops if op in "MI") == x.al.query_end - x.al.query_begin + 1
        assert sum(n for n, op in ops if op in "MD") == x.al.ref_end - x.al.ref_begin + 1
