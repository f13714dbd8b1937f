"""prepare.scan_repeats(interruptions=...) and `prepare scan --interruptions` without a GPU: the kernel call replaced by the
model (tests/tract_model.py), as tests/test_prepare_host.py does for the perfect scan."""
import json
import os

import numpy as np
import pytest

from tredparse_amd import _lib, prepare
from tredparse_amd.meta import TREDsRepo

from . import scan_model as sm
from . import tract_model as tm
from .test_prepare_host import ModelContext, rand, write_fasta


class TractContext(ModelContext):
    """Context.scan and Context.scan_tracts with the kernels replaced by the models; remembers the calls."""

    def __init__(self):
        ModelContext.__init__(self)
        self.tract_calls = []

    def scan_tracts(self, letters, seg_off, min_copies=sm.MIN_COPIES, seed_copies=tm.SEED_COPIES, max_gap=tm.MAX_GAP, cap=1 << 16):
        buf = letters if isinstance(letters, np.ndarray) else np.frombuffer(letters, np.uint8)
        assert seg_off[-1] == len(buf) and tm.rule_violation(list(min_copies), list(seed_copies), list(max_gap)) is None
        records = tm.tracts(buf, [int(x) for x in seg_off], tuple(min_copies), tuple(seed_copies), tuple(max_gap))
        self.tract_calls.append((len(buf), len(seg_off) - 1, cap, len(records)))
        return tuple(x[:cap] for x in tm.arrays(records)) + (len(records),)


def _records(out):
    return list(zip(*(x.tolist() for x in out)))


QUIET = "ACGTTGCATGCCATGACTGATCGTAGCTAGCATCGATCGGATCAGCTAGGATCTAGCTA"           # (no record under the defaults)


def test_scan_repeats_tract_path_batches_segments():
    segs = [rand(10 + k, n).encode() for k, n in enumerate((300, 0, 450, 200, 1000, 5))]
    segs[2] = segs[2][:100] + tm.FMR1.encode() + segs[2][190:]
    segs[4] = b"A" * 40 + segs[4][40:800] + tm.SCA1.encode() + segs[4][890:]
    want = tm.tracts(b"".join(segs), np.concatenate(([0], np.cumsum([len(s) for s in segs]))))
    assert len(want) >= 3 and any(r[4] == 3 and r[5] == 2 for r in want)
    for limit in (1 << 20, 1000, 1001, 2000):
        ctx = TractContext()
        out = prepare.scan_repeats(ctx, segs, max_letters=limit, interruptions=True)
        assert _records(out) == want and [x.dtype for x in out] == [np.int32, np.int64] + [np.int32] * 4
        assert all(call[0] <= limit for call in ctx.tract_calls) and not ctx.calls
        assert len(ctx.tract_calls) == {1 << 20: 1, 1000: 3, 1001: 3, 2000: 1}[limit]
    ctx = TractContext()
    assert _records(prepare.scan_repeats(ctx, segs, cap=1, interruptions=True)) == want
    assert [c[2] for c in ctx.tract_calls] == [1, len(want)]                # the cap grows
    assert _records(prepare.scan_repeats(TractContext(), [], interruptions=True)) == []
    sc, mg = list(tm.SEED_COPIES), list(tm.MAX_GAP)
    sc[2], mg[2] = 4, 7
    joined = _records(prepare.scan_repeats(TractContext(), segs, periods={3}, interruptions=(sc, mg)))
    assert joined == tm.tracts(b"".join(segs), np.concatenate(([0], np.cumsum([len(s) for s in segs]))), (0, 0, 5, 0, 0, 0), sc, mg)
    assert any(r[4] == 2 and r[5] == 2 and r[2] >= 90 for r in joined)      # the SCA1-shaped tract in one piece
    # None is today's path: the perfect scan's call, four arrays
    ctx = TractContext()
    assert _records(prepare.scan_repeats(ctx, segs)) == sm.scan(b"".join(segs), np.concatenate(([0], np.cumsum([len(s) for s in segs]))))
    assert ctx.calls and not ctx.tract_calls


def test_scan_repeats_tract_path_refusals():
    seq = rand(20, 600).encode()
    with pytest.raises(prepare.PrepareError, match="more than the 500 of one call"):
        prepare.scan_repeats(TractContext(), [seq[:100], seq], max_letters=500, interruptions=True)
    bad = {
        "seed_copies \\* p > max_gap \\+ 2 p - 2": (tm.SEED_COPIES, (1, 2, 5, 4, 5, 6)),
        "2 <= seed_copies <= min_copies": ((5, 3, 6, 3, 3, 3), tm.MAX_GAP),
        "0 <= max_gap <= 64": ((50, 50, 50, 50, 50, 50), (1, 2, 3, 65, 5, 6)),
        "whole numbers": ((5, 3, 3), tm.MAX_GAP),
    }
    for message, (sc, mg) in bad.items():
        ctx = TractContext()
        with pytest.raises(prepare.PrepareError, match=message):
            prepare.scan_repeats(ctx, [seq], min_copies=(60,) * 6 if sc[0] == 50 else None, interruptions=(sc, mg))
        assert not ctx.tract_calls
    with pytest.raises(prepare.PrepareError, match="max_gap"):
        prepare.scan_repeats(TractContext(), [seq], interruptions=(tm.SEED_COPIES, (1, 2, 3, -1, 5, 6)))
    # of a period that is off nothing is checked
    out = prepare.scan_repeats(TractContext(), [seq], periods={3}, interruptions=((9, 9, 3, 9, 9, 9), (99, 99, 3, 99, 99, 99)))
    assert len(out) == 6


def _fasta(tmp_path):
    chr1 = QUIET + tm.FMR1 + QUIET[::-1] + "CTG" * 6 + QUIET + "C" + "GATA" * 5 + "GCGTACGTAC"
    chr2 = QUIET[:29] + "T" + tm.SCA1.lower() + QUIET
    return write_fasta(tmp_path / "t.fa", [("chr1", chr1), ("chr2", chr2)], 50), chr1, chr2


def test_catalog_text_with_tracts(tmp_path):
    path, chr1, chr2 = _fasta(tmp_path)
    q = len(QUIET)
    assert sm.scan_segment(QUIET * 2) == [] and QUIET[::-1][0] != "C"
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "cat"), "--interruptions",
                                              "--write-sites", str(tmp_path / "sites")])
    ctx = TractContext()
    rows = prepare.run_scan(args, ctx=ctx)
    assert ctx.tract_calls and not ctx.calls
    b = q + 90 + q + 1
    c = b + 18 + q + 1
    want = [("chr1", q + 1, q + 90, 3, "CGG", 30, 0, "CCG", QUIET[-18:], QUIET[::-1][:18], 3, 2, "0.9778"),
            ("chr1", b, b + 17, 3, "CTG", 6, 0, "AGC", QUIET[::-1][-18:], QUIET[:18], 1, 0, "1.0000"),
            ("chr1", c, c + 19, 4, "GATA", 5, 1, "AGAT", "", "", 1, 0, "1.0000"),
            ("chr2", 31, 66, 3, "CAG", 12, 2, "AGC", (QUIET[:29] + "T")[12:], ("CA" + "TCAGCAT" + "CAG" * 15)[:18], 1, 0, "1.0000"),
            ("chr2", 76, 120, 3, "CAG", 15, 0, "AGC", ("CAG" * 12 + "CATCAGCAT")[-18:], QUIET[:18], 1, 0, "1.0000")]
    assert rows == want
    text = open(str(tmp_path / "cat.tsv")).read()
    assert text == "#contig\tstart\tend\tperiod\tmotif\tcopies\tpartial\tcanonical\tprefix\tsuffix\tseeds\tmismatches\tpurity\n" + \
        "".join("\t".join(str(x) for x in r) + "\n" for r in want)
    # --write-sites works on those rows: the FMR1-shaped tract is one site of 30 copies
    assert "chr1_{}_CGG.json".format(q + 1) in os.listdir(str(tmp_path / "sites")) and len(os.listdir(str(tmp_path / "sites"))) == 4
    locus = TREDsRepo(sites=str(tmp_path / "sites"))["chr1_{}_CGG".format(q + 1)]
    assert (locus.chr, locus.repeat_start, locus.repeat_end, locus.ref_copy, locus.repeat) == ("chr1", q + 1, q + 90, 30, "CGG")
    assert (locus.prefix, locus.suffix) == (QUIET[-18:], QUIET[::-1][:18])
    row = json.load(open(str(tmp_path / "sites" / "chr1_{}_CGG.json".format(q + 1))))["chr1_{}_CGG".format(q + 1)]
    assert (row["cutoff_prerisk"], row["cutoff_risk"]) == (31, 31)
    # either value option implies the mode; with a longer gap the SCA1-shaped tract is one row
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "g"), "--regions", "chr2", "--periods", "3",
                                              "--max-gap", "1,2,7,4,5,6", "--seed-copies", "5,3,4,3,3,3"])
    assert prepare.run_scan(args, ctx=TractContext()) == [
        ("chr2", 31, 120, 3, "CAG", 30, 0, "AGC", (QUIET[:29] + "T")[12:], QUIET[:18], 2, 2, "0.9778")]
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "h"), "--seed-copies", "5,3,3,3,3,3"])
    assert prepare.run_scan(args, ctx=TractContext()) == want


def test_catalog_without_the_flag_is_byte_identical(tmp_path):
    """The perfect scan's catalogue of the same FASTA: its ten columns, the FMR1-shaped tract in three pieces."""
    path, chr1, chr2 = _fasta(tmp_path)
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "cat")])
    assert not args.interruptions and args.seed_copies is None and args.max_gap is None
    ctx = TractContext()
    rows = prepare.run_scan(args, ctx=ctx)
    assert ctx.calls and not ctx.tract_calls
    fasta = prepare.Fasta(path)
    regions = prepare.parse_regions(fasta, None)
    records = sm.arrays(sm.scan((chr1 + chr2).encode(), [0, len(chr1), len(chr1) + len(chr2)]))
    want = []
    for seg, start, length, period in zip(*records):                       # the catalogue as it was before the tract path
        contig, text = regions[seg][0], (chr1, chr2)[seg].upper()
        g, p = int(start), int(period)
        copies, partial = divmod(int(length), p)
        end = g + copies * p
        flanks = (text[g - 18:g], text[end:end + 18]) if g >= 18 and end + 18 <= len(text) else ("", "")
        want.append((contig, g + 1, end, p, text[g:g + p], copies, partial, sm.canonical(text[g:g + p])) + flanks)
    fasta.close()
    assert rows == want and [r[5] for r in rows if r[4] in ("CGG", "GGC")] == [9, 9, 10]
    assert open(str(tmp_path / "cat.tsv")).read() == "#contig\tstart\tend\tperiod\tmotif\tcopies\tpartial\tcanonical\tprefix\tsuffix\n" + \
        "".join("\t".join(str(x) for x in r) + "\n" for r in want)
    assert prepare.catalog_text(rows) == open(str(tmp_path / "cat.tsv")).read()


def test_command_line_refusals(tmp_path, capsys):
    path, _, _ = _fasta(tmp_path)
    run = lambda *extra: prepare.main(["scan", "--fasta", path, "--out", str(tmp_path / "x")] + list(extra))
    for argv, message in ((["--max-gap", "1,2,5,4,5,6"], "seed_copies * p > max_gap + 2 p - 2"),
                          (["--seed-copies", "5,3,6,3,3,3"], "2 <= seed_copies <= min_copies"),
                          (["--max-gap", "1,2,3"], "whole numbers"),
                          (["--interruptions", "--seed-copies", "a,b"], "six counts each")):
        assert run(*argv) == 2, argv                                       # (refused before a context is made)
        assert message in capsys.readouterr().err, argv
    assert not os.path.exists(str(tmp_path / "x.tsv"))


def test_engine_scan_repeats_delegates():
    from tredparse_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.ctx = TractContext()
    seq = rand(30, 200).encode() + tm.FMR1.encode() + rand(31, 50).encode()
    want = tm.tracts(seq, [0, len(seq)])
    assert (0, 200, 90, 3, 3, 2) in [r[:1] + (200,) + r[2:] for r in want if r[3] == 3 and r[4] == 3]
    assert _records(e.scan_repeats([seq], interruptions=True)) == want
    assert _records(e.scan_repeats([seq], periods={3}, interruptions=(tm.SEED_COPIES, (0,) * 6))) == \
        [r + (1, 0) for r in sm.scan(seq, [0, len(seq)]) if r[3] == 3]
    assert _records(e.scan_repeats([seq])) == sm.scan(seq, [0, len(seq)])
    assert _lib.TRACT_SEED_COPIES == tm.SEED_COPIES and _lib.TRACT_MAX_GAP_DEFAULT == tm.MAX_GAP
