"""tredparse_amd/prepare.py without a GPU: the FASTA reader, the site of one locus against the reference's own PIEZO1 site
file, the refusals, the batching and chunk-and-merge of the scan with the kernel call replaced by the model
(tests/scan_model.py), the catalogue's text, and tred.py --sites."""
import gzip
import json
import os

import numpy as np
import pytest

from tredparse_amd import _lib, prepare
from tredparse_amd.meta import TREDsRepo

from . import scan_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
PIEZO1 = os.path.join(HERE, "golden", "sites", "PIEZO1.json")


def rand(seed, n, alphabet="ACGT"):
    return "".join(np.random.default_rng(seed).choice(list(alphabet), n))


def write_fasta(path, contigs, width=60, eol="\n", fai=False, final_eol=True):
    """contigs: [(name, letters)]; width None: one line per contig.  With fai, the index samtools faidx would write."""
    text, index = "", []
    for name, seq in contigs:
        text += ">" + name + " some description" + eol
        w = width or max(len(seq), 1)
        first = min(w, len(seq))                                           # (the first line's letters, as samtools faidx counts them)
        index.append("\t".join(str(x) for x in (name, len(seq), len(text.encode()), first, first + len(eol))))
        text += "".join(seq[k:k + w] + eol for k in range(0, len(seq), w))
    if not final_eol:
        text = text[:len(text) - len(eol)]
    with open(path, "wb") as fp:
        fp.write(text.encode())
    if fai:
        with open(str(path) + ".fai", "w") as fp:
            fp.write("\n".join(index) + "\n")
    return str(path)


class ModelContext(object):
    """Context.scan with the kernel replaced by the model; remembers the calls."""

    def __init__(self):
        self.calls = []

    def scan(self, letters, seg_off, min_copies=sm.MIN_COPIES, cap=1 << 16):
        buf = letters if isinstance(letters, np.ndarray) else np.frombuffer(letters, np.uint8)
        assert seg_off[-1] == len(buf)
        records = sm.scan(buf, [int(x) for x in seg_off], tuple(min_copies))
        self.calls.append((len(buf), len(seg_off) - 1, cap, len(records)))
        return tuple(x[:cap] for x in sm.arrays(records)) + (len(records),)


# ---- Fasta ------------------------------------------------------------------------------------------------------------------
CONTIGS = [("chrA", rand(1, 1234)), ("chrB", rand(2, 60).lower()), ("chrC", rand(3, 7) + "nnNN" + rand(4, 130)), ("chrD", "ACGT")]


@pytest.mark.parametrize("width,eol,fai,final_eol", [(60, "\n", False, True), (60, "\n", True, True), (7, "\n", False, True),
                                                     (None, "\n", False, True), (60, "\r\n", False, True), (60, "\r\n", True, True),
                                                     (7, "\n", False, False), (None, "\n", True, False)])
def test_fasta_reader(tmp_path, width, eol, fai, final_eol):
    f = prepare.Fasta(write_fasta(tmp_path / "g.fa", CONTIGS, width, eol, fai, final_eol))
    assert f.names == [c[0] for c in CONTIGS]
    rng = np.random.default_rng(5)
    for name, seq in CONTIGS:
        assert f.length(name) == len(seq) and f.fetch(name) == seq.upper().encode()
        for _ in range(30):
            a, b = sorted(rng.integers(0, len(seq) + 1, 2))
            assert f.fetch(name, a, b) == seq[a:b].upper().encode()
    with pytest.raises(prepare.PrepareError, match="outside"):
        f.fetch("chrD", 2, 5)
    with pytest.raises(prepare.PrepareError, match="no contig"):
        f.fetch("chrZ", 0, 1)
    f.close()


def test_fasta_index_equals_fai(tmp_path):
    """What the reader works out by itself is what the .fai says, blank lines at the end of the file or not."""
    path = write_fasta(tmp_path / "g.fa", CONTIGS, 50, "\n", fai=True)
    with_fai = prepare.Fasta(path).index
    os.remove(path + ".fai")
    assert prepare.Fasta(path).index == with_fai
    with open(path, "ab") as fp:
        fp.write(b"\n\n")
    assert prepare.Fasta(path).index == with_fai
    ragged = tmp_path / "ragged.fa"
    ragged.write_text(">x\nACGT\nAC\nACGT\n")
    with pytest.raises(prepare.PrepareError, match="width"):
        prepare.Fasta(str(ragged))


def test_fasta_refuses_gz(tmp_path):
    path = tmp_path / "g.fa.gz"
    with gzip.open(path, "wb") as fp:
        fp.write(b">x\nACGT\n")
    with pytest.raises(prepare.PrepareError, match="compressed"):
        prepare.Fasta(str(path))
    renamed = tmp_path / "g.fa"
    os.rename(path, renamed)                               # (the name does not say so, the first two bytes do)
    with pytest.raises(prepare.PrepareError, match="compressed"):
        prepare.Fasta(str(renamed))


# ---- prepare locus ----------------------------------------------------------------------------------------------------------
@pytest.fixture()
def piezo(tmp_path):
    """A contig with the reference's PIEZO1 strings at 1-based 501: (fasta path, the golden row)."""
    with open(PIEZO1) as fp:
        row = json.load(fp)["PIEZO1"]
    seq = rand(6, 500 - 18) + row["prefix"] + (row["repeat"] * 8).lower() + row["suffix"] + rand(7, 300)
    return write_fasta(tmp_path / "ref.fa", [("chr1", rand(8, 100)), ("chr16", seq)], 60), row


def test_locus_reproduces_the_reference_site(piezo, tmp_path, capsys):
    fasta, golden = piezo
    sites = str(tmp_path / "sites")
    rc = prepare.main(["locus", "--fasta", fasta, "--name", "PIEZO1", "--motif", "tcc", "--location", "chr16:501", "--outdir", sites,
                       "--cutoff-prerisk", "7", "--cutoff-risk", "7", "--mutation-nature", "decrease"])
    assert rc == 0
    with open(os.path.join(sites, "PIEZO1.json")) as fp:
        text = fp.read()
    row = json.loads(text)["PIEZO1"]
    assert set(row) == set(golden)                                         # every column of the reference's schema
    for column in ("prefix", "suffix", "repeat", "cutoff_prerisk", "cutoff_risk", "inheritance", "mutation_nature", "variant_type"):
        assert row[column] == golden[column], column
    span = lambda where: int(where.split("-")[1]) - int(where.split(":")[1].split("-")[0])
    assert row["repeat_location"] == "chr16:501-524" and span(row["repeat_location"]) == span(golden["repeat_location"])
    assert row["motif"] == "TCC" and row["id"] == "chr16_501_TCC"          # (the real motif, where the reference's tool writes CAG)
    assert text == json.dumps({"PIEZO1": row}, sort_keys=True, indent=2) + "\n"
    err = capsys.readouterr().err
    assert "AGCCCCTCGTCCCTGGAG|" + "tcc" * 8 + "|TGCTGCTGCTGCTGATGC" in err and "placeholder" not in err
    repo = TREDsRepo(sites=sites)
    locus = repo["PIEZO1"]
    assert locus.ref_copy == 8 and locus.repeat == "TCC" and (locus.chr, locus.repeat_start, locus.repeat_end) == ("chr16", 501, 524)
    assert repo.names[-1] == "PIEZO1" and len(repo.names) == len(TREDsRepo(sites=str(tmp_path / "none")).names) + 1
    assert not locus.is_expansion and not locus.is_recessive


def test_locus_copies_given_and_placeholders(piezo, tmp_path, capsys):
    fasta, _ = piezo
    sites = str(tmp_path / "s")
    assert prepare.main(["locus", "--fasta", fasta, "--name", "P6", "--motif", "TCC", "--location", "chr16:501", "--copies", "6",
                         "--outdir", sites]) == 0
    row = json.load(open(os.path.join(sites, "P6.json")))["P6"]
    assert row["repeat_location"] == "chr16:501-518" and row["suffix"] == "TCCTCC" + "TGCTGCTGCTGC"
    assert (row["cutoff_prerisk"], row["cutoff_risk"], row["inheritance"], row["mutation_nature"]) == (7, 7, "AD", "increase")
    assert "placeholder" in capsys.readouterr().err


def test_locus_refusals(piezo, tmp_path, capsys):
    fasta, _ = piezo
    sites = str(tmp_path / "s")
    run = lambda *extra: prepare.main(["locus", "--fasta", fasta, "--outdir", sites] + list(extra))
    cases = [
        (["--name", "X", "--motif", "CAG", "--location", "chr16:501"], "does not show"),                  # wrong motif, counted
        (["--name", "X", "--motif", "TCC", "--location", "chr16:501", "--copies", "9"], "not TCC x 9"),   # wrong copies
        (["--name", "X", "--motif", "TCC", "--location", "chr16:502", "--copies", "3"], "not TCC x 3"),   # wrong phase
        (["--name", "X", "--motif", "A", "--location", "chr16:5", "--copies", "1", "--force"], "closer than 18"),
        (["--name", "X", "--motif", "A", "--location", "chr16:{}".format(500 + 24 + 18 + 300 - 17), "--copies", "1", "--force"], "closer than 18"),
        (["--name", "HD", "--motif", "TCC", "--location", "chr16:501"], "built-in"),
        (["--name", "X", "--motif", "TCC", "--location", "chr17:501"], "no contig"),
        (["--name", "X", "--motif", "TXC", "--location", "chr16:501"], "letters A, C, G, T"),
        (["--name", "X", "--motif", "TCC", "--location", "chr16"], "contig:start"),
    ]
    for argv, message in cases:
        assert run(*argv) == 2, argv
        assert message in capsys.readouterr().err, argv
    assert not os.path.exists(sites)
    # the last place that still has its flanks, and --force where the FASTA shows something else
    assert run("--name", "EDGE", "--motif", "A", "--location", "chr16:{}".format(500 + 24 + 18 + 300 - 18), "--copies", "1", "--force") == 0
    assert run("--name", "FORCED", "--motif", "CAG", "--location", "chr16:501", "--copies", "8", "--force") == 0
    assert json.load(open(os.path.join(sites, "FORCED.json")))["FORCED"]["prefix"] == "AGCCCCTCGTCCCTGGAG"
    gz = tmp_path / "ref.fa.gz"
    gz.write_bytes(gzip.compress(b">x\nACGT\n"))
    assert prepare.main(["locus", "--fasta", str(gz), "--name", "X", "--motif", "A", "--location", "x:1"]) == 2
    assert "compressed" in capsys.readouterr().err


# ---- the scan: batching, chunk and merge ---------------------------------------------------------------------------------
def _records(out):
    return list(zip(*(x.tolist() for x in out)))


def test_scan_repeats_batches_segments():
    segs = [rand(10 + k, n).encode() for k, n in enumerate((300, 0, 450, 200, 1000, 5))]
    segs[2] = segs[2][:100] + b"CAG" * 20 + segs[2][160:]
    segs[4] = b"A" * 40 + segs[4][40:990] + b"GATA" * 3
    want = sm.scan(b"".join(segs), np.concatenate(([0], np.cumsum([len(s) for s in segs]))))
    assert len(want) >= 2
    for limit in (1 << 20, 1000, 1001, 2000):
        ctx = ModelContext()
        assert _records(prepare.scan_repeats(ctx, segs, max_letters=limit)) == want
        assert all(call[0] <= limit for call in ctx.calls)
        assert len(ctx.calls) == {1 << 20: 1, 1000: 3, 1001: 3, 2000: 1}[limit]
    ctx = ModelContext()
    assert _records(prepare.scan_repeats(ctx, segs, cap=1)) == want and [c[2] for c in ctx.calls] == [1, len(want)]   # the cap grows
    assert _records(prepare.scan_repeats(ModelContext(), [])) == []


def test_scan_repeats_chunk_and_merge():
    """A contig longer than the call limit: the pieces overlap, and the runs that touch a cut -- one that crosses several
    pieces, one that ends exactly at a cut, one that lies in an overlap and is found twice, one that qualifies only as a
    whole -- come out as the one call on the whole contig gives them."""
    limit = 500
    seq = bytearray(rand(20, 6000).encode())
    overlap = 60                                                            # max of min_copies p under the defaults... p = 1: 10
    assert max(m * p for p, m in enumerate(sm.MIN_COPIES, 1)) == 24
    stride = limit - 24
    seq[700:2300] = b"CAG" * 534                                            # across several pieces
    seq[stride * 6 - 30:stride * 6 + 24] = b"AC" * 27                       # ends where the seventh piece's overlap ends
    seq[stride * 8 + 2:stride * 8 + 22] = b"GATA" * 5                       # inside an overlap
    seq[stride * 9 - 7:stride * 9 + 5] = b"T" * 12                          # 12 letters, 7 before the ninth piece begins
    seq[stride * 10 + 24 - 4:stride * 10 + 24 + 9] = b"G" * 13              # and 9 behind the end of a piece
    del overlap
    whole = sm.scan(bytes(seq), [0, len(seq)])
    for extra in ([], [rand(21, 300).encode() + b"A" * 30]):
        segs = [bytes(seq)] + extra
        want = whole + [(1,) + r for r in sm.scan_segment(extra[0])] if extra else whole
        ctx = ModelContext()
        got = _records(prepare.scan_repeats(ctx, segs, max_letters=limit))
        assert got == want
        assert len(ctx.calls) >= 13 and all(c[0] <= limit for c in ctx.calls)
    for limit in (61, 100, 333, 5999, 6000):
        assert _records(prepare.scan_repeats(ModelContext(), [bytes(seq)], max_letters=limit)) == whole
    dense = rand(22, 3000, "AC").encode()
    all2 = (2,) * 6
    assert _records(prepare.scan_repeats(ModelContext(), [dense], all2, max_letters=100, cap=7)) == sm.scan(dense, [0, 3000], all2)
    with pytest.raises(prepare.PrepareError, match="too small"):
        prepare.scan_repeats(ModelContext(), [bytes(seq)], max_letters=40)
    periods = {2, 3}
    only = [r for r in whole if r[3] in periods]
    assert _records(prepare.scan_repeats(ModelContext(), [bytes(seq)], periods=periods, max_letters=limit)) == only
    assert prepare.parse_periods("1-6") == set(range(1, 7)) and prepare.parse_periods("2,4-5") == {2, 4, 5}
    with pytest.raises(prepare.PrepareError):
        prepare.parse_periods("0-3")


# ---- the catalogue -----------------------------------------------------------------------------------------------------------
def test_catalog_text(tmp_path):
    """A fixed input: the CTG tract is the reverse strand's CAG (canonical AGC for both); a tract 10 letters from the contig's
    end is listed without flanks and gets no site file; --regions shifts nothing."""
    quiet = "ACGTTGCATGCCATGACTGATCGTAGCTAGCATCGATCGGATCAGCTAGGATCTAGCTA"        # (no record under the defaults)
    assert sm.scan_segment(quiet * 2) == []
    chr1 = quiet + "CAG" * 7 + "CA" + quiet[::-1] + "CTG" * 6 + quiet + "C" + "GATA" * 5 + "GCGTACGTAC"
    chr2 = quiet[:30] + "T" * 12 + quiet
    path = write_fasta(tmp_path / "t.fa", [("chr1", chr1), ("chr2", chr2)], 50)
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "cat"), "--write-sites", str(tmp_path / "sites")])
    rows = prepare.run_scan(args, ctx=ModelContext())
    q = len(quiet)
    a, b, c = q + 1, q + 23 + q + 1, q + 23 + q + 18 + q + 1 + 1
    want = [("chr1", a, a + 20, 3, "CAG", 7, 2, "AGC", quiet[-18:], "CA" + quiet[::-1][:16]),
            ("chr1", b, b + 17, 3, "CTG", 6, 0, "AGC", quiet[::-1][-18:], quiet[:18]),
            ("chr1", c, c + 19, 4, "GATA", 5, 1, "AGAT", "", ""),
            ("chr2", 31, 42, 1, "T", 12, 0, "A", quiet[12:30], quiet[:18])]
    assert rows == want
    text = open(str(tmp_path / "cat.tsv")).read()
    assert text == "#contig\tstart\tend\tperiod\tmotif\tcopies\tpartial\tcanonical\tprefix\tsuffix\n" + \
        "".join("\t".join(str(x) for x in r) + "\n" for r in want)
    assert sorted(os.listdir(str(tmp_path / "sites"))) == sorted(["chr1_{}_CAG.json".format(a), "chr1_{}_CTG.json".format(b), "chr2_31_T.json"])
    repo = TREDsRepo(sites=str(tmp_path / "sites"))
    locus = repo["chr1_{}_CAG".format(a)]
    assert (locus.chr, locus.repeat_start, locus.repeat_end, locus.ref_copy, locus.prefix) == ("chr1", a, a + 20, 7, quiet[-18:])
    assert (locus.cutoff_prerisk, locus.cutoff_risk, locus.inheritance) == (8, 8, "AD")
    # a region: the same rows, in the contig's coordinates, flanks from outside the region
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "reg"), "--regions", "chr1:50-150", "chr2",
                                              "--periods", "3", "--min-copies", "10,6,7,4,4,4"])
    assert prepare.run_scan(args, ctx=ModelContext()) == [want[0]]
    args = prepare.set_argparse().parse_args(["scan", "--fasta", path, "--out", str(tmp_path / "m"), "--write-sites", str(tmp_path / "m"),
                                              "--max-sites", "2"])
    with pytest.raises(prepare.PrepareError, match="--max-sites"):
        prepare.run_scan(args, ctx=ModelContext())
    assert prepare.canonical_motif("ctg") == sm.canonical("CTG") == "AGC"


# ---- tred.py --sites -------------------------------------------------------------------------------------------------------
def test_tred_sites_option(piezo, tmp_path, monkeypatch):
    from tredparse_amd import tred
    fasta, _ = piezo
    sites = tmp_path / "mysites"
    assert prepare.main(["locus", "--fasta", fasta, "--name", "MYLOCUS", "--motif", "TCC", "--location", "chr16:501", "--outdir", str(sites)]) == 0
    monkeypatch.chdir(tmp_path)                                            # (no sites/ here)
    builtin = sorted(prepare.builtin_names())
    choices = lambda p: next(a.choices for a in p._actions if a.dest == "tred")
    assert choices(tred.set_argparse()) == choices(tred.set_argparse(["x.bam"])) == builtin and len(builtin) == 32
    p = tred.set_argparse(["x.bam", "--sites", str(sites), "--tred", "MYLOCUS"])
    assert choices(p) == sorted(builtin + ["MYLOCUS"])
    args = p.parse_args(["x.bam", "--sites", str(sites), "--tred", "MYLOCUS"])
    assert args.sites == str(sites) and args.tred == ["MYLOCUS"]
    assert tred.set_argparse().parse_args(["x.bam"]).sites == "sites"
    with pytest.raises(SystemExit):
        tred.set_argparse(["x.bam"]).parse_args(["x.bam", "--tred", "MYLOCUS"])
    # the option is argv's: a --gpus child gets it with the rest of the command line, and the run() tuple's tail is as it was
    from tredparse_amd import runtime
    assert runtime._TAIL == ("alignments", "consensus", "consensus_partial", "spectrum") and runtime.option_tail() == ()


def test_engine_scan_repeats_delegates():
    from tredparse_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.ctx = ModelContext()
    seq = rand(30, 200).encode() + b"CAG" * 9
    assert _records(e.scan_repeats([seq])) == sm.scan(seq, [0, len(seq)])
    assert _records(e.scan_repeats([seq], periods={1})) == [r for r in sm.scan(seq, [0, len(seq)]) if r[3] == 1]
    assert _lib.SCAN_MIN_COPIES == sm.MIN_COPIES
