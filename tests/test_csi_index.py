"""CSI (.csi) indexes on the host: a BAM that comes with only a .csi reads, scans and plans exactly like its .bai copy.

The layout is pinned by a CSI built byte by byte here, field by field as CSIv1 (hts-specs) lays it out -- not by the
project's writer (bamio.write_csi / csi_bytes).  Every other check compares a CSI-only copy of a BAM, at min_shift 12, 14
and 16, with the same BAM read through its .bai: both AlignmentFile layers, the whole-sample scan, the plans of the device
walks and the blocks they list (walked by tests/walk_model.py's stand-in for the device)."""
import gzip
import os
import random
import shutil
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tredparse_amd import bamio, synth, synth_bam
from tredparse_amd import tred as t
from tredparse_amd.bam_parser import DNAPE_ELONGATE, FLANKMATCH, SPAN, _site_arrays, scan_sample
from tredparse_amd.meta import TREDsRepo

from .walk_model import ModelInflater

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SHIFTS = (12, 14, 16)
SCAN_FIELDS = ("packed", "word_off", "read_len", "seq4", "seq4_off", "name_blob", "name_off", "name_id", "global_lens",
               "target_lens", "depth", "ploidy")


def _layers():
    out = [bamio.PyAlignmentFile]
    if bamio._native() is not None:
        out.append(bamio.NativeAlignmentFile)
    return out


def _csi_only(src, dst_dir, min_shift):
    """A copy of the BAM `src` in dst_dir with a .csi of min_shift next to it and no .bai."""
    os.makedirs(dst_dir, exist_ok=True)
    dst = os.path.join(dst_dir, os.path.basename(src))
    shutil.copyfile(src, dst)
    bamio.write_csi(dst, min_shift=min_shift)
    return dst


# ---- the layout, from the specification alone --------------------------------------------------------------------
def _bgzf_block(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    return (struct.pack("<4BI2BH2BHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(body) + 25) + body
            + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def _record(pos, name):
    """A mapped 50M record of contig 0 without sequence (block_size word included)."""
    body = struct.pack("<iiBBHHHiiii", 0, pos, len(name) + 1, 60, 0, 1, 0, 0, -1, -1, 0) + name + b"\0" + struct.pack("<I", 50 << 4)
    return struct.pack("<i", len(body)) + body


def _tiny(tmp_path):
    """A BAM of one 100 Mb contig with two records, each in a BGZF block of its own, and the raw bytes of its CSI: min_shift
    14, depth 5; the leaf bins 4681 + (pos >> 14) with one chunk each and loffset = the record's own virtual offset; the
    pseudo-bin 37450 ((1 << 18) - 1) / 7 + 1) with (first, last offset), (2 mapped, 0 unmapped); n_no_coor 0."""
    header = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 4) + b"ctg\0" + struct.pack("<i", 100000000)
    blocks = [_bgzf_block(header), _bgzf_block(_record(100, b"r1")), _bgzf_block(_record(20000, b"r2")), _bgzf_block(b"")]
    co = np.cumsum([0] + [len(b) for b in blocks])
    path = str(tmp_path / "tiny.bam")
    with open(path, "wb") as fp:
        fp.write(b"".join(blocks))
    v1, e1, v2, e2 = int(co[1]) << 16, int(co[2]) << 16, int(co[2]) << 16, int(co[3]) << 16
    raw = b"CSI\1" + struct.pack("<i", 14) + struct.pack("<i", 5) + struct.pack("<i", 0) + struct.pack("<i", 1)
    raw += struct.pack("<i", 3)                                           # n_bin (two bins + the pseudo-bin)
    raw += struct.pack("<I", 4681) + struct.pack("<Q", v1) + struct.pack("<i", 1) + struct.pack("<QQ", v1, e1)
    raw += struct.pack("<I", 4682) + struct.pack("<Q", v2) + struct.pack("<i", 1) + struct.pack("<QQ", v2, e2)
    raw += struct.pack("<I", 37450) + struct.pack("<Q", 0) + struct.pack("<i", 2) + struct.pack("<QQ", v1, e2) + struct.pack("<QQ", 2, 0)
    raw += struct.pack("<Q", 0)                                           # n_no_coor
    return path, raw


def test_a_csi_built_by_hand_is_read(tmp_path):
    path, raw = _tiny(tmp_path)
    with open(path + ".csi", "wb") as fp:                                 # two BGZF blocks, cut inside a bin record
        fp.write(_bgzf_block(raw[:30]) + _bgzf_block(raw[30:]) + _bgzf_block(b""))
    for cls in _layers():
        f = cls(path)
        assert [r.query_name for r in f.fetch("ctg", 0, 200)] == ["r1"]
        assert [r.query_name for r in f.fetch("ctg", 10000, 30000)] == ["r2"]
        assert [r.query_name for r in f.fetch("ctg", 149, 20001)] == ["r1", "r2"]
        assert [r.query_name for r in f.fetch("ctg")] == ["r1", "r2"]
        assert list(f.fetch("ctg", 150, 20000)) == [] and list(f.fetch("ctg", 30000, 90000000)) == []
        assert f.pileup_depth_sum("ctg", 0, 100000000) == 100
        f.close()
    # and the project's writer, read back through the specification: the same bytes
    assert gzip.decompress(open(bamio.write_csi(path, str(tmp_path / "w.csi")), "rb").read()) == raw


def test_depth_is_chosen_as_samtools_chooses_it():
    chr1 = 248956422                                                      # hg38's longest contig
    assert [bamio.csi_depth([chr1, 1000], s) for s in (12, 14, 16)] == [6, 5, 4]
    assert bamio.csi_depth([(1 << 14) - 256], 14) == 0 and bamio.csi_depth([(1 << 14) - 255], 14) == 1


# ---- the same records, scans and plans as through the .bai ------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """[(name, .bai path, {min_shift: CSI-only path}, repo, locus names)]: synthetic samples (one whole-genome shaped), a
    file whose records straddle 300-byte blocks, and the reference's t001 / t002."""
    root = str(tmp_path_factory.mktemp("csi"))
    loci = [l for l in synth.load_loci() if l["name"] in ("HD", "DM1", "SCA1", "AR")]
    p = synth.SynthParams(coverage=12, expanded_max=120, expanded_frac=0.3)
    made = [(k, path) for k, path, _ in synth_bam.make_bams(root, 2, seed=5, loci=loci, p=p)]
    made += [(k, path) for k, path, _ in synth_bam.make_bams(root, 1, seed=9, prefix="wgs", wgs_like=True)]
    recs, _ = synth_bam.simulate_sample(6, loci[:2], synth.SynthParams(coverage=8, expanded_max=120, expanded_frac=0.3))
    cut = os.path.join(root, "cut300.bam")
    synth_bam.write_bam(cut, recs, sample="cut", block=300, split_records=True, index="both")
    made.append(("cut300", cut))
    srepo, repo = TREDsRepo(), TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
    out = []
    for k, path in made:
        names = [l["name"] for l in loci] if k != "wgs0000" else [l["name"] for l in synth_bam.bench_loci()]
        out.append((k, path, {s: _csi_only(path, os.path.join(root, "csi{}".format(s)), s) for s in SHIFTS}, srepo, names))
    for s in ("t001", "t002"):
        path = os.path.join(GOLD, "bam", s + ".bam")
        out.append((s, path, {m: _csi_only(path, os.path.join(root, "csi{}".format(m)), m) for m in SHIFTS}, repo,
                    sorted(repo.names)))
    return out


def test_write_bam_and_write_csi_write_the_same_index(files):
    cut = [f for f in files if f[0] == "cut300"][0]
    assert open(cut[1] + ".csi", "rb").read() == open(cut[2][14] + ".csi", "rb").read()
    assert os.path.exists(cut[1] + ".bai")
    for name, path, csi, _, _ in files:
        assert not os.path.exists(csi[14] + ".bai"), name


def _regions(f, loci_names, repo, rng):
    out = [("chrY", 0, 100)]
    for n in loci_names:
        tr = repo[n]
        for _ in range(2):
            out.append((tr.chr, max(0, tr.repeat_start - rng.randint(0, 40000)), tr.repeat_end + rng.randint(0, 40000)))
        out.append((tr.chr, tr.repeat_start, tr.repeat_start))
    return [g for g in out if g[0] in f.references]


def _key(r):
    return (r.tid, r.pos, r.flag, r.query_name, r.reference_end, r.next_tid, r.next_pos, r.query_sequence)


def test_fetch_and_depth_agree_with_the_bai(files):
    rng = random.Random(20261015)
    for name, path, csi, repo, names in files:
        ref = bamio.AlignmentFile(path)
        regions = _regions(ref, names, repo, rng)
        want = [[_key(r) for r in ref.fetch(*g)] for g in regions]
        depth = [ref.pileup_depth_sum(*g) for g in regions]
        assert sum(map(len, want)) > 0, name
        ref.close()
        for s in SHIFTS:
            for cls in _layers():
                f = cls(csi[s])
                assert [[_key(r) for r in f.fetch(*g)] for g in regions] == want, (name, s, cls.__name__)
                assert [f.pileup_depth_sum(*g) for g in regions] == depth, (name, s, cls.__name__)
                f.close()


def _same_scan(a, b):
    assert a.opened and b.opened and a.gender == b.gender and a.readlen == b.readlen and a.dropped == b.dropped
    for key in a.unit.dtype.names:
        assert (a.unit[key] == b.unit[key]).all(), key
    for key in SCAN_FIELDS:
        x, y = getattr(a, key), getattr(b, key)
        assert (x == y) if isinstance(x, bytes) else np.array_equal(x, y), key


def test_scan_sample_agrees_with_the_bai(files):
    if bamio._native() is None:
        pytest.skip("no native BAM layer")
    for name, path, csi, repo, names in files:
        want = scan_sample(path, repo, names)
        for s in SHIFTS:
            _same_scan(scan_sample(csi[s], repo, names), want)


_TASK_KEYS = ("tid", "start", "end", "tstart", "tend", "span", "win_lo", "win_hi")


def _plans(path, repo, names):
    f = bamio.AlignmentFile(path)
    loci = [repo[n] for n in names]
    sites, alts = _site_arrays(repo, names, loci, f)
    y = [("chrY", 2781479, 2781479 + 20000)] if "chrY" in f.references else []
    readlen = f.max_read_len(101)
    kw = dict(pad=SPAN, flank=FLANKMATCH, pe_reach=DNAPE_ELONGATE, span=SPAN)
    f.plan(sites, alts, readlen, extra=y, **kw)
    coff, _, _, _ = f.plan_blocks()
    walks = f.plan_walks(sites, readlen, **kw)
    alt_walks = f.plan_alt_walks(sites, alts, readlen, **kw)
    region_walks = f.plan_region_walks(y)
    # every block the host scan reads for these regions is among the planned ones: scan with all of them preloaded
    n, cb, ob = f.plan(sites, alts, readlen, extra=y, **kw)
    cbuf, obuf = np.zeros(cb + 64, np.uint8), np.zeros(ob + 64, np.uint8)
    coff_arr, ooff = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    f.plan_fill(cbuf.ctypes.data, 0, 0, coff_arr, ooff)
    status = np.zeros(n, np.int32)
    for k in range(n):
        data = zlib.decompressobj(-15).decompress(bytes(cbuf[coff_arr[k]:coff_arr[k + 1]]))
        obuf[ooff[k]:ooff[k] + len(data)] = np.frombuffer(data, np.uint8)
    f.preload(obuf.ctypes.data, ooff, status)
    f.scan(sites, alts, readlen, **kw)
    for g in y:
        f.pileup_depth_sum(*g)
    hits, misses = f.preload_clear()
    f.close()
    return coff, walks, alt_walks, region_walks, hits, misses


def _walkable(tasks, chunks):
    ok = []
    for T in tasks:
        c = chunks[T["chunk_first"]:T["chunk_first"] + max(T["n_chunks"], 0)]
        ok.append(bool(T["n_chunks"] >= 0 and (c["begin_block"] >= T["block_first"]).all() and (c["begin_block"] < T["block_end"]).all()))
    return np.array(ok)


def test_plans_agree_with_the_bai_and_cover_the_scan(files):
    if bamio._native() is None:
        pytest.skip("no native BAM layer")
    for name, path, csi, repo, names in files:
        want = _plans(path, repo, names)
        assert want[5] == 0 and want[4] > 0, name
        for s in SHIFTS:
            got = _plans(csi[s], repo, names)
            for w, g in zip(want[1:4], got[1:4]):
                for k in _TASK_KEYS:
                    assert np.array_equal(w[0][k], g[0][k]), (name, s, k)
                assert (_walkable(*g) >= _walkable(*w)).all(), (name, s)
            assert got[5] == 0 and got[4] > 0, (name, s)               # no block the scan read was missing from the plan


def test_walked_scans_through_the_feeder_agree_with_the_bai(files, monkeypatch):
    """run_many's gpu_walk plumbing over CSI-only files, with tests/walk_model.ModelInflater in the device's place: the scans
    equal the plain scans of the .bai copies, nothing is declined and no scan inflates a block for itself."""
    if bamio._native() is None:
        pytest.skip("no native BAM layer")
    monkeypatch.setattr("tredparse_amd._lib.Inflater", ModelInflater)
    for s in SHIFTS:
        args = [(name, csi[s], repo, names, 300, False, False, True, True, "ERROR") for name, path, csi, repo, names in files]
        t.release_inflaters()
        for k in t.TIMING:
            t.TIMING[k] = 0
        ex = ThreadPoolExecutor(max_workers=2)
        chunks = [args[k:k + 2] for k in range(0, len(args), 2)]
        feeder = t._InflateFeeder(chunks, ex, 0, walk=True)
        try:
            scans = [fut.result() for _ in chunks for fut in feeder.next()[1]]
        finally:
            feeder.close()
            ex.shutdown()
            t.release_inflaters()
        tm = t.TIMING
        assert tm["walk_declined"] == 0 and tm["walk_alt_declined"] == 0 and tm["inflate_misses"] == 0, (s, dict(tm))
        for (name, path, csi, repo, names), got in zip(files, scans):
            _same_scan(got, scan_sample(path, repo, names))


# ---- which index, and what is wrong with it ---------------------------------------------------------------------------
def _one(tmp_path, files, name="wgs0000"):
    src = [f for f in files if f[0] == name][0]
    d = tmp_path / "one"
    d.mkdir()
    dst = str(d / "s.bam")
    shutil.copyfile(src[1], dst)
    return src, dst


def _errors(path):
    out = []
    for cls in _layers():
        f = cls(path)
        try:
            list(f.fetch("chr4", 3000000, 3100000))
            out.append(None)
        except ValueError as e:
            out.append(str(e))
        f.close()
    return out


def test_the_bai_is_taken_when_both_are_there(files, tmp_path):
    src, dst = _one(tmp_path, files)
    shutil.copyfile(src[1] + ".bai", dst + ".bai")
    with open(dst + ".csi", "wb") as fp:
        fp.write(b"not an index")
    assert _errors(dst) == [None] * len(_layers())
    # a valid .csi behind a broken .bai: the .bai is the one read
    bamio.write_csi(dst, min_shift=14)
    with open(dst + ".bai", "wb") as fp:
        fp.write(b"BAX\1")
    assert _errors(dst) == ["bad BAI magic"] * len(_layers())
    # <stem>.csi is found too
    os.remove(dst + ".bai")
    os.rename(dst + ".csi", dst[:-4] + ".csi")
    assert _errors(dst) == [None] * len(_layers())


def test_a_bad_csi_is_reported(files, tmp_path):
    src, dst = _one(tmp_path, files)
    good = open(bamio.write_csi(dst, min_shift=14), "rb").read()
    for data, msg in ((good[:len(good) // 2], "truncated CSI"), (b"", "truncated CSI"),
                      (bamio._bgzf(b"CSJ\1" + gzip.decompress(good)[4:]), "bad CSI magic"),
                      (bamio._bgzf(gzip.decompress(good)[:-200]), "truncated CSI")):
        with open(dst + ".csi", "wb") as fp:
            fp.write(data)
        for got in _errors(dst):
            assert got is not None and "CSI" in got, (msg, got)
    with open(dst + ".csi", "wb") as fp:
        fp.write(bamio._bgzf(b"CSJ\1" + gzip.decompress(good)[4:]))
    assert _errors(dst) == ["bad CSI magic"] * len(_layers())


def test_no_index_gives_the_message_of_before(files, tmp_path):
    _, dst = _one(tmp_path, files)
    assert _errors(dst) == ["no .bai index next to {}".format(dst)] * len(_layers())
    if bamio._native() is not None:
        with pytest.raises(ValueError, match=r"^no \.bai index next to "):
            bamio.NativeAlignmentFile(dst).check_region("chr4", 0, 10)


def test_loading_a_csi_costs_little(files):
    """Open plus the 30 loci's window queries on the whole-genome shaped sample, .csi against .bai (printed: pytest -s)."""
    import time
    if bamio._native() is None:
        pytest.skip("no native BAM layer")
    name, path, csi, repo, names = [f for f in files if f[0] == "wgs0000"][0]
    wins = [(repo[n].chr, repo[n].repeat_start - SPAN, repo[n].repeat_end + SPAN) for n in names]

    def once(p):
        t0 = time.perf_counter()
        f = bamio.NativeAlignmentFile(p)
        for g in wins:
            f.pileup_depth_sum(*g)
        f.close()
        return time.perf_counter() - t0
    best = {k: min(once(p) for _ in range(7)) for k, p in (("bai", path), ("csi", csi[14]))}
    print("open + {} window queries: .bai {:.3f} ms, .csi {:.3f} ms".format(len(wins), 1e3 * best["bai"], 1e3 * best["csi"]))
    assert best["csi"] < best["bai"] + 1e-3
