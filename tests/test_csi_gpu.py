"""GPU: BAMs that come with only a .csi on the product path -- blocks inflated, pair walks and read selection on the device
(run_many inflate_device=0, gpu_walk=True, gpu_select=True) -- give what their .bai copies give, and the reference's own
run() output on t001 / t002 (tests/golden/run_t001_t002.json).  The host side of the same is in test_csi_index.py."""
import gzip
import json
import os
import shutil

import numpy as np
import pytest

from tredparse_amd import bamio, synth, synth_bam
from tredparse_amd import tred as t
from tredparse_amd.emit import Emitter
from tredparse_amd.engine import Engine
from tredparse_amd.meta import TREDsRepo

from .test_e2e_gpu import _against_reference

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


def _csi_copy(path, d, min_shift):
    os.makedirs(d, exist_ok=True)
    dst = os.path.join(d, os.path.basename(path))
    shutil.copyfile(path, dst)
    bamio.write_csi(dst, min_shift=min_shift)
    return dst


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """(the test_select_gpu-style cohort with .bai, {min_shift: the same files with only a .csi})."""
    root = str(tmp_path_factory.mktemp("csigpu"))
    loci = [l for l in synth.load_loci() if l["name"] in ("HD", "DM1", "SCA1", "AR", "FXS", "FRDA", "SCA17")]
    made = synth_bam.make_bams(os.path.join(root, "bai"), 3, seed=77, loci=loci,
                               p=synth.SynthParams(coverage=30, expanded_max=120, expanded_frac=0.3))
    repo, srepo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites")), TREDsRepo()
    names = [l["name"] for l in loci]
    args = [(s, os.path.join(GOLD, "bam", s + ".bam"), repo, sorted(repo.names), 300, False, False, True, True, "ERROR") for s in ("t001", "t002")]
    args += [(key, path, srepo, names, 300, False, False, True, True, "ERROR") for key, path, _ in made]
    recs, _ = synth_bam.simulate_sample(78, loci[:4], synth.SynthParams(coverage=20, expanded_max=120, expanded_frac=0.3))
    rng = np.random.default_rng(78)
    recs.flag[rng.random(len(recs.flag)) < 0.03] |= 0x400
    recs.flag[rng.random(len(recs.flag)) < 0.05] ^= 0x10
    for block in (300, 20000):
        path = os.path.join(root, "bai", "cut{}.bam".format(block))
        synth_bam.write_bam(path, recs, sample="cut", block=block, split_records=True)
        args.append(("cut{}".format(block), path, srepo, names[:4], 300, False, False, True, True, "ERROR"))
    wgs = synth_bam.make_bams(os.path.join(root, "bai"), 1, seed=79, loci=loci, prefix="wgs", wgs_like=True)[0]
    args.append((wgs[0], wgs[1], srepo, names, 300, False, False, True, True, "ERROR"))
    args.append(("noalts", os.path.join(GOLD, "bam", "t001.bam"), repo, ["HD", "DM1", "AR"], 300, False, False, False, True, "ERROR"))
    csi = {}
    for s in (12, 14, 16):
        d = os.path.join(root, "csi{}".format(s))
        csi[s] = [(a[0], _csi_copy(a[1], d, s)) + a[2:] for a in args]
    return args, csi


def _run(args, engine):
    for k in t.TIMING:
        t.TIMING[k] = 0
    try:
        out = t.run_many(args, engine, batch=4, threads=3, inflate_device=0, gpu_walk=True, gpu_select=True)
    finally:
        t.release_inflaters()
    return out, dict(t.TIMING)


def _strip(r):
    r = dict(r)
    r.pop("bam", None)
    return r


def test_product_path_over_csi_only_files_equals_the_bai_run(cohort, engine):
    args, csi = cohort
    want, tw = _run(args, engine)
    assert tw["select_samples"] == len(args) and tw["select_declined"] == 0
    for s in (12, 14, 16):
        got, tg = _run(csi[s], engine)
        assert [r["samplekey"] for r in got] == [a[0] for a in args]
        assert [_strip(r) for r in got] == [_strip(r) for r in want], s
        assert tg["select_samples"] == len(args) and tg["select_declined"] == 0, (s, tg)
        assert tg["walk_declined"] <= tw["walk_declined"] and tg["inflate_misses"] <= tw["inflate_misses"], (s, tg, tw)
        assert tg["inflate_failed"] == 0


def test_native_writer_over_csi_only_files_writes_the_same_bytes(cohort, engine, tmp_path, monkeypatch):
    args, csi = cohort
    args = [a for a in args if a[0] != "noalts"][:6]
    texts = {}
    for kind, run in (("bai", args), ("csi", [c for c in csi[14] if c[0] != "noalts"][:6])):
        d = tmp_path / kind
        d.mkdir()
        monkeypatch.chdir(d)
        emit = Emitter("hg38", args[0][2], list(args[0][3]), workers=2)
        try:
            t.run_many(run[:2], engine, batch=2, threads=3, inflate_device=0, gpu_walk=True, gpu_select=True, emit=emit)
        finally:
            emit.close()
            t.release_inflaters()
        texts[kind] = [(open(d / (a[0] + ".json")).read().replace(os.path.dirname(r[1]), "DIR"),
                        gzip.open(d / (a[0] + ".tred.vcf.gz"), "rb").read().replace(os.path.dirname(r[1]).encode(), b"DIR"))
                       for a, r in zip(args[:2], run[:2])]
    assert texts["csi"] == texts["bai"]


def test_csi_only_t001_t002_against_the_reference(cohort, engine):
    want = json.load(open(os.path.join(GOLD, "run_t001_t002.json")))["samples"]
    _, csi = cohort
    for s in (12, 14, 16):
        got, tm = _run([a for a in csi[s] if a[0] in ("t001", "t002")], engine)
        assert tm["select_declined"] == 0
        for r in got:
            _against_reference(r["tredCalls"], want[r["samplekey"]])


def test_cli_on_a_csi_only_bam_writes_what_the_bai_copy_writes(engine, tmp_path, monkeypatch):
    src = os.path.join(GOLD, "bam", "t001.bam")
    bai_dir, csi_dir = tmp_path / "b", tmp_path / "c"
    bai_dir.mkdir()
    shutil.copyfile(src, bai_dir / "t001.bam")
    shutil.copyfile(src + ".bai", bai_dir / "t001.bam.bai")
    csi = _csi_copy(src, str(csi_dir), 14)
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    out = {}
    for kind, bam in (("bai", str(bai_dir / "t001.bam")), ("csi", csi)):
        monkeypatch.chdir(tmp_path)
        work = tmp_path / ("w" + kind)
        t.main([bam, "--workdir", str(work)], quiet=True)
        out[kind] = (open(work / "t001.json").read().replace(os.path.dirname(bam), "DIR"),
                     gzip.open(work / "t001.tred.vcf.gz", "rb").read().replace(os.path.dirname(bam).encode(), b"DIR"))
    assert '"HD.2": 41' in out["csi"][0]
    assert out["csi"] == out["bai"]
