"""GPU: tred.py --cohort end to end on four small synthetic HD BAMs -- 17/30, 15/20, 15/30 and 15/36, the seeds and alleles
of tests/test_trio_cli_gpu.py (alleles 150 bp reads still span, checked there on the CPU with grids from
oracle/lik_oracle.py).  cohort.json and cohort.calls.tsv are the model (tests/cohort_model.py) on the same four JSON files,
Engine.cohort on the dense grids is the model on those grids, and without --cohort the samples' files are what they were."""
import gzip
import json
import os

import numpy as np
import pytest

from tredparse_amd import _lib, synth, synth_bam
from tredparse_amd import tred as tredmod
from tredparse_amd.engine import Engine, PackedUnits
from tredparse_amd.meta import TREDsRepo
from tredparse_amd.models import calc_label
from tredparse_amd.runtime import collect_sample

from . import cohort_model as cm
from . import trio_model as tm

pytestmark = pytest.mark.gpu
TOL = 1e-6
COHORT = {"s1": (101, [17, 30]), "s2": (102, [15, 20]), "s3": (103, [15, 30]), "s4": (104, [15, 36])}     # seed, alleles


@pytest.fixture(scope="module")
def engine(ctx):
    return Engine(ctx=ctx)            # on the session's context (tests/conftest.py: it loads PyTorch's HIP runtime first)


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("cohort_bams")
    hd = [l for l in synth.load_loci() if l["name"] == "HD"]
    rows = []
    for key, (seed, alleles) in COHORT.items():
        recs, _ = synth_bam.simulate_sample(seed, hd, synth.SynthParams(coverage=30), h_pairs=[alleles])
        synth_bam.write_bam(str(d / (key + ".bam")), recs, sample=key)
        rows.append("{},{}".format(key, d / (key + ".bam")))
    (d / "samples.csv").write_text("\n".join(rows) + "\n")
    return d


def _calls(work, key):
    with open(os.path.join(str(work), key + ".json")) as fp:
        return json.load(fp)["tredCalls"]


def _printed(text, want):
    """A value printed with six significant digits against the model's."""
    return abs(float(text) - want) <= TOL + 5e-6 * abs(want)


def _same_files(work, lists, iters=cm.ITERS, alpha=cm.ALPHA):
    """cohort.json and cohort.calls.tsv of `work` against the model on the lists of the samples' files."""
    want = cm.evaluate([lists[k] for k in COHORT], 2, iters=iters, alpha=alpha)
    text = (work / "cohort.json").read_text()
    doc = json.loads(text)
    assert text == json.dumps(doc, sort_keys=True, indent=4, separators=(",", ": ")) + "\n"
    assert doc["params"] == {"iters": iters, "alpha": alpha, "tol": 1e-6} and doc["samples"] == list(COHORT) and sorted(doc["loci"]) == ["HD"]
    hd = doc["loci"]["HD"]
    assert hd["status"] == "OK" and hd["alleles"] == want["alleles"].tolist() and (hd["chromosomes"], hd["n_samples"]) == (8, 4)
    assert np.abs(np.array(hd["freq"]) - want["freq"]).max() <= TOL and np.abs(np.array(hd["count"]) - want["count"]).max() <= TOL
    assert abs(hd["loglik"] - sum(want["logZ"])) <= TOL and abs(hd["delta"] - want["delta"]) <= TOL
    tred = TREDsRepo(ref="hg38")["HD"]
    weight = lambda select: sum(float(r[[bool(select(a, b)) for a, b in zip(lists[k][0].tolist(), lists[k][1].tolist())]].sum())
                                for k, r in zip(COHORT, want["r"]))
    assert abs(hd["exp_risk"] - weight(lambda a, b: calc_label(tred, [a, b]) == "risk")) <= TOL
    assert abs(hd["exp_prerisk"] - weight(lambda a, b: calc_label(tred, [a, b]) == "prerisk")) <= TOL
    assert abs(hd["het_obs"] - weight(lambda a, b: a != b)) <= TOL and abs(hd["het_exp"] - 4 * (1 - float((want["freq"] ** 2).sum()))) <= TOL
    assert hd["hard_freq"] == {"15": 3, "17": 1, "20": 1, "30": 2, "36": 1}
    rows = [line.split("\t") for line in (work / "cohort.calls.tsv").read_text().splitlines()]
    assert rows[0] == ["SampleKey", "locus", "single", "call", "post", "P_risk", "P_prerisk", "label"] and len(rows) == 5
    for row, (key, (_, alleles)), call, post, gap in zip(rows[1:], COHORT.items(), want["call"], want["post"], want["gap"]):
        assert gap > 1e-5 and row[:4] == [key, "HD", "{}|{}".format(*alleles), "{}|{}".format(*call)], key
        assert _printed(row[4], post) and row[7] == calc_label(tred, list(call)), key
    return hd, want


def test_cohort_files_equal_the_model_on_the_same_files(engine, bams, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    common = [str(bams / "samples.csv"), "--tred", "HD", "--quiet-json"]
    engine.ctx.reset_timing()
    tredmod.main(common + ["--workdir", str(tmp_path / "plain")])
    assert engine.ctx.get_timing(_lib.KERNEL_COHORT)[0] == 0
    tredmod.main(common + ["--workdir", str(tmp_path / "cohort"), "--cohort"])
    assert engine.ctx.get_timing(_lib.KERNEL_COHORT)[0] == 1       # one call for all loci
    capsys.readouterr()
    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert names == sorted(k + ext for k in COHORT for ext in (".json", ".tred.vcf.gz"))
    assert sorted(os.listdir(str(tmp_path / "cohort"))) == sorted(names + ["cohort.json", "cohort.calls.tsv"])
    for name in names:                                              # without --cohort: byte for byte
        a, b = ((tmp_path / d / name).read_bytes() for d in ("plain", "cohort"))
        assert (gzip.decompress(a) == gzip.decompress(b)) if name.endswith(".gz") else (a == b), name
    for key, (_, alleles) in COHORT.items():
        c = _calls(tmp_path / "cohort", key)
        assert [c["HD.1"], c["HD.2"]] == alleles, key
    lists = {key: tm.pairs_from_json(_calls(tmp_path / "cohort", key)["HD.P_h1h2"]) for key in COHORT}
    hd, want = _same_files(tmp_path / "cohort", lists)
    f = dict(zip(hd["alleles"], hd["freq"]))
    assert f[15] > f[30] > f[36] > 0.05 and abs(sum(hd["freq"]) - 1) < 1e-9        # three, two and one of eight chromosomes

    # Engine.cohort on the four dense grids is the model on those grids
    repo = TREDsRepo(ref="hg38")
    scans = [collect_sample((key, str(bams / (key + ".bam")), repo, ["HD"], 300, False, False, True, True, "INFO")) for key in COHORT]
    r = engine.genotype_packed(PackedUnits.from_scans([(s, [0]) for s in scans]), dense=True)
    units = [r.unit(i) for i in range(len(COHORT))]
    res = engine.cohort([units], [2], period=3)[0]
    dense = [tm.pairs_from_grid(u.grid, 3) for u in units]
    model = cm.evaluate(dense, 2)
    assert res.status == cm.OK and res.alleles.tolist() == model["alleles"].tolist() and (res.C, res.n_samples) == (8, 4)
    assert np.abs(res.freq - model["freq"]).max() <= TOL and np.abs(res.count - model["count"]).max() <= TOL
    assert np.abs(res.trace - model["trace"]).max() <= TOL and min(model["gap"]) > 1e-5
    assert res.call == model["call"] and res.index == model["index"]
    for s in range(4):
        assert abs(res.post[s] - model["post"][s]) <= TOL and abs(res.logZ[s] - model["logZ"][s]) <= TOL
        assert np.abs(res.r[s] - model["r"][s]).max() <= TOL
    with capsys.disabled():
        print("\ncohort calls {} (files) {} (dense grids); largest difference of f between the two: {:.3g}".format(
            want["call"], model["call"], max(abs(f.get(int(c), 0.0) - float(x)) for c, x in zip(res.alleles, res.freq) if x > 1e-3)))

    # other parameters reach the kernel, and the module's own command line writes the same files from the same directory
    from tredparse_amd import cohort
    monkeypatch.setattr(engine, "close", lambda: None)            # (the command line gives its engine back: not the session's)
    before = [(tmp_path / "cohort" / n).read_bytes() for n in ("cohort.json", "cohort.calls.tsv")]
    cohort.main([str(tmp_path / "cohort" / (k + ".json")) for k in COHORT] + ["--out", str(tmp_path / "again"), "--tred", "HD"])
    capsys.readouterr()
    assert [(tmp_path / n).read_bytes() for n in ("again.json", "again.calls.tsv")] == before
    tredmod.main(common + ["--workdir", str(tmp_path / "few"), "--cohort", "--cohort-iters", "3", "--cohort-alpha", "4"])
    capsys.readouterr()
    few, _ = _same_files(tmp_path / "few", lists, iters=3, alpha=4.0)
    assert max(few["freq"]) < max(hd["freq"])                       # four pseudo-chromosomes instead of one pull towards 1 / A
