"""GPU: tred.py --pedigree end to end on four small synthetic BAMs of one family at HD -- father 17/30, mother 15/20, a
child 15/30 that fits them and a child 15/36 that does not (alleles 150 bp reads still span; on the CPU, with the model over
grids from oracle/lik_oracle.py for the same seeds, the first child's denovo is 4.7e-4 and the second's 1.0).  Every
<child>.trio.json is the model on the same three JSON files, Engine.trio on the dense grids is the model on those grids, and
without --pedigree the samples' files are what they were."""
import gzip
import json
import os

import numpy as np
import pytest

from tredparse_amd import _lib, synth, synth_bam
from tredparse_amd import tred as tredmod
from tredparse_amd.engine import Engine, PackedUnits
from tredparse_amd.meta import TREDsRepo
from tredparse_amd.runtime import collect_sample

from . import trio_model as tm

pytestmark = pytest.mark.gpu
TOL = 1e-6
FAMILY = {"dad": (101, [17, 30]), "mom": (102, [15, 20]), "kid": (103, [15, 30]), "novo": (104, [15, 36])}     # seed, alleles
PED = "# one family, two children\nf1 dad 0 0 1 1\nf1 mom 0 0 2 1\nf1 kid dad mom 2 1\nf1 novo dad mom 2 2\n"


@pytest.fixture(scope="module")
def engine(ctx):
    return Engine(ctx=ctx)            # on the session's context (tests/conftest.py: it loads PyTorch's HIP runtime first)


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = tmp_path_factory.mktemp("trio_family")
    hd = [l for l in synth.load_loci() if l["name"] == "HD"]
    rows = []
    for key, (seed, alleles) in FAMILY.items():
        recs, _ = synth_bam.simulate_sample(seed, hd, synth.SynthParams(coverage=30), h_pairs=[alleles])
        synth_bam.write_bam(str(d / (key + ".bam")), recs, sample=key)
        rows.append("{},{}".format(key, d / (key + ".bam")))
    (d / "samples.csv").write_text("\n".join(rows) + "\n")
    (d / "family.ped").write_text(PED)
    return d


def _calls(work, key):
    with open(os.path.join(str(work), key + ".json")) as fp:
        return json.load(fp)["tredCalls"]


def test_pedigree_files_equal_the_model_on_the_same_files(engine, family, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr("tredparse_amd.engine.Engine", lambda *a, **k: engine)
    common = [str(family / "samples.csv"), "--tred", "HD", "--quiet-json"]
    engine.ctx.reset_timing()
    tredmod.main(common + ["--workdir", str(tmp_path / "plain")])
    assert engine.ctx.get_timing(_lib.KERNEL_TRIO)[0] == 0
    tredmod.main(common + ["--workdir", str(tmp_path / "ped"), "--pedigree", str(family / "family.ped")])
    assert engine.ctx.get_timing(_lib.KERNEL_TRIO)[0] == 1         # one call for the whole pedigree
    capsys.readouterr()
    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert names == sorted(k + ext for k in FAMILY for ext in (".json", ".tred.vcf.gz"))
    assert sorted(os.listdir(str(tmp_path / "ped"))) == sorted(names + ["kid.trio.json", "novo.trio.json"])
    for name in names:                                              # without --pedigree: byte for byte
        a, b = ((tmp_path / d / name).read_bytes() for d in ("plain", "ped"))
        assert (gzip.decompress(a) == gzip.decompress(b)) if name.endswith(".gz") else (a == b), name
    for key, (_, alleles) in FAMILY.items():
        c = _calls(tmp_path / "ped", key)
        assert [c["HD.1"], c["HD.2"]] == alleles, key
    lists = {key: tm.pairs_from_json(_calls(tmp_path / "ped", key)["HD.P_h1h2"]) for key in FAMILY}
    denovo = {}
    for child in ("kid", "novo"):
        text = (tmp_path / "ped" / (child + ".trio.json")).read_text()
        doc = json.loads(text)
        assert text == json.dumps(doc, sort_keys=True, indent=4, separators=(",", ": ")) + "\n"
        assert (doc["father"], doc["mother"], doc["params"]) == ("dad", "mom", {"mu": 0.01, "rho": 0.9, "beta": 0.5})
        assert sorted(doc["loci"]) == ["HD"]
        got, want = doc["loci"]["HD"], tm.evaluate(lists[child], lists["dad"], lists["mom"])
        assert got["status"] == "OK" and got["call"] == list(want["call"]) == got["single"] == FAMILY[child][1]
        for name in ("post", "denovo", "paternal"):
            assert abs(got[name] - want[name]) <= TOL, (child, name)
        theirs = tm.sparsify(lists[child], want["J"], want["Jmax"], want["S"])
        assert sorted(got["P_h1h2"]) == sorted(theirs) and max(abs(got["P_h1h2"][k] - theirs[k]) for k in theirs) <= TOL
        assert got["label"] == _calls(tmp_path / "ped", child)["HD.label"]
        denovo[child] = got["denovo"]
    assert denovo["kid"] <= 5 * tm.MU and denovo["novo"] >= 0.9

    # Engine.trio on the three dense grids is the model on those grids
    repo = TREDsRepo(ref="hg38")
    scans = [collect_sample((key, str(family / (key + ".bam")), repo, ["HD"], 300, False, False, True, True, "INFO")) for key in FAMILY]
    r = engine.genotype_packed(PackedUnits.from_scans([(s, [0]) for s in scans]), dense=True)
    unit = {key: r.unit(i) for i, key in enumerate(FAMILY)}
    res = engine.trio([unit["kid"], unit["novo"]], [unit["dad"]] * 2, [unit["mom"]] * 2, 2, period=3)
    dense = {key: tm.pairs_from_grid(unit[key].grid, 3) for key in FAMILY}
    worst = 0.0
    for child, x in zip(("kid", "novo"), res):
        want = tm.evaluate(dense[child], dense["dad"], dense["mom"])
        assert (x.status, x.index, x.call) == (tm.OK, want["index"], want["call"]) and list(x.call) == FAMILY[child][1]
        assert np.abs(x.J - want["J"]).max() <= TOL and abs(x.post - want["post"]) <= TOL
        assert abs(x.denovo - want["denovo"]) <= TOL and abs(x.paternal - want["paternal"]) <= TOL
        worst = max(worst, abs(x.denovo - denovo[child]))
    assert res[0].denovo <= 5 * tm.MU and res[1].denovo >= 0.9
    with capsys.disabled():
        print("\nlargest difference of denovo between the dense grids and the files: {:.3g}".format(worst))

    # other parameters reach the kernel, and the module's own command line writes the same files from the same directory
    from tredparse_amd import trio
    monkeypatch.setattr(engine, "close", lambda: None)            # (the command line gives its engine back: not the session's)
    before = (tmp_path / "ped" / "kid.trio.json").read_bytes()
    trio.main([str(family / "family.ped"), "--workdir", str(tmp_path / "ped"), "--tred", "HD"])
    assert (tmp_path / "ped" / "kid.trio.json").read_bytes() == before
    tredmod.main(common + ["--workdir", str(tmp_path / "mu"), "--pedigree", str(family / "family.ped"), "--trio-mu", "0.2"])
    capsys.readouterr()
    doc = json.loads((tmp_path / "mu" / "kid.trio.json").read_text())
    want = tm.evaluate(lists["kid"], lists["dad"], lists["mom"], mu=0.2)
    assert doc["params"]["mu"] == 0.2 and abs(doc["loci"]["HD"]["denovo"] - want["denovo"]) <= TOL and want["denovo"] > denovo["kid"]
