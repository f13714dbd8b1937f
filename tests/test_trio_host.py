"""The host side of the trio evaluation (tredparse_amd/trio.py, tred.py --pedigree) without a GPU: the PED parser, the pair
lists from their two sources, the file pass end to end with the kernel call replaced by the model (tests/trio_model.py),
the option's refusal, and the library's symbols."""
import json
import logging
import os
import re
import subprocess

import numpy as np
import pytest

from tredparse_amd import _lib, trio
from tredparse_amd.meta import TREDsRepo

from . import trio_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class ModelEngine(object):
    """engine.Engine.trio with the kernel call replaced by the model (as tests/fake_engine.py stands in for the genotyping
    calls): the same members in, trio.TrioResult out."""

    def __init__(self):
        self.calls = []

    def trio(self, children, fathers, mothers, ploidy, period=None, mu=tm.MU, rho=tm.RHO, beta=tm.BETA):
        self.calls.append(len(children))
        as_tuple = lambda m: None if m is None else (m.a, m.b, m.lw)
        out = []
        for c, f, m, pl in zip(children, fathers, mothers, ploidy):
            r = tm.evaluate(as_tuple(c), as_tuple(f), as_tuple(m), ploidy=pl, mu=mu, rho=rho, beta=beta)
            out.append(trio.TrioResult(r["status"], (r["index"],) + tuple(r["call"]),
                                       (r["Jmax"], r["S"], r["denovo"] or 0.0, r["paternal"] or 0.0), r["J"], c))
        return out


def test_ped_parser(tmp_path):
    text = ["# family of three", "fam kid dad mom 1 2", "", "fam dad 0 0 1 1   # the father", "fam\tmom\t0\t0\t2\t1",
            "fam2 duo 0 mom2 2 -9"]
    people = trio.read_ped(text)
    assert [(p.key, p.father, p.mother, p.sex) for p in people] == [("kid", "dad", "mom", "1"), ("dad", None, None, "1"),
                                                                    ("mom", None, None, "2"), ("duo", None, "mom2", "2")]
    path = tmp_path / "f.ped"
    path.write_text("\n".join(text) + "\n")
    assert [p.key for p in trio.read_ped(str(path))] == ["kid", "dad", "mom", "duo"]
    with pytest.raises(ValueError, match="columns"):
        trio.read_ped(["fam kid dad mom 1"])
    with pytest.raises(ValueError, match="columns"):
        trio.read_ped(["fam kid dad mom 1 2 3"])
    with pytest.raises(ValueError, match="own parent"):
        trio.read_ped(["fam kid kid mom 1 2"])
    with pytest.raises(ValueError, match="twice"):
        trio.read_ped(["fam kid 0 mom 1 2", "fam kid dad 0 1 2"])


@pytest.fixture(scope="module")
def grids():
    with open(os.path.join(HERE, "golden", "grid.json")) as fp:
        cases = json.load(fp)["cases"]
    z = np.load(os.path.join(HERE, "golden", "grid.npz"))
    return {c["name"]: z["mls_%d" % i] for i, c in enumerate(cases) if "mls_%d" % i in z.files}


def test_pair_list_from_a_dense_grid(grids):
    for name in ("hd_dup_axis", "hd_typical", "hd_homo", "hd_empty"):
        p = trio.PairList.from_grid(grids[name], 3)
        a, b, lw = tm.pairs_from_grid(grids[name], 3)
        assert np.array_equal(p.a, a) and np.array_equal(p.b, b) and np.array_equal(p.lw, lw), name
        assert (p.a.dtype, p.b.dtype, p.lw.dtype) == (np.int32, np.int32, np.float64)
    p = trio.PairList.from_grid(grids["hd_dup_axis"], 3)
    assert len(p) < len(grids["hd_dup_axis"]) == 206                # the grid lists pairs twice: the first occurrence is kept
    assert len(set(zip(p.a.tolist(), p.b.tolist()))) == len(p) and p.lw.max() == 0.0 and (p.a <= p.b).all()
    g = grids["hd_dup_axis"]
    first = {}
    for k, (h1, h2) in enumerate(g[:, :2].astype(int) // 3):
        first.setdefault((h1, h2), k)
    ml = ((g[:, 2] + g[:, 3]) + g[:, 4]) + g[:, 5]
    assert np.array_equal(p.lw, ml[sorted(first.values())] - ml.max())
    assert trio.member_list(trio.PairList.from_grid(grids["hd_empty"], 3)) is None


def test_pair_list_from_a_json_dictionary():
    d = {"15,41": 0.5, "9,100": 0.125, "15,40": 0.25, "10,11": 0.125}
    p = trio.PairList.from_json(d)
    assert list(zip(p.a.tolist(), p.b.tolist())) == [(9, 100), (10, 11), (15, 40), (15, 41)]     # numeric order, not text order
    assert np.allclose(p.lw, np.log([0.25, 0.25, 0.5, 1.0]), atol=1e-15) and p.lw.max() == 0.0
    for x, y in zip((p.a, p.b, p.lw), tm.pairs_from_json(d)):
        assert np.array_equal(x, y)
    assert len(trio.PairList.from_json("")) == 0 and len(trio.PairList.from_json({})) == 0


@pytest.fixture()
def family(tmp_path):
    """t001 and t002 of the golden run as mother and father of `kid`; t002, which has no HD call of its own, is given a
    plain 15/15, and kid's file is t001's with a longer HD allele made the more likely one.  `solo` and its mother `nobody`
    are named in the pedigree and have no file."""
    with open(os.path.join(HERE, "golden", "run_t001_t002.json")) as fp:
        samples = json.load(fp)["samples"]
    assert samples["t002"]["HD.1"] == -1 and samples["t001"]["DM1.1"] == -1 and samples["t002"]["DM1.1"] == 5
    samples["t002"].update({"HD.1": 15, "HD.2": 15, "HD.P_h1h2": {"15,15": 1.0}})
    kid = dict(samples["t001"])
    kid["HD.P_h1h2"] = {"15,41": 0.3, "15,47": 0.4, "15,60": 0.3}
    kid["HD.1"], kid["HD.2"] = 15, 47
    for key, calls in (("t001", samples["t001"]), ("t002", samples["t002"]), ("kid", kid)):
        with open(str(tmp_path / (key + ".json")), "w") as fw:
            json.dump({"samplekey": key, "bam": key + ".bam", "tredCalls": calls}, fw)
    ped = tmp_path / "family.ped"
    ped.write_text("# one trio and a duo\nf1 kid t002 t001 1 2\nf1 t001 0 0 2 1\nf1 t002 0 0 1 1\nf2 solo 0 nobody 2 1\n")
    return tmp_path, str(ped), samples, kid


def test_the_file_pass_end_to_end(family, caplog):
    work, ped, samples, kid = family
    engine, repo = ModelEngine(), TREDsRepo()
    with caplog.at_level(logging.WARNING):
        written = trio.run_pedigree(ped, str(work), engine, repo, mu=0.02)
    assert written == [str(work / "kid.trio.json")] and engine.calls == [len([n for n in repo.names if n + ".1" in kid])]
    messages = " ".join(r.getMessage() for r in caplog.records)
    assert "`solo`" in messages and "`nobody`" in messages         # neither has a file
    assert "`kid`" in messages and "`t002`" in messages             # the pedigree says Male, the reads say Female
    text = open(written[0]).read()
    doc = json.loads(text)
    assert text == json.dumps(doc, sort_keys=True, indent=4, separators=(",", ": ")) + "\n"
    assert sorted(doc) == ["father", "loci", "mother", "params", "samplekey"]
    assert (doc["father"], doc["mother"], doc["samplekey"]) == ("t002", "t001", "kid")
    assert doc["params"] == {"mu": 0.02, "rho": 0.9, "beta": 0.5}
    hd = doc["loci"]["HD"]
    assert sorted(hd) == ["P_h1h2", "call", "denovo", "label", "paternal", "post", "single", "status"]
    # the model on the same three files: the father can only have given 15, the mother's 41 is far likelier than her 47
    child, father, mother = (tm.pairs_from_json(x["HD.P_h1h2"]) for x in (kid, samples["t002"], samples["t001"]))
    r = tm.evaluate(child, father, mother, mu=0.02)
    assert hd["single"] == [15, 47] and hd["call"] == list(r["call"]) == [15, 41] and hd["status"] == "OK"
    assert hd["label"] == "risk"
    for name in ("post", "denovo", "paternal"):
        assert abs(hd[name] - r[name]) <= 1e-12
    assert hd["P_h1h2"] == tm.sparsify(child, r["J"], r["Jmax"], r["S"]) and abs(sum(hd["P_h1h2"].values()) - 1) < 1e-12
    # a locus the child's file has no call at: nothing to evaluate
    dm1 = doc["loci"]["DM1"]
    assert kid["DM1.1"] == -1 and dm1["status"] == "EMPTY_CHILD" and dm1["call"] == [-1, -1] and dm1["label"] == "missing"
    assert dm1["post"] is None and dm1["denovo"] is None and dm1["P_h1h2"] == ""
    # --tred: those loci alone
    trio.run_pedigree(ped, str(work), engine, repo, loci=["HD"])
    assert sorted(json.load(open(written[0]))["loci"]) == ["HD"] and engine.calls[-1] == 1


def test_pedigree_with_no_output_is_refused(tmp_path, capsys):
    from tredparse_amd import tred
    with pytest.raises(SystemExit) as e:
        tred.main(["sample.bam", "--pedigree", str(tmp_path / "family.ped"), "--no-output"])
    assert e.value.code == 1 and "--pedigree" in capsys.readouterr().err
    args = tred.set_argparse().parse_args(["sample.bam", "--pedigree", "f.ped", "--trio-mu", "0.05", "--trio-beta", "1"])
    assert (args.pedigree, args.trio_mu, args.trio_rho, args.trio_beta) == ("f.ped", 0.05, 0.9, 1.0)
    assert tred.set_argparse().parse_args(["sample.bam"]).pedigree is None


def test_the_trio_pass_is_no_read_report():
    from tredparse_amd import runtime
    assert not any("trio" in name for name in runtime.REPORTS)


def test_trio_header_symbols_all_exported():
    """include/tredtrio.h: every declared entry point is exported by libtredgpu.so and listed in _lib.TRIO_EXPORTS."""
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tredtrio.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tredtrio_[a-z_]+)\s*\(", src)))
    assert names == sorted(_lib.TRIO_EXPORTS) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r" T (tredtrio_[a-z_]+)", out)) == set(names)
    defines = dict(re.findall(r"#define TREDGPU_(TRIO_[A-Z_]+|KERNEL_TRIO) (\d+)", src))
    assert int(defines["KERNEL_TRIO"]) == _lib.KERNEL_TRIO == 20 and int(defines["TRIO_MAX_ALLELE"]) == _lib.TRIO_MAX_ALLELE >= 1024
    assert int(defines["TRIO_PAIR_CHUNK"]) == _lib.TRIO_PAIR_CHUNK and int(defines["TRIO_GAMETE_TILE"]) == _lib.TRIO_GAMETE_TILE
    for name in ("OK", "EMPTY_CHILD", "DEGENERATE", "TOO_LONG", "BAD_ITEM"):
        assert int(defines["TRIO_" + name]) == getattr(_lib, "TRIO_" + name) == getattr(tm, name)
    assert (_lib.TRIO_MU, _lib.TRIO_RHO, _lib.TRIO_BETA) == (tm.MU, tm.RHO, tm.BETA) and tm.MAX_ALLELE == _lib.TRIO_MAX_ALLELE
