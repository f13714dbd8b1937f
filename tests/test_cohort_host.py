"""The host side of the cohort frequencies (tredparse_amd/cohort.py, Engine.cohort, tred.py --cohort) without a GPU: the
packer, the file pass end to end with Context.cohort replaced by the model (tests/cohort_model.py), the option's refusal,
and the library's symbols."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tredparse_amd import _lib, cohort
from tredparse_amd.engine import Engine
from tredparse_amd.meta import TREDsRepo
from tredparse_amd.models import calc_label
from tredparse_amd.trio import PairList

from . import cohort_model as cm
from . import trio_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class ModelContext(object):
    """_lib.Context with cohort() answered by the model, item by item, into the caller's arrays (as tests/fake_engine.py
    stands in for the genotyping calls); Engine.cohort above it is the real one."""

    def __init__(self):
        self.calls = []

    def set_model(self, step, w):
        pass

    def cohort(self, n_items, item_off, samples, ploidy, allele_off, out_status, out_n_alleles, out_alleles, out_freq, out_count,
               out_trace, out_sample_call, out_sample_values, out_r, iters=cm.ITERS, alpha=cm.ALPHA):
        self.calls.append((n_items, iters, alpha))
        off, a, b, lw = samples
        for i in range(n_items):
            lo, hi = int(item_off[i]), int(item_off[i + 1])
            lists = [(a[off[s]:off[s + 1]], b[off[s]:off[s + 1]], lw[off[s]:off[s + 1]]) for s in range(lo, hi)]
            r = cm.evaluate(lists, ploidy[lo:hi], iters=iters, alpha=alpha)
            out_status[i] = r["status"]
            if r["status"] != cm.OK:
                continue
            A, j0 = len(r["alleles"]), int(allele_off[i])
            assert A <= allele_off[i + 1] - j0
            out_n_alleles[i] = A
            out_alleles[j0:j0 + A], out_freq[j0:j0 + A], out_count[j0:j0 + A], out_trace[i] = r["alleles"], r["freq"], r["count"], r["trace"]
            for s in range(lo, hi):
                if r["call"][s - lo] is not None:
                    out_sample_call[s] = (r["index"][s - lo],) + r["call"][s - lo]
                    out_sample_values[s] = (r["logZ"][s - lo], r["post"][s - lo])
                    out_r[off[s]:off[s + 1]] = r["r"][s - lo]


def test_the_packer():
    p1, p2, p3 = PairList([5, 5], [5, 9], [-1.0, 0.0]), PairList([7], [7], [0.0]), PairList([], [], [])
    item_off, (off, a, b, lw), ploidy, allele_off, members = cohort.pack_cohort([[p1, None, p2], [], [p3, p2]], [2, 2, [2, 1]])
    assert item_off.tolist() == [0, 3, 3, 5] and off.tolist() == [0, 2, 2, 3, 3, 4]
    assert (a.tolist(), b.tolist(), lw.tolist()) == ([5, 5, 7, 7], [5, 9, 7, 7], [-1.0, 0.0, 0.0, 0.0])
    assert ploidy.tolist() == [2, 2, 2, 2, 1] and allele_off.tolist() == [0, 6, 6, 8]
    assert members[0] is p1 and members[1] is None and members[3] is None and members[4] is p2       # an empty list takes no part
    assert (item_off.dtype, off.dtype, a.dtype, lw.dtype, ploidy.dtype, allele_off.dtype) == (np.int64, np.int64, np.int32, np.float64, np.int32, np.int64)
    big = PairList(np.arange(2000), np.arange(2000), -np.arange(2000.0))
    assert cohort.pack_cohort([[big]], [2])[3].tolist() == [0, _lib.COHORT_MAX_ALLELE + 1]          # never more room than alleles
    with pytest.raises(ValueError):
        cohort.pack_cohort([[p1]], [2, 2])


def test_engine_cohort_over_the_model_context():
    ctx = ModelContext()
    engine = Engine(ctx=ctx)
    p1, p2 = PairList([5, 5], [5, 9], [-1.0, 0.0]), PairList([7], [7], [0.0])
    res = engine.cohort([[p1, None, p2], [None, None]], [[2, 2, 1], 2], iters=5, alpha=0.5, tol=1e-3)
    assert ctx.calls == [(2, 5, 0.5)]                               # ONE call for all loci
    want = cm.evaluate([(p1.a, p1.b, p1.lw), None, (p2.a, p2.b, p2.lw)], [2, 2, 1], iters=5, alpha=0.5)
    r = res[0]
    assert r.status == _lib.COHORT_OK and r.alleles.tolist() == [5, 7, 9] and np.array_equal(r.freq, want["freq"])
    assert (r.C, r.n_samples, r.delta, r.converged) == (3, 2, want["delta"], bool(want["delta"] < 1e-3))
    assert r.call == want["call"] and r.post == want["post"] and r.call[1] is None and r.r[1] is None
    assert r.loglik == want["logZ"][0] + want["logZ"][2] and r.trace.shape == (5, 2)
    assert res[1].status == _lib.COHORT_EMPTY and res[1].call == [None, None] and len(res[1].alleles) == 0 and res[1].delta is None
    with pytest.raises(_lib.TredGpuError, match="cohort"):
        engine.cohort([[p1], [PairList([9], [5], [0.0])]], [2, 2])                    # the first refused item raises


SAMPLES = {
    "m1": ("Male", {"HD": (17, 38, {"17,17": 0.2, "17,38": 0.5, "17,41": 0.3}), "SBMA": (22, 22, {"22,22": 0.9, "23,23": 0.1})}),
    "f1": ("Female", {"HD": (17, 17, {"17,17": 1.0}), "SBMA": (20, 24, {"20,24": 0.7, "20,20": 0.3})}),
}


@pytest.fixture()
def work(tmp_path):
    """t001 (HD 15/41) and t002 (DM1 5/66, no HD call) of the golden run, a male and a female with calls at HD and at the
    X-linked SBMA."""
    with open(os.path.join(HERE, "golden", "run_t001_t002.json")) as fp:
        docs = json.load(fp)["samples"]
    for key, (gender, loci) in SAMPLES.items():
        c = {"inferredGender": gender}
        for name, (h1, h2, dist) in loci.items():
            c.update({name + ".1": h1, name + ".2": h2, name + ".P_h1h2": dist})
        docs[key] = c
    for key, c in docs.items():
        with open(str(tmp_path / (key + ".json")), "w") as fw:
            json.dump({"samplekey": key, "bam": key + ".bam", "tredCalls": c}, fw)
    return tmp_path, docs


def test_the_file_pass_end_to_end(work):
    tmp, docs = work
    ctx, repo = ModelContext(), TREDsRepo()
    keys = ["t001", "m1", "t002", "f1"]
    written = cohort.run_cohort([str(tmp / (k + ".json")) for k in keys], str(tmp / "cohort"), Engine(ctx=ctx), repo,
                                loci=["HD", "SBMA", "DM1"], iters=20, alpha=0.5, tol=1e-2)
    assert written == [str(tmp / "cohort.json"), str(tmp / "cohort.calls.tsv")] and ctx.calls == [(3, 20, 0.5)]
    text = open(written[0]).read()
    doc = json.loads(text)
    assert text == json.dumps(doc, sort_keys=True, indent=4, separators=(",", ": ")) + "\n"
    assert doc["params"] == {"iters": 20, "alpha": 0.5, "tol": 1e-2} and doc["samples"] == keys and sorted(doc["loci"]) == ["DM1", "HD", "SBMA"]
    # the model on the same files: t002 has no HD call and takes no part there
    lists = {k: tm.pairs_from_json(docs[k]["HD.P_h1h2"]) for k in ("t001", "m1", "f1")}
    want = cm.evaluate([lists["t001"], lists["m1"], None, lists["f1"]], 2, iters=20, alpha=0.5)
    hd = doc["loci"]["HD"]
    assert sorted(hd) == ["alleles", "chromosomes", "converged", "count", "delta", "exp_carrier", "exp_prerisk", "exp_risk", "freq",
                          "hard_freq", "het_exp", "het_obs", "loglik", "n_samples", "status"]
    assert hd["alleles"] == want["alleles"].tolist() and hd["freq"] == want["freq"].tolist() and hd["count"] == want["count"].tolist()
    assert (hd["chromosomes"], hd["n_samples"], hd["status"]) == (6, 3, "OK")
    assert hd["delta"] == want["delta"] and hd["converged"] == bool(want["delta"] < 1e-2)
    assert abs(hd["loglik"] - sum(z for z in want["logZ"] if z is not None)) < 1e-12
    tred = repo["HD"]
    risk = prerisk = het = 0.0
    for k, s in zip(("t001", "m1", "f1"), (0, 1, 3)):
        for a, b, r in zip(lists[k][0].tolist(), lists[k][1].tolist(), want["r"][s].tolist()):
            risk += r * (calc_label(tred, [a, b]) == "risk")
            prerisk += r * (calc_label(tred, [a, b]) == "prerisk")
            het += r * (a != b)
    assert abs(hd["exp_risk"] - risk) < 1e-12 and abs(hd["exp_prerisk"] - prerisk) < 1e-12 and abs(hd["het_obs"] - het) < 1e-12
    assert 1 < hd["exp_risk"] < 2 and 0 < hd["exp_prerisk"] < 1     # t001's 41 and a share of m1's 41; m1's 38
    assert abs(hd["het_exp"] - 3 * (1 - float((want["freq"] ** 2).sum()))) < 1e-12
    assert hd["exp_carrier"] == 0.0                                 # dominant: a pair past the cut-off is a case, not a carrier
    assert hd["hard_freq"] == {"15": 1, "17": 3, "38": 1, "41": 1}  # what tredreport would count
    # the ploidy rule: Male at an X-linked locus is 1
    sbma = doc["loci"]["SBMA"]
    wx = cm.evaluate([None, tm.pairs_from_json(SAMPLES["m1"][1]["SBMA"][2]), None, tm.pairs_from_json(SAMPLES["f1"][1]["SBMA"][2])],
                     [2, 1, 2, 2], iters=20, alpha=0.5)
    assert (sbma["chromosomes"], sbma["n_samples"]) == (3, 2) and sbma["freq"] == wx["freq"].tolist()
    assert abs(sbma["het_obs"] - wx["r"][3][1]) < 1e-12 and sbma["hard_freq"] == {"20": 1, "22": 2, "24": 1}
    assert (doc["loci"]["DM1"]["n_samples"], doc["loci"]["DM1"]["chromosomes"]) == (1, 2)
    rows = [line.split("\t") for line in open(written[1]).read().splitlines()]
    assert rows[0] == ["SampleKey", "locus", "single", "call", "post", "P_risk", "P_prerisk", "label"]
    assert [(r[0], r[1]) for r in rows[1:]] == [("t001", "HD"), ("m1", "HD"), ("f1", "HD"), ("m1", "SBMA"), ("f1", "SBMA"), ("t002", "DM1")]
    by = {(r[0], r[1]): r for r in rows[1:]}
    m1 = by[("m1", "HD")]
    assert m1[2] == "17|38" and m1[3] == "{}|{}".format(*want["call"][1]) and m1[4] == "{:.6g}".format(want["post"][1])
    assert m1[7] == calc_label(tred, list(want["call"][1])) and abs(float(m1[5]) + float(m1[6]) + want["r"][1][0] - 1) < 1e-5
    assert by[("t001", "HD")][2:4] == ["15|41", "15|41"] and by[("t001", "HD")][7] == "risk"
    assert by[("m1", "SBMA")][2:4] == ["22|22", "22|22"] and by[("t002", "DM1")][2] == "5|66"
    # --tred: those loci alone; the module's defaults
    cohort.run_cohort([str(tmp / "t001.json")], str(tmp / "one"), Engine(ctx=ctx), repo, loci=["HD"])
    one = json.load(open(str(tmp / "one.json")))
    assert sorted(one["loci"]) == ["HD"] and one["params"] == {"iters": 64, "alpha": 1.0, "tol": 1e-6} and ctx.calls[-1] == (1, 64, 1.0)


def test_cohort_with_no_output_is_refused(capsys):
    from tredparse_amd import tred
    with pytest.raises(SystemExit) as e:
        tred.main(["sample.bam", "--cohort", "--no-output"])
    assert e.value.code == 1 and "--cohort" in capsys.readouterr().err
    args = tred.set_argparse().parse_args(["sample.bam", "--cohort", "--cohort-iters", "12", "--cohort-alpha", "0.25"])
    assert (args.cohort, args.cohort_iters, args.cohort_alpha, args.cohort_tol) == (True, 12, 0.25, 1e-6)
    assert tred.set_argparse().parse_args(["sample.bam"]).cohort is False


def test_the_cohort_pass_is_no_read_report():
    from tredparse_amd import runtime
    assert not any("cohort" in name for name in runtime.REPORTS)


def test_cohort_header_symbols_all_exported():
    """include/tredcohort.h: every declared entry point is exported by libtredgpu.so and listed in _lib.COHORT_EXPORTS."""
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tredcohort.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tredcohort_[a-z_]+)\s*\(", src)))
    assert names == sorted(_lib.COHORT_EXPORTS) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r" T (tredcohort_[a-z_]+)", out)) == set(names)
    defines = dict(re.findall(r"#define TREDGPU_(COHORT_[A-Z_]+|KERNEL_COHORT) (\d+)", src))
    assert int(defines["KERNEL_COHORT"]) == _lib.KERNEL_COHORT == 21
    assert int(defines["COHORT_MAX_ALLELE"]) == _lib.COHORT_MAX_ALLELE == cm.MAX_ALLELE == 1024
    assert int(defines["COHORT_MAX_ITERS"]) == _lib.COHORT_MAX_ITERS == cm.MAX_ITERS == 4096
    from . import cohort_cases
    assert int(defines["COHORT_CHUNK"]) == _lib.COHORT_CHUNK == cohort_cases.CHUNK
    assert int(defines["COHORT_LONG_LIST"]) == _lib.COHORT_LONG_LIST == cohort_cases.LONG_LIST
    for name in ("OK", "EMPTY", "TOO_LONG", "BAD_ITEM"):
        assert int(defines["COHORT_" + name]) == getattr(_lib, "COHORT_" + name) == getattr(cm, name)
    assert (_lib.COHORT_ITERS, _lib.COHORT_ALPHA, _lib.COHORT_TOL) == (cm.ITERS, cm.ALPHA, cm.TOL)
