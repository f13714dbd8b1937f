"""GPU, the long-read path through the product path (Engine(long_reads=True) -> run_many(long_reads=True) -> the composed
SW / tally / grid of Context.genotype_batch_joint): the reference's run() on synthetic BAMs of 600 and 1 000 bp reads
(tests/golden/run_long.json, tools/gen_golden.py long), and the reference's own test BAMs, where the switch changes
nothing."""
import hashlib
import json
import os

import numpy as np
import pytest

from tredparse_amd import synth, synth_bam, tred as tredmod
from tredparse_amd.engine import Engine
from tredparse_amd.meta import TREDsRepo

from .test_flags_gpu import _compare

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# tools/gen_golden.py LONG_SAMPLES (the samples are regenerated from their seeds; the golden holds the records' digest)
LONG_SAMPLES = {
    "synlong600": (["HD", "DM1", "ULD", "SCA10"],
                   dict(coverage=6.0, readlen=600, ins_mean=900.0, ins_sd=60.0, min_units=10, max_units=260), 0.3),
    "synlong1000": (["HD", "FXS"],
                    dict(coverage=5.0, readlen=1000, ins_mean=1400.0, ins_sd=80.0, min_units=10, max_units=400), 0.3),
}


@pytest.fixture(scope="module")
def long_engine(ctx):
    e = Engine(0, long_reads=True)
    yield e
    e.close()


def _args(name, bam, repo, names):
    return (name, bam, repo, names, 300, False, False, True, True, "INFO")


@pytest.mark.parametrize("name", sorted(LONG_SAMPLES))
def test_long_samples_match_reference(long_engine, tmp_path, name):
    gold = json.load(open(os.path.join(GOLD, "run_long.json")))["samples"][name]
    names, kw, alt_rate = LONG_SAMPLES[name]
    loci = [l for l in synth.load_loci() if l["name"] in names]
    assert [l["name"] for l in loci] == gold["loci"]
    recs, h_true = synth_bam.simulate_sample(gold["seed"], loci, synth.SynthParams(**kw), alt_rate=alt_rate)
    h = hashlib.sha256()
    for k in recs.FIELDS:
        h.update(np.ascontiguousarray(getattr(recs, k)).tobytes())
    assert h.hexdigest() == gold["records_sha256"], "the synthetic generator no longer reproduces the golden's sample"
    bam = str(tmp_path / (name + ".bam"))
    synth_bam.write_bam(bam, recs, sample=name, level=1)
    repo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
    scan = tredmod.collect_sample(_args(name, bam, repo, gold["loci"]), long_reads=True)
    assert scan.readlen == kw["readlen"] and not scan.dropped          # no unit lost to a length limit
    off = tredmod.collect_sample(_args(name, bam, repo, gold["loci"]))
    assert off.dropped                                                  # (without the switch some are)
    got = tredmod.run_many([_args(name, bam, repo, gold["loci"])], long_engine, long_reads=True)[0]["tredCalls"]
    want = gold["tredCalls"]
    for k in list(got):
        if k.endswith(".details"):
            got[k] = [[d["id"], d["tag"], int(d["h"])] for d in got[k]]
    _compare(got, want, name)
    assert all(got[n + ".1"] > 0 for n in gold["loci"])                # a call at every locus


def test_reference_bams_unchanged_by_the_switch(long_engine):
    """t001 / t002 (150 bp, every locus): run_many with the long-read path on gives the plain engine's bytes."""
    repo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
    args = [_args(s, os.path.join(GOLD, "bam", s + ".bam"), repo, list(repo.names)) for s in ("t001", "t002")]
    plain = Engine(0)
    try:
        want = tredmod.run_many(args, plain, batch=2)
    finally:
        plain.close()
    got = tredmod.run_many(args, long_engine, batch=2)
    assert [json.dumps(r["tredCalls"], sort_keys=True) for r in got] == [json.dumps(r["tredCalls"], sort_keys=True) for r in want]
