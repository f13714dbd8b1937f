"""GPU: the Engine's Unit-list entry points (classify, genotype, winners, alignments, consensus, grid_from_counts) against
tests/golden/engine_units.json -- what tools/gen_golden_engine_units.py recorded on an MI355X at the commit before a
Unit list became a PackedUnits (PackedUnits.from_units) and these entry points the packed path.  Two runs of the
generator there agreed byte for byte, floats included, so everything is compared exactly (floats as float.hex()).
And the ladder table: uploaded when it grows, never otherwise."""
import json
import os
import sys

import numpy as np
import pytest

from tredparse_amd.engine import Engine, PackedUnits, Unit
from tredparse_amd.meta import TREDsRepo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_engine_units as gen  # noqa: E402  (the unit lists and what is recorded of them live with the generator)

pytestmark = pytest.mark.gpu
CASES = ("four", "four_clip", "paired", "long")


@pytest.fixture(scope="module")
def golden():
    with open(gen.OUT) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def got(ctx):
    long_engine = Engine(0, long_reads=True)
    try:
        out = gen.record(Engine(ctx=ctx), long_engine)      # (computed once, shared by the tests below)
    finally:
        long_engine.close()
    return json.loads(json.dumps(out))                      # (keys and tuples as the file has them)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("part", ["classify", "genotype", "winners", "alignments", "consensus"])
def test_unit_lists_give_what_they_gave(golden, got, case, part):
    assert sorted(golden["cases"]) == sorted(got["cases"]) == sorted(CASES)
    want, have = golden["cases"][case], got["cases"][case]
    keys = {"classify": ("classify", "dump_shape", "uro"), "genotype": ("genotype", "genotype_no_grid")}.get(part, (part,))
    for k in keys:
        if isinstance(want[k], list) and len(want[k]) == len(have[k]):
            for i, (a, b) in enumerate(zip(want[k], have[k])):            # (unit by unit: a failure names the unit)
                assert a == b, (case, k, i)
        assert want[k] == have[k], (case, k)


def test_what_the_cases_hold(golden):
    """The fixture covers what it was made for: FULL reads at two alleles, partial, repeat-only and untagged reads, a unit
    without reads, a second period, pair ids that discard a pair of repeat-only reads, a long read."""
    four = golden["cases"]["four"]["genotype"]
    assert [len(u["tags"]) for u in four] == [15, 12, 0, 12]
    assert sorted(four[0]["full"]) == ["15", "20"] and four[0]["pref"] and four[0]["rept"] == 1 and 0 in four[0]["tags"]
    assert sorted(four[1]["full"]) == ["12", "14"]
    paired = golden["cases"]["paired"]["genotype"][0]
    assert paired["tags"].count(4) == 3 and paired["rept"] == 1
    assert golden["cases"]["long"]["genotype"][0]["full"] == {"100": 1}


def test_the_odd_reads_text_is_printed_verbatim(golden, got):
    odd = golden[gen.ODD_READ]
    assert got[gen.ODD_READ] == odd and odd[38] == "a" and odd[70] == "R"
    assert golden["odd_in_block"] is True and got["odd_in_block"] is True
    block = got["cases"]["four"]["alignments"][0]["14"]
    assert odd[38:71] in block and block == golden["cases"]["four"]["alignments"][0]["14"]


def test_grid_from_counts_and_the_refusals(golden, got):
    assert got["grid_from_counts"] == golden["grid_from_counts"] and golden["grid_from_counts"]["grid"] is not None
    assert got["refusals"] == golden["refusals"]
    assert golden["refusals"]["mixed_clip_classify"] == ["ValueError", "all units of one batch must share the clip setting"]
    assert golden["refusals"]["read_500_classify"][0] == golden["refusals"]["read_500_genotype"][0] == "TredGpuError"


def test_the_ladder_table_is_uploaded_when_it_grows_and_never_otherwise(ctx, monkeypatch):
    lists, _ = gen.unit_lists()
    four = lists["four"][1]
    uld = TREDsRepo(ref="hg38")["ULD"]
    assert len(uld.repeat) == 12
    reads = gen._cut(gen._genome(uld, 4, 9), [-40, -30, -20, -10], strands="+-")
    b1 = PackedUnits.from_units(four)
    b2 = PackedUnits.from_units([Unit(uld, 150, reads, 30.0, 2, (), ()), four[0]])
    assert set(b2.ladder_keys) - set(b1.ladder_keys) and set(b2.ladder_keys) & set(b1.ladder_keys)
    uploads, upload = [], ctx.set_ladders
    monkeypatch.setattr(ctx, "set_ladders", lambda ladders: (uploads.append(len(ladders)), upload(ladders))[1])
    engine = Engine(ctx=ctx)
    first = engine.genotype_packed(b1)
    w1 = engine.winners(b2)
    again = engine.genotype_packed(b1)
    w2 = engine.winners(b2)
    assert uploads == [3, 4]                                                # one call per growth and none after
    assert len(w1.items) >= 4 + 14 and all(np.array_equal(getattr(w1, k), getattr(w2, k)) for k in ("items", "win", "fields", "ops", "n_ops"))
    for k in ("tag", "h", "score", "rept", "calls", "marg"):
        assert getattr(first, k).tobytes() == getattr(again, k).tobytes(), k
    assert len(first.joint) == len(again.joint) == 4
    for (t1, s1), (t2, s2) in zip(first.joint, again.joint):
        assert t1.tobytes() == t2.tobytes() and s1 == s2


def test_consensus_after_a_longer_ladder_was_registered(ctx, golden):
    """The pileup call is given the whole registered table: a batch whose own templates are shorter than a ladder an
    earlier batch registered (ULD at 150 bp: 192 columns against 186) gets the consensus it got before."""
    four = gen.unit_lists()[0]["four"][1]
    uld = TREDsRepo(ref="hg38")["ULD"]
    longer = PackedUnits.from_units([Unit(uld, 150, gen._cut(gen._genome(uld, 4, 9), [-40, -30], strands="+-"), 30.0, 2, (), ())])
    b = PackedUnits.from_units(four)
    alleles = [sorted(int(a) for a in c) + [0] for c in golden["cases"]["four"]["consensus"]]
    engine = Engine(ctx=ctx)
    before = engine.consensus(b, alleles)
    assert len(engine.winners(longer).items) == 2
    longest = lambda keys: max(ctx._template_len(k) for k in keys)
    assert longest(engine._ladders) == 192 > longest(b.ladder_keys) == 186
    after = engine.consensus(b, alleles)
    for x in (before, after):
        have = [{str(a): c.to_dict() for a, c in sorted(u.items())} for u in x]
        assert json.loads(json.dumps(have)) == golden["cases"]["four"]["consensus"]
