"""CPU: the one-test short-cut of sw_cont_kernel's steady_exit, on the model (tests/sw_tier2_model.py).

Once some read of a wave has a candidate the kernel asks the bounded-gain test alone: a failed test no longer falls through
to the two-boundary test, which cannot fire there.  sw_tier2_model.replay has the short-cut, sw_exit_model.replay has not:
under both tiers every wave sweeps the same columns and leaves every read the same arg-max word -- on a bench-shaped batch
(one sample of the 30 loci) and on the thirteen cases of tests/sw_tier2_gpu_cases.py."""
import numpy as np
import pytest

from tredparse_amd import synth

from . import sw_exit_model as xm
from . import sw_tier2_gpu_cases as t2c
from . import sw_tier2_model as t2


def test_the_short_cut_changes_nothing_on_a_bench_shaped_batch():
    loci = [l for l in synth.load_loci() if l["name"] not in ("FXTAS", "AR")]
    b = synth.build_batch(1, loci, 1, synth.SynthParams(readlen=150))
    read_lad = np.repeat(b.unit_ladder, np.diff(b.unit_read_off))
    tot = {"tier1": 0, "tier2": 0}
    for li, lad in enumerate(b.ladders):
        reads = [synth.decode(b.codes[i]) for i in np.nonzero(read_lad == li)[0]]
        cols = t2.compare_replays(reads, lad, (1, 5, 7, 2), 10)
        for r in tot:
            tot[r] += cols[r]
    print("reads", b.n_reads, "trunk columns", tot)
    assert tot["tier2"] < tot["tier1"]


@pytest.mark.parametrize("name", list(t2c.CASES))
def test_the_short_cut_changes_nothing_on_the_gpu_cases(name):
    lad, L, scoring, clip = t2c.CASES[name]
    ladder = t2c.ladders_of(name)[0]
    R = xm.rows_per_lane(L)
    tot = {"tier1": 0, "tier2": 0}
    for q in t2c.quads_of(name):
        assert len(q) == 4
        cols = t2.compare_replays(q, ladder, scoring, R, clip=bool(clip))
        for r in tot:
            tot[r] += cols[r]
    print(name, "trunk columns", tot)
    assert tot["tier2"] <= tot["tier1"]


def test_the_added_cases_are_what_they_claim():
    """pad131: lanes 13 .. 15 of the 10-row kernel hold at most one read row; subs150: 1, 3 and 8 substitutions against the
    quad's first read; ntail150: Ns only in the last 30 bases."""
    assert all(len(r) == 131 for q in t2c.quads_of("pad131") for r in q)
    for q in t2c.quads_of("subs150"):
        assert [sum(x != y for x, y in zip(q[0], r)) for r in q] == [0, 1, 3, 8]
    ns = [r.count("N") for q in t2c.quads_of("ntail150") for r in q]
    assert sorted(ns) == [0, 0, 3, 4, 5, 6, 10, 12]
    assert all("N" not in r[:-30] for q in t2c.quads_of("ntail150") for r in q)
    assert t2c.CASES["opmd100"][0][1] == "GCN" and xm.rows_per_lane(100) == 7
