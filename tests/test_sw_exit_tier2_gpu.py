"""The second tier of sw_cont_kernel's bounded-gain exit (csrc/sw_ladder.hip: steady_exit, SW_EXIT_BOUND = 2; the per-lane
tail counts read_class_kernel leaves in SwArgs::read_tail) through tredgpu_sw_classify.

Per case (tests/sw_tier2_gpu_cases.py: the nine cases of tests/test_sw_exit_gpu.py and four that aim at the table -- reads
whose last lanes are padding, substitutions inside the repeat, Ns in the tail, the N ladder at 100 bp), quads of four reads:

* every read's tag, h and score from the production launches equal the oracle's classification, the arg-max of the
  kernel's own unpruned per-template dump, and the results of the library that holds the first tier only
  (libtredgpu_tier1.so, run once in a child process through TREDGPU_LIB);
* the trunk-column counter is strictly lower than that library's where the CPU model (tests/sw_exit_model.py, rule "tier2"
  against "tier1") says some wave leaves earlier, and equal where it says none does -- which includes the scoring outside the
  6-mer premise (the table holds 255 there) and the instantiations that do not hold the test.  Direction only: the model's
  absolute columns are not the device's in every case.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from tredparse_amd import _lib

from . import sw_exit_model as xm
from . import sw_tier2_gpu_cases as cs
from . import sw_tier2_model as t2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIER1 = os.path.join(ROOT, "tredparse_amd", "libtredgpu_tier1.so")
_BASE = {}


def _baseline():
    """every case through the library with the first tier only: one child process for all of them"""
    if not _BASE:
        assert os.path.exists(TIER1), "libtredgpu_tier1.so is missing: build() makes it"
        env = dict(os.environ, TREDGPU_LIB=TIER1)
        out = subprocess.run([sys.executable, "-m", "tests.sw_tier2_gpu_cases"], cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [l for l in out.stdout.splitlines() if l.startswith("SW_TIER2_CASES ")][-1]
        _BASE.update(json.loads(line[len("SW_TIER2_CASES "):]))
        assert _BASE["lib"] == TIER1
    return _BASE


def _argmax_of_dump(dump, mu):
    out = np.zeros((dump.shape[0], 3), np.int64)
    for i in range(dump.shape[0]):
        best = None
        for k in range(2 * mu):
            u, s = k // 2 + 1, k % 2
            score, tag = int(dump[i, k, 0]), int(dump[i, k, 5])
            if tag != _lib.TAG_NONE and (best is None or (score, -u, -s) > best[:3]):
                best = (score, -u, -s, tag)
        if best:
            out[i] = (best[3], -best[1], best[0])
    return out


@pytest.mark.parametrize("name", list(cs.CASES))
def test_results_and_trunk_columns(ctx, name):
    lad, L, scoring, clip = cs.CASES[name]
    quads = cs.quads_of(name)
    ladders = cs.ladders_of(name)
    mu = ladders[0][3]
    R = xm.rows_per_lane(L)
    assert all(len(q) == 4 for q in quads)
    model = t2.model_columns(quads, ladders[0], scoring, R, ("old", "tier1", "tier2"), clip=bool(clip))
    got, cols, _ = cs.run_case(ctx, name)
    got2, _, dump = cs.run_case(ctx, name, dump=True)
    base = _baseline()[name]
    print(name, "reads", len(got), "trunk columns: head", cols, "first tier only", base["trunk_cols"], "model", model)
    reads = [r for q in quads for r in q]
    want = po.classify(reads, np.repeat(np.arange(len(quads)), 4).astype(np.int32), po.LocusSet(ladders), clip=bool(clip),
                       scoring=scoring, threads=4).astype(np.int64)
    assert np.array_equal(got, want), ("oracle", np.nonzero((got != want).any(1))[0][:5], got[:4], want[:4])
    by_dump = _argmax_of_dump(dump, mu)
    assert np.array_equal(got, by_dump), ("dump", np.nonzero((got != by_dump).any(1))[0][:5])
    assert np.array_equal(got, got2)
    assert np.array_equal(got, np.asarray(base["res"], np.int64)), "the two libraries disagree"
    # what this call's kernel runs: both tiers in the 7- and 10-row production instantiations only
    generic = max(len(lad[0]), len(lad[2])) * scoring[0] >= 30
    if t2.kernel_rule(R, generic) == "tier2" and model["tier2"] < model["tier1"]:
        assert cols < base["trunk_cols"], (cols, base["trunk_cols"], model)
    else:
        assert cols == base["trunk_cols"], (cols, base["trunk_cols"], model)
