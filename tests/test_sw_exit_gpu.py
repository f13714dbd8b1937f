"""sw_cont_kernel's bounded-gain exit (csrc/sw_ladder.hip: steady_exit, SW_EXIT_BOUND) through tredgpu_sw_classify.

Per case (tests/sw_exit_gpu_cases.py: 100, 150 and 250 bp, an N ladder, a period-5 ladder -- the generic column loop --, a
ladder with a 39-base branch -- the GENERIC kernel --, --useclippedreads, a scoring outside the 6-mer premise), quads of four
reads of four different kinds:

* every read's tag, h and score from the production launches equal the arg-max of the kernel's own unpruned per-template
  dump, and the oracle's classification;
* the trunk-column counter is strictly lower than that of the library built with the test compiled out
  (libtredgpu_noexit.so, run once in a child process through TREDGPU_LIB) where the CPU model (tests/sw_exit_model.py) says
  some wave leaves earlier, and equal where it says none does -- which includes the 250 bp and the long-branch case, whose
  instantiations do not hold the test (sw_exit_model.kernel_rule); the results of the two libraries are identical.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from tredparse_amd import _lib

from . import sw_exit_gpu_cases as cs
from . import sw_exit_model as xm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOEXIT = os.path.join(ROOT, "tredparse_amd", "libtredgpu_noexit.so")
_BASE = {}


def _baseline():
    """every case through the library without the test: one child process for all of them"""
    if not _BASE:
        assert os.path.exists(NOEXIT), "libtredgpu_noexit.so is missing: build() makes it"
        env = dict(os.environ, TREDGPU_LIB=NOEXIT)
        out = subprocess.run([sys.executable, "-m", "tests.sw_exit_gpu_cases"], cwd=ROOT, env=env, capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [l for l in out.stdout.splitlines() if l.startswith("SW_EXIT_CASES ")][-1]
        _BASE.update(json.loads(line[len("SW_EXIT_CASES "):]))
        assert _BASE["lib"] == NOEXIT
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
    model = {"old": 0, "tier1": 0}
    for q in quads:
        res = xm.ladder_passes(q, ladders[0], scoring, R, ("old", "tier1"), clip=bool(clip))
        for r in model:
            model[r] += res[r]["cols"]
    got, cols, _ = cs.run_case(ctx, name)
    got2, _, dump = cs.run_case(ctx, name, dump=True)
    base = _baseline()[name]
    print(name, "reads", len(got), "trunk columns: head", cols, "without the test", base["trunk_cols"], "model", model)
    reads = [r for q in quads for r in q]
    want = po.classify(reads, np.repeat(np.arange(len(quads)), 4).astype(np.int32), po.LocusSet(ladders), clip=bool(clip),
                       scoring=scoring, threads=4).astype(np.int64)
    assert np.array_equal(got, want), ("oracle", np.nonzero((got != want).any(1))[0][:5], got[:4], want[:4])
    by_dump = _argmax_of_dump(dump, mu)
    assert np.array_equal(got, by_dump), ("dump", np.nonzero((got != by_dump).any(1))[0][:5])
    assert np.array_equal(got, got2)
    assert np.array_equal(got, np.asarray(base["res"], np.int64)), "the two libraries disagree"
    assert name.startswith("inside") or len(set(int(t) for t in want[:, 0])) >= 4     # the quads hold what they claim
    # what this call's kernel runs: the test is in the 7- and 10-row production instantiations only (xm.kernel_rule)
    generic = max(len(lad[0]), len(lad[2])) * scoring[0] >= 30
    rule = xm.kernel_rule(R, generic)
    if model[rule] < model["old"]:
        assert cols < base["trunk_cols"], (cols, base["trunk_cols"], model)
    else:
        assert cols == base["trunk_cols"], (cols, base["trunk_cols"], model)
