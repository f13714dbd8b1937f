"""GPU: a slice of tools/fuzz_second.py -- 1 500 random (reference, read) pairs at six scorings, a few of them long,
through the second-best kernel; all four values against the compiled reference (oracle/_ref) where it is built, otherwise
against tests/second_model.c, which tests/test_second_model.py pins to the reference."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fuzz_second_slice(ctx):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_second
    assert len(fuzz_second.DEFAULT_SCORINGS) == 6
    res = fuzz_second.campaign(n=1500, seed=20270412)
    print(res)
    assert res["mismatches"] == 0 and res["model_differs"] == 0, res
    assert res["compared"] >= 0.95 * res["pairs"] == 1425, res
    assert 2 * res["with_second"] > res["compared"] and res["word_pass"] >= 100 and res["long_pairs"] >= 10, res
