"""GPU: fixed-seed slices of the randomised parity campaigns (tools/fuzz_*.py) so that every run of the suite
re-draws them: the long campaigns logged under profiles/ are the same code with more rounds.

  fuzz_parity     pruned production kernel path vs the reference's own compiled ssw.c (oracle/_ref; without it the C
                  restatement tests/test_oracle_sw.py pins to the reference) read by read: (tag, h, score); plus the
                  per-template dump field by field on adversarial units
  fuzz_selfcheck  production launch vs arg-max over the unpruned per-template dump (GPU only, many reads)
  fuzz_hist       adversarial grid inputs vs the numpy oracle: status, enumeration, four terms per pair, CI, PP
  fuzz_grid       SW -> histograms -> grid on random synthetic batches vs the numpy oracle
  fuzz_cigar      the CIGAR kernel vs the reference's own compiled banded_sw (oracle/_ref; without it tests/cigar_model.py,
                  which tests/test_cigar_model.py pins to the reference) pair by pair at six scorings: every operation
  fuzz_long       the long-read kernel vs the C restatement (tests/test_oracle_sw.py pins it to the reference on long pairs
                  at these scorings) at ten scorings, the three row classes mixed in every call: (tag, h, score) per read
                  and every template's dump row
"""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_fuzz_parity_slice():
    import fuzz_parity
    res = fuzz_parity.campaign(rounds=80, seed=20270301)
    assert res["reads"] > 100000 and res["template_pairs"] > 200000
    assert res["mismatches"] == 0 and res["pair_mismatches"] == 0, res


def test_fuzz_selfcheck_slice():
    import fuzz_selfcheck
    res = fuzz_selfcheck.campaign(rounds=12, seed=20270302)
    assert res["reads"] > 100000
    assert res["mismatches"] == 0, res


def test_fuzz_hist_slice():
    import fuzz_hist
    res = fuzz_hist.campaign(cases_n=250, seed=20270303)
    assert res["pairs_compared"] > 100000 and res["cases_the_reference_raises_on"] > 0
    assert res["mismatches"] == 0 and res["max_abs_diff_ml_terms"] <= 1e-6, res


def test_fuzz_grid_slice():
    import fuzz_grid
    res = fuzz_grid.campaign(rounds=12, seed=20270304, max_pairs=6000)
    assert res["units_checked"] > 50
    assert res["mismatches"] == 0 and res["max_abs_diff_lik_or_pp"] <= 1e-6, res


def test_fuzz_inflate_slice():
    import fuzz_inflate
    res = fuzz_inflate.campaign(rounds=6, seed=20270305)
    assert res["streams"] == 1800 and res["intact"] == 1440 and res["damaged_refused"] > 100
    assert res["mismatches"] == 0, res


def test_fuzz_cigar_slice():
    import fuzz_cigar
    scorings = ((1, 5, 7, 2), (2, 2, 3, 1), (1, 1, 2, 1), (1, 4, 6, 1), (3, 5, 7, 2), (1, 0, 1, 1))
    res = fuzz_cigar.campaign(n=1500, seed=20270306, scorings=scorings)
    assert res["mismatches"] == 0, res
    assert res["compared"] >= 0.9 * res["pairs"] == 1350, res
    assert 2 * res["with_gap"] > res["compared"], res
    assert res["wide_tier"] >= 1, res


def test_fuzz_long_slice():
    """Ten rounds meet each of the ten scorings once.  The oracle side is the cost: 33 s of the 34 on 16 threads (64 s on
    8); the GPU's share is under a second."""
    import fuzz_long
    res = fuzz_long.campaign(rounds=10, seed=20270307)
    print(res)
    assert res["reads"] > 300 and res["template_pairs"] > 50000, res
    assert sorted(res["scorings"]) == sorted("/".join(map(str, s)) for s in fuzz_long.SCORINGS), res
    assert min(res["class8"], res["class16"], res["class32"]) >= 50, res
    assert res["mismatches"] == 0 and res["pair_mismatches"] == 0, res
