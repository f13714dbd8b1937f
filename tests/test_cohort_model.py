"""The cohort model (tests/cohort_model.py) on the CPU: the orientation values of DESIGN 4 ("Cohort frequencies"), the
properties the model has by its definition, every refusal with the precedence, and that every item the GPU tests use
(tests/cohort_cases.py) has the status it is meant to have and a call to compare."""
import math

import numpy as np
import pytest

from . import cohort_cases as cases
from . import cohort_model as cm


@pytest.fixture(scope="module")
def golden():
    return cases.golden_cohort()


@pytest.fixture(scope="module")
def fit(golden):
    return cm.evaluate(*golden)


def test_the_orientation_values(golden, fit):
    names = cases.GOLDEN_NAMES
    assert len(names) == 13 and fit["status"] == cm.OK and len(fit["alleles"]) == 300 and fit["C"] == 25
    for t, loglik, delta in ((1, -114.147313, 1.506e-1), (2, -57.445099, 4.071e-2), (8, -55.429842, 2.077e-3), (64, -55.119594, 1.382e-4)):
        assert abs(fit["trace"][t - 1, 0] - loglik) < 5e-7 and abs(fit["trace"][t - 1, 1] / delta - 1) < 5e-4, t
    f = dict(zip(fit["alleles"].tolist(), fit["freq"].tolist()))
    for allele, want in ((15, 0.15397), (41, 0.15047), (20, 0.07705), (30, 0.07705), (33, 0.07705), (47, 0.03949)):
        assert abs(f[allele] - want) < 5e-6, allele
    samples = dict(zip(names, golden[0]))
    single = {n: (int(s[0][np.argmax(s[2])]), int(s[1][np.argmax(s[2])])) for n, s in samples.items()}
    call, post, gap = (dict(zip(names, fit[k])) for k in ("call", "post", "gap"))
    moved = {n for n in names if call[n] != single[n]}
    assert moved == {"hd_no_full", "hd_no_pe_model"}
    assert (single["hd_no_full"], call["hd_no_full"]) == ((76, 76), (78, 79))                   # hd_no_full moves from 76/76
    assert (single["hd_no_pe_model"], call["hd_no_pe_model"]) == ((20, 91), (20, 80))
    for n, want in (("hd_no_full", 0.0503), ("hd_no_pe_model", 0.1621), ("hd_typical", 0.9504), ("hd_fullsearch", 0.9586),
                    ("hd_expanded_rept_pe", 0.1741), ("hd_100x", 0.2118)):
        assert abs(post[n] - want) < 5e-5, n
    assert abs(min(gap.values()) - 4.7e-2) < 5e-4 and min(gap, key=gap.get) == "hd_no_pe_model"
    assert not fit["converged"] and fit["delta"] == fit["trace"][-1, 1]
    assert cm.evaluate(*golden, tol=1e-3)["converged"]              # a report against tol, not a control: the same 64 steps


def test_frequencies_sum_to_one_and_the_objective_does_not_decrease(fit, golden):
    assert abs(fit["freq"].sum() - 1) < 1e-12 and abs(fit["count"].sum() - fit["C"]) < 1e-9
    assert len(fit["objective"]) == 64 and np.diff(fit["objective"]).min() > -1e-9
    for alpha in (1e-6, 100.0):
        r = cm.evaluate(*golden, iters=12, alpha=alpha)
        assert abs(r["freq"].sum() - 1) < 1e-12 and np.diff(r["objective"]).min() > -1e-9


def test_identical_homozygous_samples():
    for N, alpha in ((1, 1.0), (7, 0.25), (40, 3.0)):
        r = cm.evaluate([cases.one(9, 9)] * N, 2, iters=5, alpha=alpha)
        assert r["alleles"].tolist() == [9] and r["freq"][0] == (2 * N + alpha / 1) / (2 * N + alpha) == 1.0
    # beside one sample of another allele: A = 2, the formula with its pseudo-count
    N, alpha = 6, 0.5
    r = cm.evaluate([cases.one(9, 9)] * N + [cases.one(4, 4)], 2, iters=3, alpha=alpha)
    assert r["freq"].tolist() == [(2 + alpha / 2) / (2 * N + 2 + alpha), (2 * N + alpha / 2) / (2 * N + 2 + alpha)]


def test_a_ploidy_1_sample_adds_one_chromosome():
    both = cm.evaluate([cases.one(9, 9), cases.one(4, 4)], [2, 1], iters=4)
    assert both["C"] == 3 and both["count"].tolist() == [1.0, 2.0]
    assert both["freq"].tolist() == [(1 + 0.5) / 4, (2 + 0.5) / 4]
    assert cm.evaluate([cases.one(9, 9), cases.one(4, 4)], 2, iters=4)["C"] == 4


def test_sharp_lists_reproduce_counting():
    samples = [cases.lst((5, 9, 0.0), (5, 5, -60.0), (9, 9, -60.0))] * 3 + [cases.lst((5, 5, 0.0), (5, 9, -60.0))] * 2 + [cases.one(9, 9)]
    r = cm.evaluate(samples, 2, alpha=1e-9)
    assert r["alleles"].tolist() == [5, 9] and np.abs(r["freq"] - np.array([7.0, 5.0]) / 12).max() < 1e-8


def test_a_flat_symmetric_list_splits_its_count_evenly():
    r = cm.evaluate([cases.lst((5, 5, 0.0), (9, 9, 0.0))], 2)
    assert r["freq"].tolist() == [0.5, 0.5] and r["count"].tolist() == [1.0, 1.0] and r["r"][0].tolist() == [0.5, 0.5]
    r = cm.evaluate([cases.lst((5, 5, 0.0), (9, 9, 0.0)), cases.one(5, 9)], 2, iters=10)
    assert r["count"].tolist() == [2.0, 2.0] and r["freq"].tolist() == [0.5, 0.5]


def test_the_tie_rule():
    # the largest q, then the smallest a, then the first in the list
    r = cm.evaluate([cases.lst((9, 9, 0.0), (5, 5, 0.0))], 2)
    assert (r["index"][0], r["call"][0], r["gap"][0]) == (1, (5, 5), 0.0)
    r = cm.evaluate([cases.lst((5, 5, -1.0), (5, 5, 0.0), (5, 5, 0.0))], 2)
    assert (r["index"][0], r["call"][0]) == (1, (5, 5))


def test_every_refusal_and_the_precedence():
    for name, make in cases.REFUSED.items():
        (samples, ploidy), status = make()
        r = cm.evaluate(samples, ploidy, iters=3)
        assert r["status"] == status and len(r["alleles"]) == 0 and not r["trace"].any() and r["trace"].shape == (3, 2), name
        assert r["call"] == [None] * len(samples), name
    with pytest.raises(ValueError):
        cm.evaluate([cases.one(5, 5)], 2, iters=0)
    with pytest.raises(ValueError):
        cm.evaluate([cases.one(5, 5)], 2, iters=cm.MAX_ITERS + 1)
    with pytest.raises(ValueError):
        cm.evaluate([cases.one(5, 5)], 2, alpha=0.0)


def test_an_empty_sample_in_the_middle_changes_nothing():
    samples, ploidy = cases.small_item(4)
    a = cm.evaluate(samples, ploidy, iters=6)
    b = cm.evaluate(samples[:2] + [None, cases.lst()] + samples[2:], [2, 2, 1, 2, 2, 2], iters=6)
    assert a["freq"].tobytes() == b["freq"].tobytes() and a["trace"].tobytes() == b["trace"].tobytes() and a["C"] == b["C"]
    assert b["call"][2] is None and b["call"][3] is None and [c for c in b["call"] if c is not None] == a["call"]


def test_every_gpu_case_has_a_call_to_compare(golden):
    for iters, alpha in ((1, 1.0), (2, 1.0), (64, 1e-6), (64, 100.0)):
        r = cm.evaluate(*golden, iters=iters, alpha=alpha)
        assert min(r["gap"]) > 1e-5, (iters, alpha)
    for name, make in cases.CASES.items():
        items, params = make()
        for samples, ploidy in items:
            r = cm.evaluate(samples, ploidy, **params)
            assert r["status"] == cm.OK and all(g is None or g > 1e-5 for g in r["gap"]), name
    for samples, ploidy in cases.batch_of_nine(golden):
        r = cm.evaluate(samples, ploidy, iters=7)
        assert all(g is None or g > 1e-5 for g in r["gap"])
    for n in (3, 5):
        assert min(cm.evaluate(*cases.small_item(n), iters=5)["gap"]) > 1e-5 and min(cm.evaluate(*cases.small_item(n), iters=9)["gap"]) > 1e-5
    r = cm.evaluate(*cases.CASES["chunk_plus_1"]()[0][0], iters=9)
    assert all(g > 1e-5 for g in r["gap"])
    # the edges the cases are there for
    assert [len(s[0]) for s in cases.CASES["list_sizes"]()[0][0][0]] == [1, 63, 64, 65, 255, 256, 257, 1000]
    for name, entries in (("chunk_minus_1", cases.CHUNK - 1), ("chunk", cases.CHUNK), ("chunk_plus_1", cases.CHUNK + 1),
                          ("two_chunks_plus_5", 2 * cases.CHUNK + 5)):
        samples, _ = cases.CASES[name]()[0][0]
        assert sum(int((s[0] == 5).sum() + (s[1] == 5).sum()) for s in samples) == entries
    assert [len(cm.evaluate(*it, iters=1)["alleles"]) for it in cases.CASES["support_1_64_65"]()[0]] == [1, 64, 65]
    assert len(cm.evaluate(*cases.CASES["support_1025"]()[0][0], iters=1)["alleles"]) == 1025
    r = cm.evaluate(*cases.CASES["lw_minus_800"]()[0][0])
    assert r["r"][0][0] == 0.0 and r["r"][1][1] == 0.0
    assert abs(cm.evaluate(*cases.CASES["max_lw_minus_50"]()[0][0])["logZ"][0] - -50) < 10
    assert math.isinf(cm.evaluate(*cases.CASES["one_pair_one_sample"]()[0][0])["gap"][0])
