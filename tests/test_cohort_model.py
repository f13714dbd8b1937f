"""The cohort model (tests/cohort_model.py) on the CPU: the orientation values of DESIGN 4 ("Cohort frequencies"), the
properties the model has by its definition, every refusal with the precedence, and that every item the GPU tests use
(tests/cohort_cases.py) has the status it is meant to have and a call to compare -- an exact tie where one is intended, and
then more than 1e-5 to the best pair outside the tied group.  The comparison of the GPU tests (tests/cohort_compare.py) is
tested here, too: the spread of the reference its tolerances are derived from is measured again, it accepts the float64
model on every case, and it rejects five deliberately wrong variants of the model, two of which the absolute 1e-6 alone let
pass."""
import math

import numpy as np
import pytest

from . import cohort_cases as cases
from . import cohort_compare as cc
from . import cohort_model as cm


@pytest.fixture(scope="module")
def golden():
    return cases.golden_cohort()


@pytest.fixture(scope="module")
def fit(golden):
    return cm.evaluate(*golden)


@pytest.fixture(scope="module")
def evaluations(golden):
    """[(name, item, parameters, ties, the float64 model, the long-double model)] of every item the GPU tests compare."""
    return [(name, item, params, ties) + cc.reference(*item, **params) for name, item, params, ties in cases.compared(golden)]


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


def test_every_gpu_case_has_a_call_to_compare(golden, evaluations):
    for name, _, params, ties, want, ref in evaluations:
        assert want["status"] == ref["status"] == (cm.OK if name not in ("batch_of_nine", "big_call") else want["status"]), name
        for r in (want, ref):
            assert all(g is None or g > 1e-5 for g in r["beyond" if ties else "gap"]), (name, params)
        assert want["index"] == ref["index"], (name, params)
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


def _same_bits(x, y):
    """Of two numbers of one type (a long double's bytes have padding: they are not compared)."""
    return x.dtype == y.dtype and x == y and np.signbit(x) == np.signbit(y)


def test_the_new_cases_are_what_they_are_meant_to_be(evaluations):
    by_name = {}
    for name, item, _, _, want, ref in evaluations:
        by_name.setdefault(name, []).append((item, want, ref))
    # the lone 0 of every long list at its edge, the two ploidy-1 lists beyond the threshold
    (peaks, want, _), (hap, hap_want, _) = by_name["long_list_edges"]
    assert [len(s[0]) for s in peaks[0]] == [1025] * 7 + [2049] * 2 and want["index"] == [0, 63, 64, 255, 256, 1023, 1024, 2047, 2048]
    assert hap[1] == 1 and [len(s[0]) for s in hap[0]] == [1025, 1500] and hap[0][0][0].tolist() == list(range(1025))
    assert len(set(hap[0][1][0].tolist())) < 1500 and hap_want["status"] == cm.OK
    # the ties: exact in both evaluations, the call the one the rule gives, the rest of the list beyond 1e-5
    for name in cases.TIES:
        for k, (item, want, ref) in enumerate(by_name[name]):
            assert want["index"] == ref["index"] == cases.TIE_CALLS[name][k], name
            for r in (want, ref):
                for s, q in enumerate(r["q"]):
                    tied = np.flatnonzero(q == q[r["index"][s]])
                    assert len(tied) == 2 and _same_bits(q[tied[0]], q[tied[1]]) and q[tied[0]] == q.max(), (name, s)
                    assert r["gap"][s] == 0.0 and r["beyond"][s] > 1e-5, (name, s)
                if name != "duplicates":                            # f(5) and f(7), bit for bit
                    f = dict(zip(r["alleles"].tolist(), r["freq"]))
                    assert _same_bits(f[5], f[7]), name
                    assert all(c[0] == 5 for c in r["call"]), name
    n, i, j = cases.DUPLICATES[5]
    dup = by_name["duplicates"][0][0][0][5]
    assert len(dup[0]) == n > cases.LONG_LIST and j == i + 2 * 64 and all((dup[0][k], dup[1][k], dup[2][k]) == (6, 8, 0.0) for k in (i, j))
    # the big call: more items than a launch has workgroups, more chunks than four times that, a refused and an empty class
    classes = cases.big_call()
    A = [len(want["alleles"]) for _, want, _ in by_name["big_call"]]
    assert [want["status"] for _, want, _ in by_name["big_call"]] == [cm.OK, cm.OK, cm.OK, cm.BAD_ITEM, cm.EMPTY, cm.OK] and max(A) >= 4
    assert len(classes) == cases.BIG_N > 65536 and int(np.take(A, classes).sum()) > 4 * 65536 and set(classes.tolist()) == set(range(6))
    assert not set(cm.evaluate(*cases.OTHER_ALLELES)["alleles"].tolist()) & {5, 9, 12}
    for name in ("long_a_above_b_in_wavefront_3", "long_allele_1025", "long_heterozygous_at_ploidy_1"):
        (samples, ploidy), _ = cases.REFUSED[name]()
        assert len(samples[-1][0]) == 1100 > cases.LONG_LIST and ploidy[-1] == (1 if "ploidy_1" in name else 2)


def test_the_spread_of_the_reference_stays_within_the_constants(evaluations):
    S = {}
    for name, _, params, _, want, ref in evaluations:
        if want["status"] == cm.OK:
            for out, d in cc.spread(want, ref).items():
                S[out] = max(S.get(out, 0.0), d)
    print("\nS_out:", {k: float("%.3g" % v) for k, v in sorted(S.items())})
    assert sorted(S) == sorted(cc.S_OUT) == sorted(cc.RELATIVE + cc.ABSOLUTE)
    for out in S:
        assert S[out] <= cc.S_OUT[out], (out, S[out])
        assert cc.TOLERANCE[out] == cc.FACTOR * cc.S_OUT[out] and cc.FACTOR == 64
    assert cc.REL_CAP == 1e-10 and all(cc.TOLERANCE[out] <= cc.REL_CAP for out in cc.RELATIVE)
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63 and cc.FLOOR == 2.0 ** -1000 and cc.TOL == 1e-6


def test_the_comparison_accepts_the_model(evaluations):
    for name, _, params, ties, want, ref in evaluations:
        cc.same(cc.from_model(want), want, ref, (name, params), ties=ties)


def _mutant(monkeypatch, hook, wrong, item, params):
    """The float64 model of an item with the function `wrong` in place of cohort_model's `hook`, as same() takes it."""
    with monkeypatch.context() as m:
        m.setattr(cm, hook, wrong)
        return cc.from_model(cm.evaluate(*item, **params))


def _rejected(got, want, ref, **how):
    try:
        cc.same(got, want, ref, **how)
    except AssertionError:
        return True
    return False


def test_the_comparison_rejects_five_wrong_models(monkeypatch, golden, evaluations):
    at = {(name, tuple(sorted(params.items()))): (item, params, want, ref) for name, item, params, _, want, ref in evaluations}
    # (a) the factor 2 dropped for one pair: the heterozygous pair with the smallest r of the golden cohort's largest list
    # (the smallest r of all is a homozygous pair's, which has no such factor)
    item, params, want, ref = at["golden", (("iters", 64),)]
    s = int(np.argmax([len(x[0]) for x in item[0]]))
    het = np.flatnonzero(item[0][s][0] != item[0][s][1])
    k = int(het[np.argmin(want["r"][s][het])])
    assert len(item[0][s][0]) == 5460 and sum(len(x[0]) == 5460 for x in item[0]) == 1 and cc.FLOOR < want["r"][s][k] < 1e-30
    def het_but_one(ia, ib, real=cm._het):
        h = real(ia, ib)
        if len(ia) == 5460:
            h[k] = 1.0
        return h
    got = _mutant(monkeypatch, "_het", het_but_one, item, params)
    assert _rejected(got, want, ref) and not _rejected(got, want, ref, relative=False)
    # (b) the weights rounded through single precision
    single = lambda lw, m, real=cm._weights: real(lw, m).astype(np.float32).astype(lw.dtype)
    got = _mutant(monkeypatch, "_weights", single, item, params)
    assert _rejected(got, want, ref) and not _rejected(got, want, ref, relative=False)
    # (c) the last entry of the last incidence chunk of chunk_plus_1 left out of n: allele 5, the last sample's a
    item, params, want, ref = at["chunk_plus_1", (("iters", 3),)]
    def without_the_tail(lists, ploidy, w, m, pos, f, dtype=np.float64, real=cm._e_step):
        q, Z, logZ, n = real(lists, ploidy, w, m, pos, f, dtype)
        entries = [x for s, qs, Zs in zip(lists, q, Z) for a, b, r in zip(s[0], s[1], qs / Zs) for c, x in ((a, r), (b, r)) if c == 5]
        assert len(entries) == cases.CHUNK + 1 and abs(cm._seq_sum(entries) - n[0]) < 1e-9
        n[0] = cm._seq_sum(entries[:-1])
        return q, Z, logZ, n
    assert want["alleles"][0] == 5 and _rejected(_mutant(monkeypatch, "_e_step", without_the_tail, item, params), want, ref)
    # (d) the first of the largest q, whatever its a;  (e) the last of a full tie
    first_q = lambda qs, a: int(np.argmax(qs))
    last_of_a_tie = lambda qs, a: max(range(len(qs)), key=lambda k: (qs[k], -a[k], k))
    for name, wrong, passes in (("symmetric", first_q, "duplicates"), ("duplicates", last_of_a_tie, "symmetric")):
        item, params, want, ref = at[name, (("iters", 16),)]
        assert _rejected(_mutant(monkeypatch, "_pick", wrong, item, params), want, ref, ties=True), name
        item, params, want, ref = at[passes, (("iters", 16),)]     # (each is seen by its own mechanism alone)
        assert not _rejected(_mutant(monkeypatch, "_pick", wrong, item, params), want, ref, ties=True), name
