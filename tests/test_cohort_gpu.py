"""GPU: tredcohort_evaluate (include/tredcohort.h, csrc/cohort.hip) against the model (tests/cohort_model.py): statuses, A,
the support and every sample's call exactly; f, count, r, post, logZ and both trace columns within the project's tolerance,
1e-6 absolute, and -- f, count, r and post relatively -- within 64 times the spread of the reference against the model in
long double (tests/cohort_compare.py has the comparison and says where the tolerances come from).  Over the golden HD
cohort, crafted lists at the kernels' edges (the wavefront's and the workgroup's strides over a list, the chunk of the
incidence list, the size of the support, the allele cap), exact ties, refusals from short and long lists, parameters up to
the iteration cap, batches, repeats, one call beyond the launch caps, and what a call leaves behind for the next.  The call
is compared wherever the model's gap between the best and the second log q exceeds 1e-5 -- in the tie cases, between the
tied pairs and the best other -- and every case here has to qualify (tests/test_cohort_model.py checks on the CPU that they
do)."""
import json

import numpy as np
import pytest

from tredparse_amd import _lib

from . import cohort_cases as cases
from . import cohort_compare as cc
from . import cohort_model as cm

pytestmark = pytest.mark.gpu
CHUNK, CAP = _lib.COHORT_CHUNK, _lib.COHORT_MAX_ALLELE
same = cc.same


def pack(items, rooms=None):
    """The arrays of one Context.cohort call for [(samples, ploidy)], samples a list of (a, b, lw) or None.  rooms: per item
    its room in the three allele arrays (default: as many as the header says are always enough)."""
    item_off = np.zeros(len(items) + 1, np.int64)
    item_off[1:] = np.cumsum([len(s) for s, _ in items])
    flat = [x for s, _ in items for x in s]
    off = np.zeros(len(flat) + 1, np.int64)
    off[1:] = np.cumsum([0 if x is None else len(x[0]) for x in flat])
    cat = lambda i, dt: np.ascontiguousarray(np.concatenate([np.asarray(x[i], dt) for x in flat if x is not None] + [np.zeros(0, dt)]))
    ploidy = np.ascontiguousarray(np.concatenate([np.broadcast_to(np.asarray(p, np.int32), (len(s),)) for s, p in items] + [np.zeros(0, np.int32)]), np.int32)
    allele_off = np.zeros(len(items) + 1, np.int64)
    allele_off[1:] = np.cumsum(np.minimum(2 * np.diff(off[item_off]), CAP + 1) if rooms is None else rooms)
    return item_off, (off, cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)), ploidy, allele_off


def outputs(item_off, samples, allele_off, iters):
    """Output arrays that hold no zero: whatever the call leaves alone shows."""
    n, ns, room = len(item_off) - 1, len(samples[0]) - 1, int(allele_off[-1])
    return (np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(room, -1, np.int32), np.full(room, np.nan), np.full(room, np.nan),
            np.full((n, iters, 2), np.nan), np.full((ns, 3), -1, np.int32), np.full((ns, 2), np.nan), np.full(int(samples[0][-1]), np.nan))


def run(ctx, items, iters=cm.ITERS, alpha=cm.ALPHA, rooms=None):
    """One Context.cohort call: per item a dict of its outputs (room: its whole room in the three allele arrays)."""
    item_off, samples, ploidy, allele_off = pack(items, rooms)
    out = outputs(item_off, samples, allele_off, iters)
    ctx.cohort(len(items), item_off, samples, ploidy, allele_off, *out, iters=iters, alpha=alpha)
    status, n_alleles, alleles, freq, count, trace, call, values, r = out
    per = []
    for i in range(len(items)):
        lo, hi, j0, j1 = int(item_off[i]), int(item_off[i + 1]), int(allele_off[i]), int(allele_off[i + 1])
        per.append(dict(status=int(status[i]), A=int(n_alleles[i]), alleles=alleles[j0:j1], freq=freq[j0:j1], count=count[j0:j1],
                        trace=trace[i], call=call[lo:hi], values=values[lo:hi],
                        r=[r[samples[0][s]:samples[0][s + 1]] for s in range(lo, hi)]))
    return per


def check(ctx, items, ties=False, **params):
    got = run(ctx, items, **params)
    for k, (g, (samples, ploidy)) in enumerate(zip(got, items)):
        same(g, *cc.reference(samples, ploidy, **params), what="item {}".format(k), ties=ties)
    return got


@pytest.fixture(scope="module", autouse=True)
def observed():
    yield
    print("\nlargest differences from the model:", json.dumps({k: float("%.2g" % v) for k, v in cc.OBSERVED.items()}, sort_keys=True))


@pytest.fixture(scope="module")
def golden():
    return cases.golden_cohort()


@pytest.mark.parametrize("iters", [1, 2, 64])
def test_the_golden_cohort(ctx, golden, iters):
    ctx.reset_timing()
    got = check(ctx, [golden], iters=iters)[0]
    n, ms = ctx.get_timing(_lib.KERNEL_COHORT)
    assert n == 1 and ms > 0                                        # get_timing counts one call
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_COHORT) == (0, 0.0)
    if iters == 64:
        assert got["A"] == 300 and abs(got["trace"][63, 0] - -55.119594) < 1e-6
        calls = dict(zip(cases.GOLDEN_NAMES, (tuple(c[1:].tolist()) for c in got["call"])))
        assert calls["hd_no_full"] == (78, 79) and calls["hd_no_pe_model"] == (20, 80) and calls["hd_typical"] == (15, 41)


@pytest.mark.parametrize("alpha", [1e-6, 100.0])
def test_the_golden_cohort_at_other_alphas(ctx, golden, alpha):
    check(ctx, [golden], alpha=alpha)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_crafted_cases(ctx, name):
    items, params = cases.CASES[name]()
    check(ctx, items, **params)


@pytest.mark.parametrize("name", sorted(cases.TIES))
def test_exact_ties(ctx, name):
    items, params = cases.TIES[name]()
    for k, (g, (samples, ploidy)) in enumerate(zip(run(ctx, items, **params), items)):
        if name != "duplicates":                                    # what the tie rests on first: f(5) and f(7), bit for bit
            f = dict(zip(g["alleles"][:g["A"]].tolist(), g["freq"][:g["A"]]))
            assert g["status"] == cm.OK and f[5].tobytes() == f[7].tobytes(), (name, f[5], f[7])
        same(g, *cc.reference(samples, ploidy, **params), what=name, ties=True)
        assert g["call"][:, 0].tolist() == cases.TIE_CALLS[name][k], name


@pytest.mark.parametrize("name", sorted(cases.REFUSED))
def test_refusals(ctx, name):
    item, status = cases.REFUSED[name]()
    good = cases.small_item(3)
    got = check(ctx, [good, item, good], iters=5)
    assert got[1]["status"] == status
    alone = run(ctx, [good], iters=5)[0]
    for key in ("freq", "count", "trace", "call", "values"):       # the neighbours of a refused item are unaffected
        assert got[0][key].tobytes() == got[2][key].tobytes() == alone[key].tobytes(), (name, key)


def _bits(x):
    return [x["status"], x["A"]] + [x[k].tobytes() for k in ("alleles", "freq", "count", "trace", "call", "values")] + [r.tobytes() for r in x["r"]]


def test_a_batch_equals_its_items_one_by_one_in_two_orders(ctx, golden):
    items = cases.batch_of_nine(golden)
    assert len(items) == 9
    alone = [_bits(run(ctx, [it], iters=7)[0]) for it in items]
    assert [a[0] for a in alone][3:5] == [cm.BAD_ITEM, cm.EMPTY]
    for order in (list(range(9)), [8, 3, 0, 7, 4, 1, 6, 2, 5]):
        got = check(ctx, [items[k] for k in order], iters=7)
        for k, g in zip(order, got):
            assert _bits(g) == alone[k], (order, k)


def test_rooms_of_exactly_A_give_the_same_bits(ctx, golden):
    items = cases.batch_of_nine(golden)
    rooms = [len(cm.evaluate(*it, iters=1)["alleles"]) for it in items]
    assert rooms[3:5] == [0, 0] and min(rooms[:3] + rooms[5:]) > 0
    # The empty item gets no room.  The refused one cannot: the header asks for room for the distinct alleles of an item's
    # lists in 0 .. MAX_ALLELE whatever becomes of the item -- the host sizes before the device has validated anything --,
    # and a call with less is refused as a whole (-2).  Its lists name 5, 6 and 7.
    with pytest.raises(_lib.TredGpuError, match=r"\(-2\).*item 3 has 3 alleles and room for 0"):
        run(ctx, items, iters=7, rooms=rooms)
    rooms[3] = 3
    generous, tight = run(ctx, items, iters=7), run(ctx, items, iters=7, rooms=rooms)
    for k, (g, t) in enumerate(zip(generous, tight)):
        assert len(t["alleles"]) == rooms[k] and (g["A"] == rooms[k] or k == 3) and not g["alleles"][g["A"]:].any()
        for key in ("alleles", "freq", "count"):
            g[key] = g[key][:rooms[k]]
        assert _bits(g) == _bits(t), k


def test_the_iteration_cap(ctx):
    item = cases.small_item(2)
    got = check(ctx, [item], iters=_lib.COHORT_MAX_ITERS)[0]
    assert _lib.COHORT_MAX_ITERS == cm.MAX_ITERS == 4096 and got["trace"].shape == (4096, 2) and np.isfinite(got["trace"]).all()


@pytest.fixture(scope="module")
def other_alleles_on_a_fresh_context():
    fresh = _lib.Context(0)
    try:
        return _bits(run(fresh, [cases.OTHER_ALLELES], iters=5)[0])
    finally:
        fresh.close()


def _nothing_is_left(ctx, fresh_bits):
    """A small item over alleles of its own, on the context that has just run something large, against the same item on a
    context that never ran anything: the device's scratch (f, part, sflag, w) is reused from call to call."""
    got = check(ctx, [cases.OTHER_ALLELES], iters=5)[0]
    assert _bits(got) == fresh_bits


def test_a_call_beyond_the_launch_caps(ctx, other_alleles_on_a_fresh_context):
    classes, iters = cases.big_call(), cases.BIG_ITERS
    alone = [check(ctx, [it], iters=iters)[0] for it in cases.BIG_CLASSES]
    assert [a["status"] for a in alone] == [cm.OK, cm.OK, cm.OK, cm.BAD_ITEM, cm.EMPTY, cm.OK]
    # more items than a launch has workgroups (65 536), more chunks than four times that: every grid-stride loop strides
    assert len(classes) > 65536 and sum(alone[c]["A"] for c in classes) > 4 * 65536
    got = run(ctx, [cases.BIG_CLASSES[c] for c in classes], iters=iters)
    bits = [_bits(a) for a in alone]
    wrong = [i for i, (g, c) in enumerate(zip(got, classes)) if _bits(g) != bits[c]]
    assert not wrong, (len(wrong), wrong[:10], [int(classes[i]) for i in wrong[:10]])
    _nothing_is_left(ctx, other_alleles_on_a_fresh_context)


def test_nothing_of_the_largest_support_is_left_for_the_next_call(ctx, other_alleles_on_a_fresh_context):
    items, params = cases.CASES["support_1025"]()
    assert run(ctx, items, **params)[0]["A"] == CAP + 1
    _nothing_is_left(ctx, other_alleles_on_a_fresh_context)


def test_the_same_call_twice_gives_the_same_bits(ctx, golden):
    items = [golden, cases.small_item(5), cases.CASES["chunk_plus_1"]()[0][0]]
    first, second = (run(ctx, items, iters=9) for _ in range(2))
    assert [_bits(x) for x in first] == [_bits(x) for x in second]


def test_bad_arguments_leave_the_outputs_alone(ctx):
    item_off, samples, ploidy, allele_off = pack([cases.small_item(3)])
    def refused(args=None, **params):
        out = outputs(item_off, samples, allele_off, 4)
        before = [x.copy() for x in out]
        a = dict(item_off=item_off, samples=samples, ploidy=ploidy, allele_off=allele_off)
        a.update(args or {})
        with pytest.raises(_lib.TredGpuError, match=r"\(-2\)"):
            ctx.cohort(1, a["item_off"], a["samples"], a["ploidy"], a["allele_off"], *out, **params)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(out, before))
    for params in (dict(iters=0), dict(iters=_lib.COHORT_MAX_ITERS + 1), dict(iters=4, alpha=0.0), dict(iters=4, alpha=-1.0),
                   dict(iters=4, alpha=float("nan")), dict(iters=4, alpha=float("inf"))):
        refused(**params)
    refused(dict(item_off=None), iters=4)
    refused(dict(ploidy=None), iters=4)
    refused(dict(allele_off=None), iters=4)
    refused(dict(samples=(samples[0], None, samples[2], samples[3])), iters=4)
    refused(dict(item_off=np.array([1, 3], np.int64)), iters=4)                            # does not begin at 0
    refused(dict(samples=(np.array([0, 2, 1, 3], np.int64),) + samples[1:]), iters=4)      # descends
    refused(dict(allele_off=np.array([0, 1], np.int64)), iters=4)                          # less room than alleles
    out = outputs(item_off, samples, allele_off, 4)
    with pytest.raises(_lib.TredGpuError, match=r"\(-2\)"):
        ctx.cohort(1, item_off, samples, ploidy, allele_off, None, *out[1:], iters=4)
    ctx.cohort(0, None, (None,) * 4, None, None, *(None,) * 9)      # no item: nothing to do
