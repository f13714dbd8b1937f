"""GPU: tredtrio_evaluate (include/tredtrio.h, csrc/trio.hip) against the model (tests/trio_model.py): status and call
exactly, J, Jmax, log S, denovo and paternal within the project's tolerance for log-likelihoods, 1e-6 absolute -- over the
golden HD grids, crafted lists at the kernels' edges (the pair chunk, the gamete tile, the child kernel's strides, the
allele cap), refusals, parameters, batches and repeats.  The call is compared wherever the model's gap between the best and
the second J exceeds 1e-5, and every case here has to qualify."""
import json
import math
import os

import numpy as np
import pytest

from tredparse_amd import _lib
from tredparse_amd import engine as eng
from tredparse_amd import trio

from . import trio_model as tm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-6
CHUNK, TILE, CAP = _lib.TRIO_PAIR_CHUNK, _lib.TRIO_GAMETE_TILE, _lib.TRIO_MAX_ALLELE
OBSERVED = {}            # the largest difference per output over the whole module, printed at its end


class Item(object):
    """One (trio, locus): the members' lists (a, b, lw) -- None: no list --, the child's ploidy, the parents' flags
    (default: 1 where there is a list)."""

    def __init__(self, child, father=None, mother=None, ploidy=2, f_inf=None, m_inf=None):
        self.child, self.father, self.mother, self.ploidy = child, father, mother, ploidy
        self.f_inf = int(father is not None) if f_inf is None else f_inf
        self.m_inf = int(mother is not None) if m_inf is None else m_inf

    def model(self, **params):
        # (a parent whose flag is 0 is not looked at, whatever its list holds)
        return tm.evaluate(self.child, self.father if self.f_inf else None, self.mother if self.m_inf else None,
                           ploidy=self.ploidy, **params)


def _pack(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([0 if l is None else len(l[0]) for l in lists])
    cat = lambda i, dt: np.ascontiguousarray(np.concatenate([np.asarray(l[i], dt) for l in lists if l is not None] + [np.zeros(0, dt)]))
    return off, cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)


def run(ctx, items, **params):
    """One Context.trio call: [(status, (index, a, b), (Jmax, S, denovo, paternal), J)] per item, and the raw arrays."""
    n = len(items)
    child, father, mother = (_pack([getattr(it, role) for it in items]) for role in ("child", "father", "mother"))
    status, call, values = np.full(n, -1, np.int32), np.full((n, 3), -1, np.int32), np.full((n, 4), np.nan)
    J = np.full(int(child[0][-1]), np.nan)
    ctx.trio(n, child, father, mother, np.array([it.ploidy for it in items], np.int32), np.array([it.f_inf for it in items], np.int32),
             np.array([it.m_inf for it in items], np.int32), status, call, values, J, **params)
    per = [(int(status[i]), tuple(call[i].tolist()), tuple(values[i].tolist()), J[child[0][i]:child[0][i + 1]]) for i in range(n)]
    return per, (status, call, values, J)


def _seen(name, diff):
    OBSERVED[name] = max(OBSERVED.get(name, 0.0), float(diff))


def same(got, want, what=""):
    """One item of run() against the model's dict."""
    status, (index, a, b), (Jmax, S, denovo, paternal), J = got
    assert status == want["status"], what
    if status not in (tm.OK, tm.DEGENERATE):
        assert (index, a, b) == (0, 0, 0) and (Jmax, S, denovo, paternal) == (0, 0, 0, 0) and not J.any(), what
        return
    assert want["gap"] > 1e-5, what                                 # every case has a call to compare
    assert (index, (a, b)) == (want["index"], want["call"]), what
    _seen("J", np.abs(J - want["J"]).max())
    _seen("Jmax", abs(Jmax - want["Jmax"]))
    _seen("log S", abs(math.log(S) - math.log(want["S"])))
    assert np.abs(J - want["J"]).max() <= TOL and abs(Jmax - want["Jmax"]) <= TOL, what
    assert abs(math.log(S) - math.log(want["S"])) <= TOL and abs(1 / S - want["post"]) <= TOL, what
    if status == tm.DEGENERATE:
        assert (denovo, paternal) == (0, 0), what
        return
    _seen("denovo", abs(denovo - want["denovo"]))
    _seen("paternal", abs(paternal - want["paternal"]))
    assert abs(denovo - want["denovo"]) <= TOL and abs(paternal - want["paternal"]) <= TOL, what


def check(ctx, items, **params):
    got, _ = run(ctx, items, **params)
    for k, (g, it) in enumerate(zip(got, items)):
        same(g, it.model(**params), "item {}".format(k))
    return got


@pytest.fixture(scope="module", autouse=True)
def observed():
    yield
    print("\nlargest differences from the model:", json.dumps(OBSERVED, sort_keys=True))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "grid.json")) as fp:
        cases = json.load(fp)["cases"]
    z = np.load(os.path.join(HERE, "golden", "grid.npz"))
    return {c["name"]: tm.pairs_from_grid(z["mls_%d" % i], 3) for i, c in enumerate(cases) if c["locus"] == "HD" and "mls_%d" % i in z.files}


ROWS = [("hd_typical", "hd_fullsearch", "hd_low_cov"), ("hd_typical", "hd_close", "hd_homo"),
        ("hd_no_full", "hd_expanded_rept_pe", "hd_dup_axis"), ("hd_expanded_rept_pe", "hd_100x", "hd_close"),
        ("hd_low_cov", "hd_typical", "hd_homo"), ("hd_close", "hd_homo", "hd_typical")]


def test_the_orientation_rows(ctx, golden):
    ctx.reset_timing()
    got = check(ctx, [Item(*(golden[n] for n in names)) for names in ROWS])
    assert [g[1][1:] for g in got] == [(15, 41), (15, 41), (66, 81), (20, 72), (15, 41), (17, 19)]
    n, ms = ctx.get_timing(_lib.KERNEL_TRIO)
    assert n == 1 and ms > 0
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_TRIO) == (0, 0.0)


def test_golden_lists_in_every_role(ctx, golden):
    g = golden
    assert len(g["hd_empty"][0]) == 0 and len(g["hd_homo"][0]) == len(g["hd_partial_only"][0]) == 1
    assert len(g["hd_rept_only_extended"][0]) == 5460
    items = [Item(g["hd_empty"], g["hd_typical"], g["hd_close"]),                         # EMPTY_CHILD
             Item(g["hd_typical"], g["hd_empty"], g["hd_low_cov"]),                       # an empty list says nothing
             Item(g["hd_typical"], g["hd_fullsearch"], g["hd_empty"], m_inf=0),
             Item(g["hd_typical"], None, None),
             Item(g["hd_haploid"], g["hd_100x"], g["hd_typical"], ploidy=1),              # the father is ignored
             Item(g["hd_haploid"], None, g["hd_haploid"], ploidy=1),
             Item(g["hd_typical"], g["hd_haploid"], g["hd_low_cov"]),
             Item(g["hd_rept_only_extended"], g["hd_typical"], g["hd_rept_only_extended"]),
             Item(g["hd_typical"], g["hd_rept_only_extended"], g["hd_fullsearch"])]
    for one in ("hd_homo", "hd_partial_only"):
        items += [Item(g[one], g["hd_typical"], g["hd_close"]), Item(g["hd_typical"], g[one], g["hd_low_cov"]),
                  Item(g["hd_typical"], g["hd_fullsearch"], g[one]), Item(g[one], g[one], g[one])]
    got = check(ctx, items)
    assert got[0][0] == tm.EMPTY_CHILD and got[4][1][1:] == (22, 22) and got[4][2][3] == 0.0
    assert got[1][3].tolist() == check(ctx, [Item(g["hd_typical"], None, g["hd_low_cov"])])[0][3].tolist()
    assert np.array_equal(got[4][3], check(ctx, [Item(g["hd_haploid"], None, g["hd_typical"], ploidy=1)])[0][3])


def crafted(rng, n, lo=10, hi=70, distinct=None):
    """n pairs (a <= b) drawn without repeats from lo .. hi (or the first n of the diagonal-first enumeration of `distinct`
    alleles), lw distinct, the first 0."""
    if distinct is not None:
        al = lo + np.arange(distinct)
        a, b = np.concatenate([al, al[:-1]]), np.concatenate([al, al[1:]])
        a, b = a[:n], b[:n]
    else:
        ia, ib = np.triu_indices(hi - lo + 1)
        pick = rng.permutation(len(ia))[:n]
        a, b = lo + ia[pick], lo + ib[pick]
    assert len(a) == n
    lw = -np.sort(rng.random(n) * 6 + 0.05)
    lw[0] = 0.0
    return a.astype(np.int32), b.astype(np.int32), rng.permutation(lw)


@pytest.mark.parametrize("n_parent", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5])
def test_a_parent_at_the_pair_chunk(ctx, n_parent):
    rng = np.random.default_rng(n_parent)
    child = crafted(rng, 40, 20, 60)
    check(ctx, [Item(child, crafted(rng, n_parent, 10, 90), crafted(rng, 300)),
                Item(child, crafted(rng, 7), crafted(rng, n_parent, 10, 90))])


@pytest.mark.parametrize("n_alleles", [TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_a_child_at_the_gamete_tile(ctx, n_alleles):
    rng = np.random.default_rng(n_alleles)
    child = crafted(rng, 2 * n_alleles - 1, 30, distinct=n_alleles)
    assert len(set(child[0].tolist()) | set(child[1].tolist())) == n_alleles
    check(ctx, [Item(child, crafted(rng, 200, 20, 250), crafted(rng, 150, 20, 250))])


@pytest.mark.parametrize("n_child", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_child_lists_at_the_strides_of_the_child_kernel(ctx, n_child):
    rng = np.random.default_rng(n_child)
    check(ctx, [Item(crafted(rng, n_child), crafted(rng, 90), crafted(rng, 110)),
                Item(crafted(rng, n_child), crafted(rng, 90), None, ploidy=2)])


def test_alleles_at_the_ends_of_the_range(ctx):
    one = lambda *pairs: (np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32),
                          -0.5 * np.arange(len(pairs)))
    edge = one((0, 1), (0, 0), (1, CAP), (CAP, CAP), (0, CAP), (1, 1))
    got = check(ctx, [Item(edge, one((0, CAP), (1, 2)), one((1, CAP - 1), (0, 0))), Item(edge, edge, edge),
                      Item(one((0, CAP + 1)), edge, edge), Item(edge, one((3, 4), (CAP + 1, CAP + 1)), edge),
                      Item(edge, edge, one((2, CAP + 7))), Item(edge, one((3, 4), (CAP + 1, CAP + 1)), edge, f_inf=0)],
                rho=0.99)
    assert [g[0] for g in got] == [tm.OK, tm.OK, tm.TOO_LONG, tm.TOO_LONG, tm.TOO_LONG, tm.OK]


def test_weights_that_underflow(ctx):
    rng = np.random.default_rng(5)
    child, father, mother = crafted(rng, 30), crafted(rng, 50), crafted(rng, 1500)
    for l in (child, father, mother):
        l[2][1::3] = -800.0                                         # exp(-800) is 0
    got = check(ctx, [Item(child, father, mother)])
    assert math.exp(-800.0) == 0.0 and got[0][0] == tm.OK
    # a parent none of whose weights is a number above 0: 0 / 0 in its gamete tables, and so in the child's sums
    dead = (father[0], father[1], np.full(len(father[0]), -800.0))
    got = check(ctx, [Item(child, dead, mother)])
    assert got[0][0] == tm.DEGENERATE


def test_the_floor_and_degenerate(ctx):
    one = lambda x, y: (np.array([x], np.int32), np.array([y], np.int32), np.zeros(1))
    got = check(ctx, [Item(one(100, 100), one(30, 30), one(30, 30))], rho=0.5)
    assert got[0][0] == tm.OK and abs(got[0][3][0] + 100.0) <= 1e-9 and got[0][2][2] == 1.0
    got = check(ctx, [Item(one(500, 600), one(30, 30), one(30, 30))], rho=0.01)
    assert got[0][0] == tm.DEGENERATE and abs(got[0][3][0] + 100.0) <= 1e-9 and got[0][1] == (0, 500, 600)


def test_the_tie_rule(ctx):
    a, b = np.array([12, 10, 10, 9, 9], np.int32), np.array([30, 30, 31, 40, 41], np.int32)
    lw = np.array([0.0, 0.0, 0.0, -1.0, -1.0])
    got, _ = run(ctx, [Item((a, b, lw)), Item((a[::-1].copy(), b[::-1].copy(), lw[::-1].copy()))])
    assert got[0][1] == (1, 10, 30) and got[1][1] == (2, 10, 31)    # the largest J, the smallest x, the first
    assert tm.evaluate((a, b, lw), None, None)["index"] == 1
    many = (np.full(700, 7, np.int32), 8 + np.arange(700, dtype=np.int32), np.zeros(700))
    assert run(ctx, [Item(many)])[0][0][1] == (0, 7, 8)


def _bad_lists():
    ok = lambda: [np.array([5, 6, 7], np.int32), np.array([9, 9, 9], np.int32), np.array([0.0, -1.0, -2.0])]
    out = {}
    for name, (col, value) in {"a above b": (0, 10), "a negative": (0, -1), "lw nan": (2, math.nan), "lw inf": (2, math.inf),
                               "lw minus inf": (2, -math.inf), "lw positive": (2, 1e-9)}.items():
        l = ok()
        l[col][1] = value
        out[name] = tuple(l)
    l = ok()
    l[0][2], l[1][2] = -3, -2                                       # both negative, in order
    out["both negative"] = tuple(l)
    return tuple(ok()), out


def test_every_bad_item_cause(ctx):
    ok, bad = _bad_lists()
    items, names = [], []
    for name, l in sorted(bad.items()):
        items += [Item(l, ok, ok), Item(ok, l, ok), Item(ok, ok, l), Item(ok, l, ok, f_inf=0)]
        names += [name] * 4
    items += [Item(ok, ok, ok, ploidy=p) for p in (0, 3, -1)] + [Item(ok, ok, ok)]
    got = check(ctx, items)
    want = [tm.BAD_ITEM, tm.BAD_ITEM, tm.BAD_ITEM, tm.OK] * len(bad) + [tm.BAD_ITEM] * 3 + [tm.OK]
    assert [g[0] for g in got] == want
    # a pair that is both wrong and too long is wrong; an empty child with a bad parent is refused for the parent
    long_and_bad = (np.array([CAP + 5], np.int32), np.array([CAP + 2], np.int32), np.zeros(1))
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    got = check(ctx, [Item(long_and_bad, ok, ok), Item(empty, bad["lw nan"], ok), Item(empty, None, None)])
    assert [g[0] for g in got] == [tm.BAD_ITEM, tm.BAD_ITEM, tm.EMPTY_CHILD]


def test_a_batch_of_nine_equals_its_items_one_by_one(ctx, golden):
    g, rng = golden, np.random.default_rng(9)
    ok, bad = _bad_lists()
    items = [Item(g["hd_typical"], g["hd_fullsearch"], g["hd_low_cov"]), Item(crafted(rng, 300), crafted(rng, CHUNK + 9), crafted(rng, 64)),
             Item(g["hd_close"], g["hd_homo"], g["hd_typical"]), Item(crafted(rng, 65), None, crafted(rng, 2000, 10, 90)),
             Item(bad["a above b"], g["hd_typical"], g["hd_close"]),                      # refused
             Item(g["hd_empty"], g["hd_typical"], g["hd_close"]),                         # empty
             Item(g["hd_no_full"], g["hd_expanded_rept_pe"], g["hd_dup_axis"]), Item(g["hd_haploid"], ok, g["hd_typical"], ploidy=1),
             Item(crafted(rng, 129, 100, 170, distinct=65), crafted(rng, 31), crafted(rng, 1023))]
    batch = check(ctx, items)
    assert [b[0] for b in batch] == [0, 0, 0, 0, tm.BAD_ITEM, tm.EMPTY_CHILD, 0, 0, 0]
    for k, it in enumerate(items):
        alone = run(ctx, [it])[0][0]
        assert alone[:3] == batch[k][:3] and alone[3].tobytes() == batch[k][3].tobytes(), k
    # in another order and with other neighbours, too
    back = run(ctx, items[::-1])[0][::-1]
    for x, y in zip(batch, back):
        assert x[:3] == y[:3] and x[3].tobytes() == y[3].tobytes()


def test_a_call_beyond_the_launch_caps(ctx):
    """70 000 items of six classes: more items than a launch has workgroups (65 536), so trio_prepare_kernel and
    trio_child_kernel stride over the items, and twice as many gamete work units and more, so trio_gamete_kernel strides and
    finds an item by its binary search over tile counts that differ from class to class.  Every item has the bits of its
    class alone, and every class is the model's."""
    rng = np.random.default_rng(70)
    ok, bad = _bad_lists()
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    classes = [Item(crafted(rng, 5), crafted(rng, 7), crafted(rng, 9)), Item(crafted(rng, 40), crafted(rng, 12), crafted(rng, 3)),
               Item(crafted(rng, 6), None, crafted(rng, 8)), Item(bad["a above b"], ok, ok), Item(empty, ok, ok),
               Item(crafted(rng, 70, distinct=40), crafted(rng, 20), crafted(rng, 20))]
    alone = check(ctx, classes)
    assert [a[0] for a in alone] == [tm.OK, tm.OK, tm.OK, tm.BAD_ITEM, tm.EMPTY_CHILD, tm.OK]
    which = rng.choice(len(classes), 70000, p=[0.3, 0.2, 0.15, 0.05, 0.05, 0.25])
    tiles = [(min(2 * len(c.child[0]), CAP + 1) + TILE - 1) // TILE for c in classes]
    assert tiles == [1, 2, 1, 1, 0, 3] and len(which) > 65536 and 2 * sum(tiles[c] for c in which) > 2 * 65536
    got, _ = run(ctx, [classes[c] for c in which])
    wrong = [i for i, (g, c) in enumerate(zip(got, which)) if g[:3] != alone[c][:3] or g[3].tobytes() != alone[c][3].tobytes()]
    assert not wrong, (len(wrong), wrong[:10], [int(which[i]) for i in wrong[:10]])


@pytest.mark.parametrize("params", [dict(mu=1e-6), dict(mu=0.5), dict(rho=0.01), dict(rho=0.99), dict(beta=0.0), dict(beta=1.0),
                                    dict(mu=0.3, rho=0.7, beta=0.2)])
def test_parameters(ctx, golden, params):
    rng = np.random.default_rng(17)
    items = [Item(*(golden[n] for n in ROWS[0])), Item(*(golden[n] for n in ROWS[3])),
             Item(crafted(rng, 70, 10, 40), crafted(rng, 40, 10, 40), crafted(rng, 45, 10, 40))]
    check(ctx, items, **params)


@pytest.mark.parametrize("params", [dict(mu=0.0), dict(mu=1.0), dict(mu=-0.1), dict(mu=math.nan), dict(rho=0.0), dict(rho=1.0),
                                    dict(rho=1.5), dict(beta=-1e-9), dict(beta=1.0 + 1e-9), dict(beta=math.nan)])
def test_parameters_out_of_range_are_bad_arguments(ctx, golden, params):
    it = Item(golden["hd_close"], golden["hd_homo"], golden["hd_typical"])
    with pytest.raises(_lib.TredGpuError, match=r"\(-2\).*out of range"):
        run(ctx, [it], **params)
    # nothing was written, and the context goes on
    child = _pack([it.child])
    status = np.full(1, -7, np.int32)
    p = _lib.TrioParams(params.get("mu", 0.01), params.get("rho", 0.9), params.get("beta", 0.5))
    import ctypes as C
    rc = ctx.lib.tredtrio_evaluate(ctx.h, C.byref(p), 1, *[x.ctypes.data for x in child * 3], *[np.ones(1, np.int32).ctypes.data] * 3,
                                   status.ctypes.data, np.zeros(3, np.int32).ctypes.data, np.zeros(4).ctypes.data,
                                   np.zeros(len(child[1])).ctypes.data)
    assert rc == -2 and status[0] == -7
    check(ctx, [it])


def test_bad_arguments(ctx):
    ok = (np.array([5], np.int32), np.array([9], np.int32), np.zeros(1))
    with pytest.raises(_lib.TredGpuError, match=r"\(-2\)"):
        ctx.trio(1, (np.array([0, -1], np.int64),) + ok, _pack([ok]), _pack([ok]), np.ones(1, np.int32), np.ones(1, np.int32),
                 np.ones(1, np.int32), np.zeros(1, np.int32), np.zeros(3, np.int32), np.zeros(4), np.zeros(1))
    with pytest.raises(_lib.TredGpuError, match=r"\(-2\)"):
        ctx.trio(1, _pack([ok]), _pack([ok]), _pack([ok]), None, np.ones(1, np.int32), np.ones(1, np.int32), np.zeros(1, np.int32),
                 np.zeros(3, np.int32), np.zeros(4), np.zeros(1))
    ctx.trio(0, _pack([]), _pack([]), _pack([]), None, None, None, None, None, None, None)      # no item: nothing to do
    check(ctx, [Item(ok, ok, ok)])


def test_the_same_call_twice_gives_the_same_bits(ctx, golden):
    rng = np.random.default_rng(3)
    items = [Item(*(golden[n] for n in names)) for names in ROWS] + [Item(crafted(rng, 500), crafted(rng, 1700), crafted(rng, 1100))]
    _, first = run(ctx, items)
    _, again = run(ctx, items)
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes()


def test_engine_trio(ctx, golden):
    engine = eng.Engine(ctx=ctx)
    lists = {k: trio.PairList(*v) for k, v in golden.items()}
    names = ROWS + [("hd_empty", "hd_typical", "hd_close")]
    ctx.reset_timing()
    res = engine.trio([lists[n[0]] for n in names], [lists[n[1]] for n in names], [lists[n[2]] for n in names[:-1]] + [None], 2)
    assert ctx.get_timing(_lib.KERNEL_TRIO)[0] == 1                 # one call for all items
    for r, n in zip(res[:-1], ROWS):
        want = tm.evaluate(*(golden[x] for x in n))
        assert (r.status, r.index, r.call) == (tm.OK, want["index"], want["call"]) and r.pairs is lists[n[0]]
        assert abs(r.post - want["post"]) <= TOL and abs(r.denovo - want["denovo"]) <= TOL and abs(r.paternal - want["paternal"]) <= TOL
        assert np.abs(r.J - want["J"]).max() <= TOL
        mine, theirs = r.P_h1h2(), tm.sparsify(golden[n[0]], want["J"], want["Jmax"], want["S"])
        assert sorted(mine) == sorted(theirs) and max(abs(mine[k] - theirs[k]) for k in mine) <= TOL
    assert res[-1].status == tm.EMPTY_CHILD and res[-1].call == (-1, -1) and res[-1].post is None and res[-1].P_h1h2() == ""
    assert res[2].call == (66, 81) and res[2].to_dict()["status"] == "OK"
    bad = trio.PairList([9], [5], [0.0])
    with pytest.raises(_lib.TredGpuError, match="trio: status {} .* unit 1".format(tm.BAD_ITEM)):
        engine.trio([lists["hd_close"], bad], [None, None], [lists["hd_homo"]] * 2, 2)
    with pytest.raises(_lib.TredGpuError, match=r"\(-2\)"):
        engine.trio([lists["hd_close"]], [None], [None], 2, mu=2.0)
    assert engine.trio([], [], [], 2) == []
