"""The items the cohort unit is tested on (tests/test_cohort_gpu.py), kept apart so that tests/test_cohort_model.py can show
on the CPU, with the model alone, that every one of them has a call to compare (a gap above 1e-5; where a tie is intended,
an exact one and more than 1e-5 beyond it) and the status it is meant to have.  An item is (samples, ploidy): samples a
list of (a, b, lw) or None, ploidy one or per sample."""
import json
import os

import numpy as np

from . import cohort_model as cm
from . import trio_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = 1024                    # TREDGPU_COHORT_CHUNK
LONG_LIST = 1024                # TREDGPU_COHORT_LONG_LIST: longer lists take the kernels' other path
CAP = cm.MAX_ALLELE
GOLDEN_NAMES = []


def golden_lists():
    """{name: (a, b, lw)} of the golden HD grids (period 3), in the order of grid.json."""
    with open(os.path.join(HERE, "golden", "grid.json")) as fp:
        cases = json.load(fp)["cases"]
    z = np.load(os.path.join(HERE, "golden", "grid.npz"))
    return {c["name"]: tm.pairs_from_grid(z["mls_%d" % i], 3) for i, c in enumerate(cases) if c["locus"] == "HD" and "mls_%d" % i in z.files}


def golden_cohort():
    """The 13 non-empty golden HD lists as one item, hd_haploid at ploidy 1."""
    g = golden_lists()
    names = [n for n in g if len(g[n][0])]
    GOLDEN_NAMES[:] = names
    return [g[n] for n in names], [1 if n == "hd_haploid" else 2 for n in names]


def crafted(n, seed, base=10):
    """A list of n pairs over consecutive alleles from `base`: every (a, b), a <= b, in order until there are n; lw drawn in
    -30 .. -3 with a lone 0."""
    rng = np.random.RandomState(seed)
    m = 1
    while m * (m + 1) // 2 < n:
        m += 1
    pairs = [(base + i, base + j) for i in range(m) for j in range(i, m)][:n]
    lw = -rng.uniform(3.0, 30.0, n)
    lw[rng.randint(n)] = 0.0
    return np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32), lw


def one(a, b, lw=0.0):
    return np.array([a], np.int32), np.array([b], np.int32), np.array([lw], np.float64)


def lst(*triples):
    return (np.array([t[0] for t in triples], np.int32), np.array([t[1] for t in triples], np.int32),
            np.array([t[2] for t in triples], np.float64))


def small_item(n):
    """n diploid samples of three pairs each over the alleles 5, 9 and 12."""
    return [lst((5, 5, -0.5 * s), (5, 9, 0.0), (9, 12, -1.0 - s)) for s in range(n)], 2


def entries_item(entries):
    """An item whose allele 5 has exactly `entries` incidence entries: samples of {(5, 5): -1, (5, 9): 0} give three each, a
    sample of the single pair (5, 11) one."""
    samples = [lst((5, 5, -1.0), (5, 9, 0.0)) for _ in range(entries // 3)] + [one(5, 11) for _ in range(entries % 3)]
    return samples, 2


def support_item(A):
    """An item whose support is the alleles 0 .. A - 1: samples over windows of 40 alleles, each with the homozygous pairs and
    the pairs of neighbours of its window."""
    samples = []
    for lo in range(0, A, 40):
        hi = min(lo + 40, A)
        t = [(c, c, -1.0 - (c * 7 % 5)) for c in range(lo, hi)] + [(c, c + 1, -2.0 - (c * 3 % 7)) for c in range(lo, hi - 1)]
        t[(lo // 40) % len(t)] = t[(lo // 40) % len(t)][:2] + (0.0,)
        samples.append(lst(*t))
    return samples, 2


def _sizes():
    return [crafted(n, 100 + n) for n in (1, 63, 64, 65, 255, 256, 257, 1000)], 2


def _mixed_ploidy():
    return [crafted(65, 1), one(12, 12), lst((11, 11, -2.0), (13, 13, 0.0), (20, 20, -0.7)), crafted(30, 2), one(40, 40)], [2, 1, 1, 2, 2]


def _empty_samples():
    e = lst()
    return [e, None, crafted(20, 3), e, crafted(64, 4), None, e], [2, 1, 2, 2, 2, 1, 2]


CASES = {
    "one_sample": lambda: ([([crafted(40, 7)], 2)], {}),
    "one_allele": lambda: ([([one(7, 7), one(7, 7, -3.0), one(7, 7)], [2, 1, 2])], {}),
    "one_pair_one_sample": lambda: ([([one(0, 1024)], 2)], {}),
    "list_sizes": lambda: ([_sizes()], {}),
    "long_list_threshold": lambda: ([([crafted(n, 200 + n) for n in (LONG_LIST - 1, LONG_LIST, LONG_LIST + 1, 2 * LONG_LIST + 1)], 2)], dict(iters=16)),
    "chunk_minus_1": lambda: ([entries_item(CHUNK - 1)], dict(iters=3)),
    "chunk": lambda: ([entries_item(CHUNK)], dict(iters=3)),
    "chunk_plus_1": lambda: ([entries_item(CHUNK + 1)], dict(iters=3)),
    "two_chunks_plus_5": lambda: ([entries_item(2 * CHUNK + 5)], dict(iters=3)),
    "support_1_64_65": lambda: ([([one(3, 3)], 1), support_item(64), support_item(65)], dict(iters=8)),
    "support_1025": lambda: ([support_item(CAP + 1)], dict(iters=8)),
    "alleles_0_and_1024": lambda: ([([lst((0, 0, -1.0), (0, 1024, 0.0), (1024, 1024, -2.0)), one(0, 0), one(1024, 1024)], [2, 2, 1])], {}),
    "lw_minus_800": lambda: ([([lst((5, 6, -800.0), (5, 7, 0.0), (6, 6, -2.0)), lst((6, 7, 0.0), (7, 7, -800.0))], 2)], {}),
    "max_lw_minus_50": lambda: ([([lst((5, 6, -50.0), (5, 7, -53.0), (6, 6, -51.5)), crafted(10, 5, base=4)], 2)], {}),
    "mixed_ploidy": lambda: ([_mixed_ploidy()], {}),
    "empty_samples": lambda: ([_empty_samples()], {}),
}

_GOOD = [lst((5, 6, 0.0), (6, 6, -1.0)), one(5, 5)]
REFUSED = {
    "a_above_b": lambda: ((_GOOD + [lst((5, 6, 0.0), (7, 6, -1.0))], 2), cm.BAD_ITEM),
    "negative_allele": lambda: ((_GOOD + [lst((-1, 6, 0.0))], 2), cm.BAD_ITEM),
    "lw_nan": lambda: ((_GOOD + [lst((5, 6, float("nan")))], 2), cm.BAD_ITEM),
    "lw_inf": lambda: ((_GOOD + [lst((5, 6, float("inf")))], 2), cm.BAD_ITEM),
    "lw_minus_inf": lambda: ((_GOOD + [lst((5, 6, 0.0), (6, 6, float("-inf")))], 2), cm.BAD_ITEM),
    "lw_positive": lambda: ((_GOOD + [lst((5, 6, 1e-300))], 2), cm.BAD_ITEM),
    "ploidy_0": lambda: ((_GOOD, [2, 0]), cm.BAD_ITEM),
    "ploidy_3": lambda: ((_GOOD, [3, 2]), cm.BAD_ITEM),
    "ploidy_of_an_empty_sample": lambda: ((_GOOD + [None], [2, 2, 7]), cm.BAD_ITEM),
    "heterozygous_at_ploidy_1": lambda: ((_GOOD, [1, 2]), cm.BAD_ITEM),
    "allele_1025": lambda: ((_GOOD + [one(5, CAP + 1)], 2), cm.TOO_LONG),
    "allele_far_too_long": lambda: ((_GOOD + [one(2 ** 31 - 1, 2 ** 31 - 1)], 2), cm.TOO_LONG),
    "bad_before_too_long": lambda: ((_GOOD + [one(5, CAP + 1), lst((9, 8, 0.0))], 2), cm.BAD_ITEM),
    "too_long_before_empty": lambda: (([None, one(CAP + 1, CAP + 1)], 2), cm.TOO_LONG),
    "bad_in_an_item_without_pairs": lambda: (([None, None], [2, 5]), cm.BAD_ITEM),
    "empty": lambda: (([None, lst(), None], [2, 1, 2]), cm.EMPTY),
    "no_sample": lambda: (([], 2), cm.EMPTY),
}


def peaked(n, at, seed, base=10):
    """crafted(n, seed, base) with its lone 0 at position `at`."""
    a, b, lw = crafted(n, seed, base)
    lw[lw == 0.0] = -3.0
    lw[at] = 0.0
    return a, b, lw


def haploid(n, seed, distinct=None):
    """A ploidy-1 list of n homozygous pairs: over the alleles 0 .. n - 1 in order, or drawn from 0 .. distinct - 1 with
    repeats; lw drawn in -30 .. -3 with a lone 0."""
    rng = np.random.RandomState(seed)
    a = np.arange(n, dtype=np.int32) if distinct is None else rng.randint(0, distinct, n).astype(np.int32)
    lw = -rng.uniform(3.0, 30.0, n)
    lw[rng.randint(n)] = 0.0
    return a, a.copy(), lw


def fillers(n, seed):
    """n pairs over consecutive alleles from 100 up, lw drawn in -40 .. -30: what a list is padded with."""
    a, b, _ = crafted(n, seed, base=100)
    return a, b, -np.random.RandomState(seed).uniform(30.0, 40.0, n)


def with_pairs(l, at, pairs):
    """The list l with the pairs (a, b, lw) put in place of those at the positions `at`."""
    a, b, lw = (x.copy() for x in l)
    for k, (x, y, v) in zip(at, pairs):
        a[k], b[k], lw[k] = x, y, v
    return a, b, lw


def join(*lists):
    return tuple(np.concatenate([l[i] for l in lists]) for i in range(3))


# The workgroup path (lists of more than LONG_LIST pairs) at the edges of its strides and wavefronts, and at ploidy 1.
LONG_PEAKS = [(LONG_LIST + 1, at) for at in (0, 63, 64, 255, 256, 1023, 1024)] + [(2 * LONG_LIST + 1, at) for at in (2047, 2048)]
CASES["long_list_edges"] = lambda: ([([peaked(n, at, 300 + at) for n, at in LONG_PEAKS], 2),
                                     ([haploid(CAP + 1, 31), haploid(1500, 32, distinct=200)], 1)], dict(iters=16))

# Exact ties.  Two mechanisms make them exact on any device: a pair that stands twice in a list -- the same q bit for bit
# under any f, the earlier one wins -- and an item that is invariant under swapping the alleles 5 and 7, whose f(5) and f(7)
# are equal bit for bit by induction over the iterations (their incidence lists have the same length, order and values): the
# call is the pair with a = 5, although it comes second.
# (n, i, j): a list of n pairs with the pair (6, 8, 0) at i and j.  The wavefront's path: the lanes 0 and 1, one lane in two
# strides, the last partial stride.  The workgroup's: one wavefront, two wavefronts, one thread in two strides, the last
# partial stride.
DUPLICATES = [(100, 0, 1), (100, 5, 69), (150, 129, 149), (150, 60, 149),
              (1100, 10, 20), (1100, 10, 138), (1100, 10, 266), (1100, 200, 1099), (1100, 1030, 1090)]
SYM, SYM_HOMO = lst((7, 9, 0.0), (5, 9, 0.0), (9, 9, -3.0)), lst((7, 7, 0.0), (5, 5, 0.0), (9, 9, -3.0))
TIES = {
    "duplicates": lambda: ([([with_pairs(fillers(n, 400 + k), (i, j), [(6, 8, 0.0)] * 2) for k, (n, i, j) in enumerate(DUPLICATES)], 2)],
                           dict(iters=16)),
    "symmetric": lambda: ([([SYM, SYM_HOMO, join(fillers(70, 41), SYM), join(fillers(1100, 42), SYM), SYM], 2)], dict(iters=16)),
    "symmetric_ploidy_1": lambda: ([([lst((7, 7, 0.0), (5, 5, 0.0), (9, 9, -1.0)), SYM], [1, 2])], dict(iters=16)),
}
TIE_CALLS = {"duplicates": [[i for _, i, _ in DUPLICATES]], "symmetric": [[1, 1, 71, 1101, 1]], "symmetric_ploidy_1": [[1, 1]]}


def _long_refused(changes, ploidy=2):
    """_GOOD and a list of 1100 pairs, changed at {index: (a, b, lw)}."""
    l = haploid(1100, 51, distinct=300) if ploidy == 1 else peaked(1100, 17, 52)
    at = sorted(changes)
    return _GOOD + [with_pairs(l, at, [changes[k] for k in at])], [2, 2, ploidy]


REFUSED.update({
    "long_a_above_b_in_wavefront_3": lambda: (_long_refused({200: (30, 20, -5.0)}), cm.BAD_ITEM),
    "long_a_above_b_in_the_second_stride": lambda: (_long_refused({1024: (30, 20, -5.0)}), cm.BAD_ITEM),
    "long_nan_last": lambda: (_long_refused({1099: (20, 30, float("nan"))}), cm.BAD_ITEM),
    "long_allele_1025": lambda: (_long_refused({300: (20, CAP + 1, -5.0)}), cm.TOO_LONG),
    "long_bad_before_too_long": lambda: (_long_refused({100: (20, CAP + 1, -5.0), 900: (30, 20, -5.0)}), cm.BAD_ITEM),
    "long_heterozygous_at_ploidy_1": lambda: (_long_refused({700: (3, 4, -5.0)}, ploidy=1), cm.BAD_ITEM),
})

# The classes of the call beyond the launch caps (tests/test_cohort_gpu.py): supports of 3, 4, 4 and 6 alleles, a refused
# and an empty item.
BIG_CLASSES = [small_item(2), ([crafted(10, 11)], 2),
               ([lst((3, 3, -1.0), (3, 8, 0.0), (8, 20, -2.5)), one(20, 20), lst((2, 2, 0.0), (8, 8, -1.0))], [2, 2, 1]),
               REFUSED["a_above_b"]()[0], REFUSED["empty"]()[0], ([crafted(21, 12, base=0), one(3, 3)], 2)]
BIG_N, BIG_ITERS = 70000, 3
OTHER_ALLELES = ([lst((1, 1, -0.5), (1, 4, 0.0), (4, 700, -1.0)), one(4, 4)], 2)    # a small item over alleles of its own


def big_call():
    """The class of every item of the big call: more than 65 536 items and more than 4 x 65 536 chunks."""
    return np.random.RandomState(70).choice(len(BIG_CLASSES), BIG_N, p=[0.1, 0.3, 0.15, 0.05, 0.05, 0.35])


def batch_of_nine(golden):
    """Nine items, a refused and an empty one in the middle."""
    return [small_item(4), CASES["mixed_ploidy"]()[0][0], golden, REFUSED["a_above_b"]()[0], REFUSED["empty"]()[0],
            support_item(65), _sizes(), CASES["lw_minus_800"]()[0][0], entries_item(70)]


GOLDEN_PARAMS = [dict(iters=1), dict(iters=2), dict(iters=64), dict(iters=64, alpha=1e-6), dict(iters=64, alpha=100.0)]


def compared(golden):
    """(name, item, parameters, ties) of every item the GPU tests compare with the model."""
    for params in GOLDEN_PARAMS:
        yield "golden", golden, params, False
    for group, ties in ((CASES, False), (TIES, True)):
        for name, make in group.items():
            items, params = make()
            for item in items:
                yield name, item, params, ties
    for item in batch_of_nine(golden):
        yield "batch_of_nine", item, dict(iters=7), False
    for item in BIG_CLASSES:
        yield "big_call", item, dict(iters=BIG_ITERS), False
    yield "small_item(3)", small_item(3), dict(iters=5), False
    yield "other_alleles", OTHER_ALLELES, dict(iters=5), False
    yield "iteration_cap", small_item(2), dict(iters=cm.MAX_ITERS), False
