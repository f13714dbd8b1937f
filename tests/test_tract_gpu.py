"""tredtract_scan (include/tredtract.h, csrc/tract.hip) against the definition (tests/tract_model.py), field by field: a gap
at every edge of a lane and of a tile, seeds longer than a tile, a chain of thousands of seeds across the workgroups of the
device-wide prefix sums, dense seeds, N and case, random planted segments, the perfect scan as the special case, and the
contract of the call."""
import ctypes as C

import numpy as np
import pytest

from tredparse_amd import _lib

from . import scan_model as sm
from . import tract_model as tm

pytestmark = pytest.mark.gpu

T = _lib.SCAN_TILE
MOTIFS = {1: "A", 2: "AC", 3: "CAG", 4: "GATA", 5: "AACCT", 6: "AAGGCT"}
SEEDS = tm.SEED_COPIES                     # min_copies == seed_copies: a seed alone is a record too
SENTINEL = -77


def rand_letters(seed, n, alphabet="ACGT"):
    return np.frombuffer("".join(alphabet).encode(), np.uint8)[np.random.default_rng(seed).integers(0, len(alphabet), n)].copy()


def as_buf(text):
    return np.frombuffer(text.encode() if isinstance(text, str) else text, np.uint8)


def gpu_tracts(ctx, buf, seg_off, mc=sm.MIN_COPIES, sc=tm.SEED_COPIES, mg=tm.MAX_GAP, cap=1 << 16):
    out = ctx.scan_tracts(buf, seg_off, mc, sc, mg, cap)
    assert out[6] == len(out[0])
    return list(zip(*(x.tolist() for x in out[:6])))


def other(ch):
    return "ACGT"[("ACGT".index(ch) + 1) % 4]


def site(p, g, copies, shifted=False):
    """motif x copies, g letters that all differ from the template, the template again for `copies` copies; shifted: the
    right half goes on as if the g letters were not there (an insertion: the phase changes).  Returns (letters, where the
    gap begins)."""
    m = MOTIFS[p]
    left = m * copies
    gap = "".join(other(m[(len(left) + j) % p]) for j in range(g))
    phase = len(left) + (0 if shifted else g)
    right = "".join(m[(phase + j) % p] for j in range(copies * p))
    return left + gap + right, len(left)


@pytest.fixture(scope="module")
def boundaries():
    """Random letters with, per period, gap size 1 .. max_gap + 1 and position, two seeds around a gap that begins d letters
    from a tile's first letter and another pair d letters from a lane's first letter in the middle of the tile, d from
    -(g + 1) to 1: the gap ends in front of the boundary, straddles it at every split, begins at it and behind it.  Per
    period also a pair with an inserted letter.  Returns (letters, [(gap start, g, period, linked?)])."""
    sites = []
    for p in range(1, 7):
        for g in range(1, tm.MAX_GAP[p - 1] + 2):
            for d in range(-g - 1, 2):
                sites.append((p, g, d, False))
        sites.append((p, 1, 0, True))
    buf = rand_letters(41, (len(sites) + 1) * T)
    placed = []
    for k, (p, g, d, shifted) in enumerate(sites):
        letters, at = site(p, g, SEEDS[p - 1] + 1, shifted)
        for boundary in ((k + 1) * T, k * T + 2048 + 64 * (k % 7)):
            start = boundary + d - at
            buf[start:start + len(letters)] = as_buf(letters)
            buf[start - 1] = ord(other(chr(buf[start - 1 + p])))            # the seeds end where the test means them to
            buf[start + len(letters)] = ord(other(chr(buf[start + len(letters) - p])))
            placed.append((boundary + d, g, p, g <= tm.MAX_GAP[p - 1] and (not shifted or p == 1)))
    return buf, placed


def test_gap_at_every_boundary_one_segment(ctx, boundaries):
    buf, placed = boundaries
    want = tm.tracts(buf, [0, len(buf)], SEEDS)
    have = {(r[1], r[2], r[3]): r for r in want}
    for gap_at, g, p, is_linked in placed:                                  # the tracts are what the test means them to be
        copies = SEEDS[p - 1] + 1
        whole = have.get((gap_at - copies * p, 2 * copies * p + g, p))
        if is_linked:
            assert whole is not None and whole[4:] == (2, g), (gap_at, g, p)
        else:
            assert whole is None and (gap_at - copies * p, copies * p, p) in have, (gap_at, g, p)
    assert gpu_tracts(ctx, buf, [0, len(buf)], SEEDS) == want
    assert gpu_tracts(ctx, buf, [0, len(buf)]) == tm.tracts(buf, [0, len(buf)])          # the default min_copies


def test_gap_at_every_boundary_segment_end_in_the_gap(ctx, boundaries):
    """The same letters with a segment's end in every gap: in front of it, inside it and behind it by turns.  Nothing is
    linked across it."""
    buf, placed = boundaries
    cuts = sorted({0, len(buf)} | {gap_at + (0, g // 2, g)[k % 3] for k, (gap_at, g, _, _) in enumerate(placed)})
    want = tm.tracts(buf, cuts, SEEDS)
    for gap_at, g, p, _ in placed:
        copies = SEEDS[p - 1] + 1
        assert not any(r[3] == p and r[2] == 2 * copies * p + g and r[5] == g for r in want if cuts[r[0]] + r[1] == gap_at - copies * p)
    assert gpu_tracts(ctx, buf, cuts, SEEDS) == want


def test_seeds_longer_than_a_tile(ctx):
    """A gap with a seed of more than a tile in front of it, behind it, on both sides; one tract over three tiles and more
    whose three seeds are each longer than a tile; the same with the last seed out of phase."""
    long3, long5 = "CAG" * (T // 3 + 40), "AACCT" * (T // 5 + 13)
    parts = [
        "TTGA" + long3 + "CAT" + "CAG" * 4 + "TTA",
        "TTGA" + "CAG" * 4 + "CTG" + long3 + "TTA",
        "GG" + long5 + "AAGCT" + long5 + "GG",
        "TT" + long3 + "CAA" + long3 + "CGG" + long3 + "TT",
        "TT" + long3 + "CAA" + long3 + "CGGA" + long3 + "TT",
    ]
    buf = as_buf("".join(parts))
    off = np.concatenate(([0], np.cumsum([len(x) for x in parts])))
    want = tm.tracts(buf, off)
    n3, n5 = len(long3), len(long5)
    assert {(0, 4, n3 + 15, 3, 2, 1), (1, 4, n3 + 15, 3, 2, 1), (2, 2, 2 * n5 + 5, 5, 2, 1), (3, 2, 3 * n3 + 6, 3, 3, 2),
            (4, 2, 2 * n3 + 4, 3, 2, 1)} <= set(want)
    assert gpu_tracts(ctx, buf, off) == want
    whole = as_buf(parts[3])                                               # one segment, and in front of it letters of none
    assert gpu_tracts(ctx, np.concatenate((as_buf("CAGCAGCAGCAG"), whole)), [12, 12 + len(whole)]) == tm.tracts(whole, [0, len(whole)])


def test_chain_of_thousands_of_seeds(ctx):
    """(CGG)9 AGG five thousand times: one tract of 5 000 seeds, whose list goes over twenty workgroups of the prefix sums.
    With a letter inserted in the middle: two."""
    unit, n = "CGG" * 9 + "AGG", 5000
    chain = "TA" + unit * n + "TA"
    want = tm.tracts(chain, [0, len(chain)])
    assert (0, 2, 30 * n - 3, 3, n, n - 1) in want
    assert gpu_tracts(ctx, as_buf(chain), [0, len(chain)]) == want
    broken = "TA" + unit * (n // 2) + "T" + unit * (n - n // 2) + "TA"
    want = tm.tracts(broken, [0, len(broken)])
    assert {(0, 2, 15 * n - 3, 3, n // 2, n // 2 - 1), (0, 15 * n + 3, 15 * n - 3, 3, n // 2, n // 2 - 1)} <= set(want)
    assert gpu_tracts(ctx, as_buf(broken), [0, len(broken)]) == want


def test_dense_seeds(ctx):
    """AAAAAC over and over: period-1 seeds of five letters that a C links, inside one perfect run of period 6.  And 20 000
    letters over {A, C} with the smallest seeds the rule allows."""
    dense = "G" + "AAAAAC" * 2000 + "G"
    want = tm.tracts(dense, [0, len(dense)])
    assert (0, 1, 12000 - 1, 1, 2000, 1999) in want and (0, 1, 12000, 6, 1, 0) in want
    assert gpu_tracts(ctx, as_buf(dense), [0, len(dense)]) == want
    buf = rand_letters(21, 20000, "AC")
    mc, mg = (3, 2, 2, 2, 2, 2), (2, 1, 1, 1, 1, 1)
    assert tm.rule_violation(mc, mc, mg) is None
    want = tm.tracts(buf, [0, 7000, len(buf)], mc, mc, mg)
    assert len(want) > 5000 and sum(1 for r in want if r[4] >= 2) > 400
    assert gpu_tracts(ctx, buf, [0, 7000, len(buf)], mc, mc, mg, cap=6 * len(buf)) == want


def test_n_case_and_empty_segments(ctx):
    parts = ["TT" + "CAG" * 6 + "CNG" + "CAG" * 6 + "TT",                  # an N in a gap is a mismatch
             "",
             "TT" + "cag" * 6 + "CtG" + "CAG" * 3 + "cAg" * 3 + "TT",      # codes, not bytes
             "TT" + "CAG" * 6 + "NNN" + "CAG" * 6 + "TT",
             "TT" + "CAG" * 6 + "NNNN" + "CAG" * 6 + "TT",                 # four letters: not linked
             "", "",
             "A" * 5 + "N" + "a" * 5]
    buf = as_buf("".join(parts))
    off = np.concatenate(([0], np.cumsum([len(x) for x in parts])))
    want = tm.tracts(buf, off)
    assert {(0, 2, 39, 3, 2, 1), (2, 2, 39, 3, 2, 1), (3, 2, 39, 3, 2, 3), (4, 2, 18, 3, 1, 0), (4, 24, 18, 3, 1, 0), (7, 0, 11, 1, 2, 1)} <= set(want)
    assert gpu_tracts(ctx, buf, off) == want


def test_the_largest_gap(ctx):
    """TREDTRACT_MAX_GAP letters between two seeds, all of them mismatches (the most a seed's byte of the link table holds),
    some of them, and one letter more: not linked.  Across a tile's edge and inside a lane."""
    mc, mg = (0, 0, 23, 0, 0, 30), (0, 0, 64, 0, 0, 64)
    assert tm.rule_violation(mc, mc, mg) is None and tm.rule_violation(mc, (0, 0, 22, 0, 0, 30), mg) is not None
    full3, at3 = site(3, 64, 25)
    full6, at6 = site(6, 64, 31)
    some = "CAG" * 25 + "".join("CAGT"[k % 4] if k % 5 else "N" for k in range(64)) + ("CAG" * 26)[64 % 3:][:75]
    over, _ = site(3, 65, 25)
    parts = ["T" * (T - at3 - 30) + full3 + "TT", "GG" + full6 + "GG", "TT" + some + "TT", "TT" + over + "TT"]
    buf = as_buf("".join(parts))
    off = np.concatenate(([0], np.cumsum([len(x) for x in parts])))
    want = tm.tracts(buf, off, mc, mc, mg)
    assert {(0, T - at3 - 30, 214, 3, 2, 64), (1, 2, 2 * 186 + 64, 6, 2, 64), (2, 2, 214, 3, 2, 50), (3, 2, 75, 3, 1, 0),
            (3, 142, 75, 3, 1, 0)} <= set(want)
    assert gpu_tracts(ctx, buf, off, mc, mc, mg) == want


def test_random_planted_segments(ctx):
    """Eight calls of 150 planted segments of 20 .. 160 letters each, over four alphabets, with random parameters within the
    rules per call."""
    rng = np.random.default_rng(20240612)
    multi = triple = 0
    for call in range(8):
        parts = [tm.planted(rng, ("AC", "ACG", "ACGT", "ACN")[k % 4]) for k in range(150)]
        mc, sc, mg = tm.random_params(rng)
        buf = as_buf("".join(parts))
        off = np.concatenate(([0], np.cumsum([len(x) for x in parts])))
        want = tm.tracts(buf, off, mc, sc, mg)
        multi += sum(1 for r in want if r[4] >= 2)
        triple += sum(1 for r in want if r[4] >= 3)
        assert gpu_tracts(ctx, buf, off, mc, sc, mg) == want, (call, mc, sc, mg)
    assert multi >= 100 and triple >= 10, (multi, triple)


def test_without_gaps_it_is_the_scan(ctx, boundaries):
    buf = boundaries[0]
    off = [0, 5 * T + 3, 5 * T + 3, 40 * T - 2, len(buf)]
    for mc in (sm.MIN_COPIES, (2,) * 6, (0, 3, 0, 2, 0, 5)):
        seg, start, length, period, total = ctx.scan(buf, off, mc, cap=len(buf))
        out = ctx.scan_tracts(buf, off, mc, mc, (0,) * 6, cap=len(buf))
        assert total == out[6] == len(seg) > 0
        for got, ref in zip(out[:4], (seg, start, length, period)):
            assert got.dtype == ref.dtype and np.array_equal(got, ref)
        assert (out[4] == 1).all() and (out[5] == 0).all()


def raw_call(ctx, buf, off, mc, sc, mg, cap, room=None, null=()):
    """tredtract_scan itself on sentinel-filled outputs: (rc, the six arrays, out_n).  null: the arguments passed as NULL."""
    room = max(cap, 1) if room is None else room
    outs = [np.full(room, SENTINEL, dt) for dt in (np.int32, np.int64, np.int32, np.int32, np.int32, np.int32)]
    off = np.asarray(off, np.int64)
    mc, sc, mg = (np.asarray(x, np.int32) for x in (mc, sc, mg))
    total = C.c_int64(SENTINEL)
    ptr = lambda a, name: None if name in null else a.ctypes.data
    rc = ctx.lib.tredtract_scan(ctx.h, ptr(buf, "letters"), ptr(off, "off"), len(off) - 1, ptr(mc, "mc"), ptr(sc, "sc"), ptr(mg, "mg"),
                                cap, *[ptr(o, "out") for o in outs], None if "n" in null else C.byref(total))
    return rc, outs, total.value


def test_cap_below_the_total(ctx, boundaries):
    buf = boundaries[0][:60 * T]
    want = tm.tracts(buf, [0, len(buf)], SEEDS)
    periods = [r[3] for r in want]
    assert len(set(periods)) >= 3 and periods != sorted(periods)           # (the merge of the periods' lists has work to do)
    for cap in (0, 1, len(want) // 2, len(want) - 1, len(want), len(want) + 5):
        rc, outs, total = raw_call(ctx, buf, [0, len(buf)], SEEDS, SEEDS, tm.MAX_GAP, cap, room=len(want) + 10)
        assert rc == 0 and total == len(want)
        k = min(cap, len(want))
        for got, ref in zip(outs, tm.arrays(want)):
            assert np.array_equal(got[:k], ref[:k]) and (got[k:] == SENTINEL).all()


def test_two_calls_identical_bytes(ctx, boundaries):
    buf = boundaries[0]
    first = raw_call(ctx, buf, [0, 100, len(buf)], SEEDS, SEEDS, tm.MAX_GAP, len(buf))
    other_call = raw_call(ctx, rand_letters(3, 3 * T), [0, 3 * T], SEEDS, SEEDS, tm.MAX_GAP, 3 * T)        # (another call in between)
    second = raw_call(ctx, buf, [0, 100, len(buf)], SEEDS, SEEDS, tm.MAX_GAP, len(buf))
    assert first[0] == second[0] == other_call[0] == 0 and first[2] == second[2] > 0
    for x, y in zip(first[1], second[1]):
        assert x.tobytes() == y.tobytes()


def test_period_switched_off(ctx, boundaries):
    buf = boundaries[0][-50 * T:]
    for mc in ((0, 6, 5, 4, 4, 4), (10, 0, 5, 0, 4, 6), (0, 0, 0, 0, 0, 4)):
        sc = [9 if m == 0 else s for m, s in zip(mc, tm.SEED_COPIES)]     # (of a period that is off: not read)
        mg = [99 if m == 0 else g for m, g in zip(mc, tm.MAX_GAP)]
        want = tm.tracts(buf, [0, len(buf)], mc)
        assert len(want) > 0 and gpu_tracts(ctx, buf, [0, len(buf)], mc, sc, mg) == want


def test_refusals_leave_outputs_untouched(ctx):
    buf = rand_letters(4, 1000)
    buf[100:190] = as_buf(tm.FMR1)
    ok = dict(off=[0, 1000], mc=sm.MIN_COPIES, sc=tm.SEED_COPIES, mg=tm.MAX_GAP, cap=16, null=())
    cases = {
        "the inequality": dict(mg=(1, 2, 5, 4, 5, 6)),                     # 3 * 3 > 5 + 4 does not hold
        "the inequality, period 1": dict(mg=(5, 2, 3, 4, 5, 6)),
        "seed_copies above min_copies": dict(sc=(5, 3, 6, 3, 3, 3)),
        "seed_copies 1": dict(sc=(5, 3, 3, 1, 3, 3)),
        "a negative gap": dict(mg=(1, 2, 3, -1, 5, 6)),
        "a gap above 64": dict(mc=(70, 40, 30, 20, 20, 20), sc=(70, 40, 30, 20, 20, 20), mg=(1, 65, 3, 4, 5, 6)),
        "letters NULL": dict(null=("letters",)), "seg_off NULL": dict(null=("off",)), "min_copies NULL": dict(null=("mc",)),
        "seed_copies NULL": dict(null=("sc",)), "max_gap NULL": dict(null=("mg",)), "outputs NULL": dict(null=("out",)),
        "out_n NULL": dict(null=("n",)),
        "descending": dict(off=[0, 600, 500, 1000]), "negative": dict(off=[-1, 1000]),
        "min_copies 1": dict(mc=(10, 6, 1, 4, 4, 4)), "min_copies -1": dict(mc=(10, 6, 5, 4, -1, 4)), "all off": dict(mc=(0,) * 6),
        "cap negative": dict(cap=-1), "too many letters": dict(off=[0, _lib.SCAN_MAX_LETTERS + 1]),
    }
    for name, change in cases.items():
        args = dict(ok, **change)
        rc, outs, total = raw_call(ctx, buf, args["off"], args["mc"], args["sc"], args["mg"], args["cap"], room=16, null=args["null"])
        assert rc == -2, name
        assert total == SENTINEL and all((o == SENTINEL).all() for o in outs), name
        assert ctx.lib.tredtract_last_error(), name
    rc, outs, total = raw_call(ctx, buf, ok["off"], (70, 40, 30, 20, 20, 20), (70, 40, 30, 20, 20, 20), (64, 64, 64, 64, 64, 64), 16)
    assert rc == 0 and total == 0                                          # (64 is allowed)
    rc, outs, total = raw_call(ctx, buf, ok["off"], ok["mc"], ok["sc"], ok["mg"], ok["cap"])
    assert rc == 0 and total == len(tm.tracts(buf, [0, 1000])) >= 1
    with pytest.raises(_lib.TredGpuError, match="max_gap \\+ 2 p - 2"):
        ctx.scan_tracts(buf, [0, 1000], max_gap=(1, 2, 5, 4, 5, 6))
    with pytest.raises(ValueError):
        ctx.scan_tracts(buf, [0, 1001])
    assert ctx.scan_tracts(b"", [0])[6] == 0 and ctx.scan_tracts(b"", [0, 0, 0])[6] == 0
    assert ctx.scan_tracts(as_buf("ACGTTGCATGCA"), [0, 12])[6] == 0       # (letters, and no seed)


def test_timing_counts_the_calls(ctx):
    buf = as_buf("TT" + tm.FMR1 + "TT" + "ACGTTGCA" * 1100)
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_TRACT) == (0, 0.0)
    for _ in range(3):
        ctx.scan_tracts(buf, [0, len(buf)])
    n, ms = ctx.get_timing(_lib.KERNEL_TRACT)
    assert n == 3 and ms > 0.0 and ctx.get_timing(_lib.KERNEL_SCAN) == (0, 0.0)
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_TRACT) == (0, 0.0)


def test_release_is_idempotent(ctx):
    buf = as_buf("TT" + tm.FMR1 + "TT" + tm.SCA1)
    want = tm.tracts(buf, [0, len(buf)])
    assert (0, 2, 90, 3, 3, 2) in want and gpu_tracts(ctx, buf, [0, len(buf)]) == want
    ctx.lib.tredtract_release(ctx.h)
    ctx.lib.tredtract_release(ctx.h)
    assert gpu_tracts(ctx, buf, [0, len(buf)]) == want         # (the state is made again by the next call)
    ctx.lib.tredtract_release(ctx.h)


def test_more_tiles_than_the_table_scans_take_in_one_batch(ctx):
    """4 201 tiles: each of the 16 wavefronts of the scans over the tiles' tables has a stretch of 320 tiles, five steps
    of 64, more than one batch of loads -- the table of seed counts per tile and period, a workgroup a period, too.  Interrupted tracts inside a stretch and
    across the boundary of two, seeds of many tiles, a segment's end beside them.  (Periods 1 and 4 are off and the seeds are
    long: the model's time on 17 M letters.)"""
    mc, sc, mg = (0, 8, 6, 0, 4, 4), (0, 6, 5, 0, 4, 4), (0, 2, 3, 0, 5, 6)
    n = 4200 * T + 5
    buf = rand_letters(31, n)

    def put(at, text):
        buf[at:at + len(text)] = as_buf(text)
        buf[at - 1], buf[at + len(text)] = ord("T"), ord("T")
        return at

    a = put(320 * T - 40, "CAG" * 20 + "CTG" + "CAG" * 20)                 # the gap lies on the boundary of two stretches
    b = put(127 * T - 9, "AC" * T + "GC" + "AC" * T)
    c = put(2000 * T + 5, "AAGGC" * (26 * T) + "ATGGC" + "AAGGC" * 30)
    d = put(4198 * T - 30, "CAG" * 30 + "CAA" + "CAG" * (T // 3))
    for k, at in enumerate(range(20000, n - 5000, 250000)):
        if not any(s - 200 < at < e + 200 for s, e in ((a, a + 200), (b, b + 4 * T + 10), (c, c + 131 * T), (d, d + T + 200))):
            put(at, "CAG" * (6 + k % 5) + "CGG" + "CAG" * 7)
    cut = [0, 319 * T + 1, 2050 * T, 2050 * T, n]
    want = tm.tracts(buf, cut, mc, sc, mg)
    assert {(0, b, 4 * T + 2, 2, 2, 1), (1, a - 319 * T - 1, 123, 3, 2, 1), (3, d - 2050 * T, 93 + T // 3 * 3, 3, 2, 1)} <= set(want)
    assert any(r[0] == 3 and r[3] == 5 and r[4] == 2 and r[5] == 1 for r in want) and len(want) > 60
    assert gpu_tracts(ctx, buf, cut, mc, sc, mg) == want
