"""tredscan_scan (include/tredscan.h, csrc/scan.hip) against the definition (tests/scan_model.py): runs at every edge of a
tile -- the letters one wavefront owns --, segments' ends, dense and random input, the cap, the refusals, timing, release."""
import ctypes as C

import numpy as np
import pytest

from tredparse_amd import _lib

from . import scan_model as sm

pytestmark = pytest.mark.gpu

T = _lib.SCAN_TILE
ALL2 = (2, 2, 2, 2, 2, 2)
MOTIFS = {1: "A", 2: "AC", 3: "CAG", 4: "GATA", 5: "AACCT", 6: "AAGGCT"}
SENTINEL = -77


def rand_letters(seed, n, alphabet="ACGT"):
    return np.frombuffer("".join(alphabet).encode(), np.uint8)[np.random.default_rng(seed).integers(0, len(alphabet), n)].copy()


def plant(buf, start, p, length):
    """A run of period p and exactly `length` letters at `start`, whatever the letters around it are."""
    motif = np.frombuffer(MOTIFS[p].encode(), np.uint8)
    buf[start:start + length] = np.resize(motif, length)
    others = lambda ch: next(x for x in b"ACGT" if x != ch)
    buf[start - 1] = others(buf[start - 1 + p])
    buf[start + length] = others(buf[start + length - p])
    return (start, length, p)


def gpu_records(ctx, buf, seg_off, min_copies=sm.MIN_COPIES, cap=1 << 16):
    seg, start, length, period, total = ctx.scan(buf, seg_off, min_copies, cap)
    assert total == len(seg)
    return list(zip(seg.tolist(), start.tolist(), length.tolist(), period.tolist()))


@pytest.fixture(scope="module")
def edges():
    """38 tiles of random letters with a run at every edge of the tiling: per period a run that starts at T - 1, T and T + 1
    of a tile boundary, one whose last e_p one is the letter before a boundary (the look-ahead of that letter is the first
    letters of the next tile) and one whose last one is the boundary's; a run of 3 T + 5 letters; an N on either side of a
    boundary inside a run.  Returns (letters, the planted (start, length, period))."""
    buf = rand_letters(11, 38 * T)
    planted, edge = [], 1
    for p in range(1, 7):
        for delta in (-1, 0, 1):
            planted.append(plant(buf, edge * T + delta, p, 12 * p + 1))
            edge += 1
        for last_one in (-1, 0):                        # the run is [i0, i1 + p) with its last one at i1 - 1
            end = edge * T + last_one + 1 + p
            planted.append(plant(buf, end - 14 * p, p, 14 * p))
            edge += 1
    planted.append(plant(buf, edge * T - 3, 3, 3 * T + 5))
    edge += 4
    a = plant(buf, edge * T - 60, 1, 120)                # an N is the last letter of a tile: two runs of 59 and 60
    buf[edge * T - 1] = ord("N")
    b = plant(buf, (edge + 1) * T - 40, 2, 100)          # an N is the first letter of a tile
    buf[(edge + 1) * T] = ord("n")
    assert edge + 2 <= 38
    return buf, planted, [a, b]


def test_tile_edges_one_segment(ctx, edges):
    buf, planted, _ = edges
    want = sm.scan(buf, [0, len(buf)])
    assert set((0,) + r for r in planted) <= set(want)                   # the runs are where the test means them to be
    assert gpu_records(ctx, buf, [0, len(buf)]) == want
    want2 = sm.scan(buf, [0, len(buf)], ALL2)
    assert gpu_records(ctx, buf, [0, len(buf)], ALL2, cap=len(buf)) == want2 and len(want2) > len(want)


def test_tile_edges_cut_into_segments(ctx, edges):
    """The same letters with segments' ends at and next to tile boundaries, in the middle of runs, with empty segments and
    segments of 1 .. 6 letters between them, and letters in front of the first segment that belong to none."""
    buf, planted, (a, b) = edges
    cuts = {5, len(buf)}
    for k, (start, length, p) in enumerate(planted):
        cuts.add(start + (length // 2 if k % 3 == 0 else p if k % 3 == 1 else length - 1))
    for edge in (1, 2, 3, 20, 21):
        cuts.update((edge * T - 1, edge * T, edge * T + 1))
    base = 7 * T + 100
    for p in range(0, 7):                                                # segments of 0, 1, .. 6 letters, twice each
        cuts.update((base, base + p))
        base += p
        cuts.update((base, base + p))
        base += p
    off = sorted(cuts)
    off = off[:3] + [off[2]] + off[3:] + [len(buf)]                      # (empty segments: in the middle and at the end)
    want = sm.scan(buf, off)
    assert gpu_records(ctx, buf, off) == want
    assert gpu_records(ctx, buf, off, ALL2, cap=len(buf)) == sm.scan(buf, off, ALL2)


def test_small_and_whole_run_segments(ctx):
    """Segments of 0, 1 and p letters for every p; a segment that is one run throughout, longer than two tiles; a run cut in
    two by a segment's end; a run that ends with its segment; all in one call, under the defaults and with every
    min_copies 2."""
    parts = [b"", b"A"] + [("ACGTAC"[:p]).encode() for p in range(1, 7)] + [("A" * p).encode() for p in range(1, 7)]
    parts += [b"CAG" * ((2 * T + 100) // 3), b"", b"GATA" * 10, b"GATA" * 10, b"TTTTTTTTTTTTTTTTTTTTTTTTTTTTTT", b"AC" * 3000 + b"A",
              rand_letters(5, 40).tobytes() + b"GATA" * 5, b"T"]
    buf = np.frombuffer(b"".join(parts), np.uint8)
    off = np.concatenate(([0], np.cumsum([len(x) for x in parts])))
    for mc in (sm.MIN_COPIES, ALL2):
        want = sm.scan(buf, off, mc)
        assert gpu_records(ctx, buf, off, mc) == want
    want = sm.scan(buf, off)
    whole = len(parts[14])
    assert (14, 0, whole, 3) in want and (16, 0, 40, 4) in want and (17, 0, 40, 4) in want and (19, 0, 6001, 2) in want


def test_one_run_over_the_whole_buffer(ctx):
    n = 5 * T + 17
    buf = np.full(n, ord("g"), np.uint8)
    assert gpu_records(ctx, buf, [0, n]) == [(0, 0, n, 1)]
    buf = np.resize(np.frombuffer(b"AAGGCT", np.uint8), n)
    assert gpu_records(ctx, buf, [0, n], ALL2) == sm.scan(buf, [0, n], ALL2)
    assert (0, 0, n, 6) in gpu_records(ctx, buf, [0, n])


def test_dense_two_letters(ctx):
    """20 000 letters over {A, C}, every min_copies 2: records at most letters: the cap given holds them all."""
    buf = rand_letters(21, 20000, "AC")
    want = sm.scan(buf, [0, len(buf)], ALL2)
    cap = 6 * len(buf)
    seg, start, length, period, total = ctx.scan(buf, [0, len(buf)], ALL2, cap)
    assert total == len(want) <= cap and total > 5000
    assert list(zip(seg.tolist(), start.tolist(), length.tolist(), period.tolist())) == want


def test_random_with_n(ctx):
    buf = rand_letters(22, 20000, "ACGTN")
    buf[3000:3100] = ord("A")
    buf[T - 20:T + 30] = np.resize(np.frombuffer(b"cAg", np.uint8), 50)
    want = sm.scan(buf, [0, 9000, len(buf)])
    assert len(want) >= 2 and gpu_records(ctx, buf, [0, 9000, len(buf)]) == want
    assert gpu_records(ctx, buf, [0, 9000, len(buf)], (3, 2, 2, 2, 2, 2), cap=40000) == sm.scan(buf, [0, 9000, len(buf)], (3, 2, 2, 2, 2, 2))


def raw_call(ctx, buf, off, mc, cap, room=None, letters_null=False, off_null=False, mc_null=False, out_null=False, n_null=False):
    """tredscan_scan itself on sentinel-filled outputs: (rc, the four arrays, out_n)."""
    room = max(cap, 1) if room is None else room
    outs = [np.full(room, SENTINEL, dt) for dt in (np.int32, np.int64, np.int32, np.int32)]
    off = np.asarray(off, np.int64)
    mc = np.asarray(mc, np.int32)
    total = C.c_int64(SENTINEL)
    ptr = lambda a, null: None if null else a.ctypes.data
    rc = ctx.lib.tredscan_scan(ctx.h, ptr(buf, letters_null), ptr(off, off_null), len(off) - 1, ptr(mc, mc_null), cap,
                               *[ptr(o, out_null) for o in outs], None if n_null else C.byref(total))
    return rc, outs, total.value


def test_cap_below_the_total(ctx, edges):
    buf = edges[0]
    want = sm.scan(buf, [0, len(buf)])
    for cap in (0, 1, len(want) // 2, len(want) - 1, len(want), len(want) + 5):
        rc, outs, total = raw_call(ctx, buf, [0, len(buf)], sm.MIN_COPIES, cap, room=len(want) + 10)
        assert rc == 0 and total == len(want)
        k = min(cap, len(want))
        for got, ref in zip(outs, sm.arrays(want)):
            assert np.array_equal(got[:k], ref[:k]) and (got[k:] == SENTINEL).all()


def test_period_switched_off(ctx, edges):
    buf = edges[0]
    for mc in ((0, 6, 5, 4, 4, 4), (10, 0, 5, 0, 4, 0), (0, 0, 0, 0, 0, 2)):
        assert gpu_records(ctx, buf, [0, len(buf)], mc, cap=len(buf)) == sm.scan(buf, [0, len(buf)], mc)


def test_two_calls_identical_bytes(ctx, edges):
    buf = edges[0]
    first = raw_call(ctx, buf, [0, 100, len(buf)], ALL2, len(buf))
    other = raw_call(ctx, rand_letters(3, 3 * T), [0, 3 * T], ALL2, 3 * T)           # (another call in between)
    second = raw_call(ctx, buf, [0, 100, len(buf)], ALL2, len(buf))
    assert first[0] == second[0] == other[0] == 0 and first[2] == second[2] > 0
    for x, y in zip(first[1], second[1]):
        assert x.tobytes() == y.tobytes()


def test_refusals_leave_outputs_untouched(ctx):
    buf = rand_letters(4, 1000)
    ok = dict(buf=buf, off=[0, 1000], mc=sm.MIN_COPIES, cap=16)
    cases = {
        "letters NULL": dict(letters_null=True), "seg_off NULL": dict(off_null=True), "min_copies NULL": dict(mc_null=True),
        "outputs NULL": dict(out_null=True), "out_n NULL": dict(n_null=True),
        "descending": dict(off=[0, 600, 500, 1000]), "negative": dict(off=[-1, 1000]),
        "min_copies 1": dict(mc=(10, 6, 1, 4, 4, 4)), "min_copies -1": dict(mc=(10, 6, 5, 4, -1, 4)), "all off": dict(mc=(0,) * 6),
        "cap negative": dict(cap=-1), "too many letters": dict(off=[0, _lib.SCAN_MAX_LETTERS + 1]),
    }
    for name, change in cases.items():
        args = dict(ok, **change)
        rc, outs, total = raw_call(ctx, args.pop("buf"), args.pop("off"), args.pop("mc"), args.pop("cap"), room=16, **args)
        assert rc == -2, name
        assert total == SENTINEL and all((o == SENTINEL).all() for o in outs), name
        assert ctx.lib.tredscan_last_error(), name
    rc, outs, total = raw_call(ctx, ok["buf"], ok["off"], ok["mc"], ok["cap"])
    assert rc == 0 and total == len(sm.scan(buf, [0, 1000]))
    with pytest.raises(_lib.TredGpuError, match="switched off"):
        ctx.scan(buf, [0, 1000], (0,) * 6)
    with pytest.raises(ValueError):
        ctx.scan(buf, [0, 1001])
    assert ctx.scan(b"", [0], sm.MIN_COPIES)[4] == 0 and ctx.scan(b"", [0, 0, 0], sm.MIN_COPIES)[4] == 0


def test_timing_counts_the_calls(ctx):
    buf = rand_letters(6, 2 * T + 3)
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_SCAN) == (0, 0.0)
    for _ in range(3):
        ctx.scan(buf, [0, len(buf)])
    n, ms = ctx.get_timing(_lib.KERNEL_SCAN)
    assert n == 3 and ms > 0.0
    ctx.reset_timing()
    assert ctx.get_timing(_lib.KERNEL_SCAN) == (0, 0.0)


def test_release_is_idempotent(ctx):
    buf = rand_letters(7, T + 9)
    buf[100:140] = ord("T")
    want = sm.scan(buf, [0, len(buf)])
    assert gpu_records(ctx, buf, [0, len(buf)]) == want
    ctx.lib.tredscan_release(ctx.h)
    ctx.lib.tredscan_release(ctx.h)
    assert gpu_records(ctx, buf, [0, len(buf)]) == want       # (the state is made again by the next call)
    ctx.lib.tredscan_release(ctx.h)


def test_more_tiles_than_the_table_scans_take_in_one_batch(ctx):
    """4 201 tiles: each of the 16 wavefronts of the two scans over the tiles' tables (csrc/scan.hip) has a stretch of 320
    tiles, five steps of 64, more than one batch of loads.  Runs inside a stretch, across the boundary of two stretches and
    across several steps, segments' ends beside them.  (Periods 1 and 4 are off: the model's time on 17 M letters.)"""
    mc = (0, 6, 5, 0, 4, 4)
    n = 4200 * T + 5
    buf = rand_letters(31, n)
    planted = [plant(buf, 300 * T - 7, 2, 5 * T), plant(buf, 127 * T - 1, 2, 2 * T + 3), plant(buf, 318 * T + 9, 6, 4 * T),
               plant(buf, 640 * T - 30, 3, T + 60), plant(buf, 2000 * T + 5, 5, 130 * T), plant(buf, 4199 * T - 30, 3, T + 30)]
    for k, at in enumerate(range(20000, n - 5000, 250000)):
        if not any(s - 100 < at < s + length + 100 for s, length, _ in planted):
            planted.append(plant(buf, at, (2, 3, 5, 6)[k % 4], 60 + k % 7))
    cut = [0, 319 * T + 1, 2050 * T, 2050 * T, n]
    want = sm.scan(buf, cut, mc)
    assert {(0, 300 * T - 7, 5 * T, 2), (0, 318 * T + 9, T - 8, 6), (1, 0, 3 * T + 8, 6), (1, 2000 * T + 5 - 319 * T - 1, 50 * T - 5, 5),
            (3, 0, 80 * T + 5, 5), (3, 4199 * T - 30 - 2050 * T, T + 30, 3)} <= set(want)       # (segment 2 is empty)
    assert gpu_records(ctx, buf, cut, mc) == want
