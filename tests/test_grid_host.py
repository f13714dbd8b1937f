"""CPU: tredparse_amd/csrc/grid_host.h, the slot layout and the workspace plan of the likelihood grid, through the stand-alone
driver tests/grid_host_main.cpp built with the address and undefined-behaviour sanitizers: the offsets of a unit's tables,
the bound on a slot (the layout at the worst admissible arguments: it dominates every layout a unit can get and stays below
the closed form it replaces), the work items of a unit, and every size plan_grid hands the launcher and the C API.  The
expected values are written out here, from the rules the kernels and the C API used before the header existed."""
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MAXOBS, MAXM, TQ, CB, RG, RS, TC, MAX_ROWS = 256, 768, 16, 64, 128, 16, 32, 1024
OBS = (4 * MAXOBS + MAXOBS + 1 + 3) * 4 // 8          # an Obs in doubles: four lists of MAXOBS ints, base[MAXOBS + 1], three counts
# grid_prepare_kernel refuses a unit unless hmaxv / period < MAXM and 1 <= period < 18, and dmax = 2 * max(hmaxv - readlen, 1)
# with readlen >= 0
DMAX = 2 * (MAXM * 17 - 1)
DESC_BYTES, ITEM_BYTES, COUNTER_BYTES, SPAN = 216, 20, 64 * (6 * TQ + 1), 1000
GIB, MIB = 1 << 30, 1 << 20


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grid_host") / "grid_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "grid_host_main.cpp")])

    def call(*args):
        flat = []
        for a in args:
            flat += [str(x) for x in a] if isinstance(a, (list, tuple)) else [str(a)]
        r = subprocess.run([exe] + flat, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr        # the sanitizers report nothing
        return [[int(x) for x in line.split() if x != "|"] for line in r.stdout.splitlines()]
    return call


def layout(nrow, ncol, nt, run_pe, haploid, dmax, n_near):
    """unit_layout as grid_prepare_kernel had it: the tables one after the other, the end rounded up to 16 doubles"""
    sizes = [OBS, (nrow + 2) // 2, nrow, nrow, nrow * n_near, nrow * n_near, dmax + 1,
             nrow * ((nt + 31) // 32 * 32) if run_pe else 0, ncol * nt if run_pe and not haploid else 0, nrow * ncol]
    offs = [sum(sizes[:k]) for k in range(len(sizes))]
    return offs + [(sum(sizes) + 15) // 16 * 16]


def bound(rows, cols, nt_max):
    return layout(rows, cols, max(nt_max, 0), True, False, DMAX, cols)[-1]


def old_bound(rows, cols, nt_max):
    """grid_slot_doubles_max as it was written out by hand"""
    nt = max(nt_max, 0)
    return OBS + rows * 3 + 2 + 2 * 18 * MAXM + 2 + rows * ((nt + 31) // 32 * 32) + cols * nt + 3 * rows * cols + 16


def items(nrow, ncol):
    return 1 if nrow <= RS else -(-ncol // CB) * -(-nrow // RG)


def test_constants(run):
    assert OBS == 642
    assert run("K") == [[MAXOBS, MAXM, TQ, CB, RG, RS, TC, MAX_ROWS, DMAX, OBS, DESC_BYTES, ITEM_BYTES, COUNTER_BYTES]]


@pytest.mark.parametrize("args,want", [
    # haploid, no paired-end term: no near, no roll tables -- 642 | 11 | 20 | 20 | 0 | 0 | 3 | 0 | 0 | 20 = 716 -> 720
    ((20, 1, 7, 0, 1, 2, 0), [0, 642, 653, 673, 693, 693, 693, 696, 696, 696, 720]),
    # diploid with the paired-end term, 37 spanning pairs: roll1 rows of 64, roll2 columns of 37
    # 642 | 21 | 40 | 40 | 200 | 200 | 301 | 40 * 64 | 50 * 37 | 2000 = 7854 -> 7856
    ((40, 50, 37, 1, 0, 300, 5), [0, 642, 663, 703, 743, 943, 1143, 1444, 4004, 5854, 7856]),
    # haploid with the paired-end term: roll1 only -- 642 | 3 | 5 | 5 | 0 | 0 | 11 | 5 * 32 | 0 | 5 = 831 -> 832
    ((5, 1, 32, 1, 1, 10, 0), [0, 642, 645, 650, 655, 655, 655, 666, 826, 826, 832]),
    # a short grid (nrow = RS), every column near -- 642 | 9 | 16 | 16 | 1120 | 1120 | 3 | 0 | 0 | 1120 = 4046 -> 4048
    ((16, 70, 0, 0, 0, 2, 70), [0, 642, 651, 667, 683, 1803, 2923, 2926, 2926, 2926, 4048]),
    # the caps: 642 | 513 | 1024 | 1024 | 2^20 | 2^20 | 26111 | 1024 * 1024 | 1024 * 1000 | 2^20 = 5247618 -> 5247632
    ((1024, 1024, 1000, 1, 0, DMAX, 1024), [0, 642, 1155, 2179, 3203, 1051779, 2100355, 2126466, 3175042, 4199042, 5247632]),
])
def test_layout_offsets(run, args, want):
    assert run("L", args) == [want] and want == layout(*args) and want[-1] % 16 == 0


def test_bound_dominates_every_layout(run):
    """every combination the issue names, none skipped: the layout is at most the bound at its own rows, columns and n_target
    (hence at every larger cap and nt_max: the bound grows with each), and at most the bound at the largest of them"""
    cap, nts = MAX_ROWS, (0, 5, 31, 32, 33, 1000)
    sizes = (1, 8, RS, RS + 1, 64, 65, 128, 129, cap)
    combos = [(r, c, nt, pe, hap, dmax, nn) for r, c, nt, pe, hap, dmax in itertools.product(sizes, sizes, nts, (0, 1), (0, 1), (2, DMAX))
              for nn in (0, 1, c)]
    assert len(combos) == 9 * 9 * 6 * 2 * 2 * 2 * 3
    bounds = {}
    for (r, c, nt), b in zip(itertools.product(sizes, sizes, nts), run(*[("M", r, c, nt) for r, c, nt in itertools.product(sizes, sizes, nts)])):
        assert b == [bound(r, c, nt)]
        bounds[r, c, nt] = b[0]
    top = bounds[cap, cap, 1000]
    got = []
    for k in range(0, len(combos), 2000):                             # (a command line holds 2 000 records comfortably)
        got += run(*[("L",) + x for x in combos[k:k + 2000]])
    assert len(got) == len(combos)
    for x, L in zip(combos, got):
        assert L == layout(*x), x
        assert L[-1] <= bounds[x[0], x[1], x[2]] <= top, x


def test_bound_does_not_exceed_the_old_closed_form(run):
    sizes, nts = (1, 8, RS, RS + 1, 64, 65, 128, 129, 365, MAX_ROWS), (-3, 0, 5, 31, 32, 33, 1000, 3000000)
    for r, c, nt in itertools.product(sizes, sizes, nts):
        b = run("M", r, c, nt)[0][0]
        assert b == bound(r, c, nt) <= old_bound(r, c, nt)
        # what the hand sum carried beyond it: the row-offset line counted as a full line of doubles, the repeat-only table at
        # 2 * 18 * MAXM + 2 entries where 2 * (17 * MAXM - 1) + 1 are the most, 16 doubles -- less the padding of the total
        pad = b - (layout(r, c, max(nt, 0), True, False, DMAX, c)[9] + r * c)
        assert 0 <= pad < 16 and old_bound(r, c, nt) - b == r - (r + 2) // 2 + 1557 - pad
    # the bench batch's cap (hist_stride 64, maxinsert 300): 1 739 doubles less the padding of the total to 16
    assert old_bound(365, 365, 40) - bound(365, 365, 40) == 365 - 183 + 1557 - 11 == 1728


def plan(n_units, hist_stride, max_insert, max_target, limit):
    """the arithmetic of run_grid_device and launch_grid_pass, over the bound above"""
    cap = min(max(hist_stride + 1 + max(max_insert, 0), 8), MAX_ROWS)
    slot = bound(cap, cap, max_target)
    room = (slot + 16) * 8
    per_queue = -(-n_units // 16)
    all_bytes = 16 * per_queue * room
    pool_bytes = max(min(all_bytes, limit), room)
    pool_doubles = pool_bytes // 8
    n_sub = TQ
    while n_sub > 1 and pool_doubles // n_sub < slot + 16:
        n_sub >>= 1
    item_cap = TQ * per_queue * (-(-cap // CB) * -(-cap // RG))
    kde_pdf = n_units * SPAN * 8
    return [cap, slot, room, all_bytes, pool_bytes, int(all_bytes > pool_bytes), pool_doubles, n_sub, pool_doubles // n_sub // 16 * 16,
            item_cap, item_cap // TQ, (item_cap + 3) // 4 * 4,
            pool_bytes, n_units * DESC_BYTES, item_cap * ITEM_BYTES + 64, COUNTER_BYTES, kde_pdf + n_units * 4, kde_pdf]


PLANS = [
    # the bench batch: cap 365, slot 465 312 doubles, every sub-pool of the 12 GiB holds 216 slots
    ((30000, 64, 300, 40, 12 * GIB), dict(cap=365, slot=465312, pool_bytes=12 * GIB, may_defer=1, n_sub=16, item_region=1875 * 18)),
    ((180, 64, 300, 40, 12 * GIB), dict(cap=365, all_bytes=192 * 3722624, pool_bytes=192 * 3722624, may_defer=0, n_sub=16)),
    # 4 MiB: one slot of 3.55 MiB, one sub-pool
    ((30000, 64, 300, 40, 4 * MIB), dict(pool_bytes=4 * MIB, may_defer=1, n_sub=1, sub_doubles=524288)),
    ((180, 64, 300, 0, 64 * MIB), dict(slot=427344, pool_bytes=64 * MIB, may_defer=1, n_sub=16, sub_doubles=524288)),
    # smaller than one slot: the pool is one slot room
    ((30000, 64, 300, 40, 1 * MIB), dict(pool_bytes=3722624, may_defer=1, n_sub=1, sub_doubles=465328)),
    ((12, 64, 300, 40, 1 * MIB), dict(pool_bytes=3722624, may_defer=1, n_sub=1, item_region=18, item_cap=288)),
    # the residue classes of the units per queue
    ((1, 64, 300, 40, 12 * GIB), dict(all_bytes=16 * 3722624, may_defer=0, n_sub=16, item_region=18)),
    ((15, 64, 300, 40, 12 * GIB), dict(all_bytes=16 * 3722624, may_defer=0, item_region=18)),
    ((16, 64, 300, 40, 12 * GIB), dict(all_bytes=16 * 3722624, may_defer=0, item_region=18)),
    ((17, 64, 300, 40, 12 * GIB), dict(all_bytes=32 * 3722624, may_defer=0, item_region=36)),
    # the cap: clipped at GRID_MAX_ROWS, never below 8, a negative maxinsert counts as 0
    ((100, 800, 300, 1000, 12 * GIB), dict(cap=1024, slot=5247632, item_region=7 * 16 * 8)),
    ((100, 1, 0, 0, 12 * GIB), dict(cap=8, item_region=7)),
    ((100, 64, -5, 0, 12 * GIB), dict(cap=65, item_region=7 * 2)),
]
FIELDS = ["cap", "slot", "room", "all_bytes", "pool_bytes", "may_defer", "pool_doubles", "n_sub", "sub_doubles", "item_cap", "item_region",
          "item_best", "pool", "descs", "items", "counters", "kde", "kde_pdf"]


@pytest.mark.parametrize("args,want", PLANS)
def test_plan_grid(run, args, want):
    got = run("P", args)[0]
    assert got == plan(*args)
    p = dict(zip(FIELDS, got))
    for k, v in want.items():
        assert p[k] == v, (k, p[k], v)
    n_units = args[0]
    assert p["n_sub"] in (1, 2, 4, 8, 16) and p["sub_doubles"] % 16 == 0 and p["n_sub"] * p["sub_doubles"] <= p["pool_doubles"]
    assert p["sub_doubles"] >= p["slot"] + 16 and p["slot"] == bound(p["cap"], p["cap"], args[3])
    assert p["item_cap"] == TQ * p["item_region"] and p["item_region"] >= -(-n_units // TQ) * items(p["cap"], p["cap"])
    assert p["pool_bytes"] >= p["room"] == (p["slot"] + 16) * 8 and p["may_defer"] == int(p["all_bytes"] > p["pool_bytes"])
    assert p["item_best"] % 4 == 0 and p["item_cap"] <= p["item_best"] and p["items"] >= p["item_best"] * 4 + p["item_cap"] * 16
    assert p["n_sub"] == 16 or p["pool_doubles"] // (2 * p["n_sub"]) < p["slot"] + 16      # as many sub-pools as hold a slot each


@pytest.mark.parametrize("nrow,ncol,want", [
    (RS, 1024, 1), (RS + 1, 1024, 16), (RS + 1, CB, 1), (RS + 1, CB + 1, 2), (RG, CB, 1), (RG + 1, CB, 2), (RG + 1, CB + 1, 4),
    (1, 1, 1), (365, 365, 18), (1024, 1024, 128),
])
def test_unit_items(run, nrow, ncol, want):
    assert run("I", nrow, ncol) == [[want]] and items(nrow, ncol) == want
