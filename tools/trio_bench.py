#!/usr/bin/env python3
"""Device time of the trio unit (tredtrio_evaluate, csrc/trio.hip) beside a numpy restatement of the model on one core.

N items, drawn with `seed`: each a (child, father, mother) of the golden HD grids (tests/golden/grid.npz; 1 to 5 460 pairs a
list), and one item in sixteen (at least one) of crafted --fullsearch size: 300 alleles, 45 150 pairs in every role, so
300 x 45 150 transmissions per parent.  get_timing's selector gives the device time (HIP events around the call's three
launches): the median of REPEATS calls after a warm-up, and their range; the wall time of the call includes staging and
read-back.  The clocks are read (rocm-smi, nothing is set) before and after.  The same items then go through numpy on one
core -- vectorised per item, the parent's pairs in blocks --, whose results must equal the kernel's within 1e-6.  Fixes no
target: one JSON line.

    python tools/trio_bench.py N seed [REPEATS]                       (on the GPU)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOOR = float(np.exp(-100.0))


def clocks():
    """What rocm-smi shows of the clocks right now (read only); None where the tool is missing."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=60).stdout
        card = sorted(json.loads(out).items())[0][1]
        return {k: v for k, v in card.items() if "sclk" in k or "mclk" in k or "fclk" in k}
    except Exception:
        return None


def median_range(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def transmission_table(cap, mu, rho, beta):
    """T(c | p) at c - p + cap, the steps by their recurrence."""
    table = np.zeros(2 * cap + 1)
    table[cap] = 1 - mu
    step = 1 - rho
    for d in range(1, cap + 1):
        table[cap + d], table[cap - d] = (mu * beta) * step, (mu * (1 - beta)) * step
        step = step * rho
    return table


def numpy_trio(child, father, mother, table, cap, mu, block=4096):
    """(index, Jmax, S, denovo, paternal, J) of one diploid item with both parents informative."""
    x, y, lw = child
    alleles, inv = np.unique(np.concatenate([x, y]), return_inverse=True)
    px, py = inv[:len(x)], inv[len(x):]
    g = []
    for a, b, plw in (father, mother):
        w = np.exp(plw)
        acc, acc0 = np.zeros(len(alleles)), np.zeros(len(alleles))
        for k in range(0, len(a), block):
            ak, bk, wk = a[k:k + block], b[k:k + block], w[k:k + block]
            da, db = alleles[:, None] - ak[None, :], alleles[:, None] - bk[None, :]
            acc += ((0.5 * table[da + cap] + 0.5 * table[db + cap]) * wk[None, :]).sum(axis=1)       # (no BLAS: one core)
            acc0 += ((0.5 * (1 - mu) * (da == 0) + 0.5 * (1 - mu) * (db == 0)) * wk[None, :]).sum(axis=1)
        g.append((acc / w.sum(), acc0 / w.sum()))
    (gF, g0F), (gM, g0M) = g
    het = x != y
    cross, cross0 = gF[py] * gM[px], g0F[py] * g0M[px]
    t = gF[px] * gM[py] + het * cross
    t0 = g0F[px] * g0M[py] + het * cross0
    pat = np.where(het, cross, 0.5 * t)
    J = lw + np.log(np.maximum(t, FLOOR))
    best = np.lexsort((np.arange(len(J)), x, -J))[0]
    w = np.exp(lw)
    A = (w * t).sum()
    return int(best), float(J[best]), float(np.exp(J - J[best]).sum()), float(1 - (w * t0).sum() / A), float((w * pat).sum() / A), J


def main():
    from tredparse_amd import _lib
    from tredparse_amd.trio import PairList, pack_members
    n_items, seed = int(sys.argv[1]), int(sys.argv[2])
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 15
    rng = np.random.default_rng(seed)
    with open(os.path.join(ROOT, "tests", "golden", "grid.json")) as fp:
        cases = json.load(fp)["cases"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "grid.npz"))
    golden = [PairList.from_grid(z["mls_%d" % i], 3) for i, c in enumerate(cases)
              if c["locus"] == "HD" and c["ploidy"] == 2 and "mls_%d" % i in z.files and len(z["mls_%d" % i])]

    def fullsearch():
        ia, ib = np.triu_indices(300)
        lw = -rng.random(len(ia)) * 30
        lw[rng.integers(len(lw))] = 0.0
        return PairList(ia + 1, ib + 1, lw)

    n_full = max(1, n_items // 16)
    members = [[fullsearch() if i < n_full else golden[rng.integers(len(golden))] for i in range(n_items)] for _ in range(3)]
    (child, _), (father, f_inf), (mother, m_inf) = (pack_members(m) for m in members)
    ploidy = np.full(n_items, 2, np.int32)
    status, call, values = np.zeros(n_items, np.int32), np.zeros((n_items, 3), np.int32), np.zeros((n_items, 4))
    J = np.zeros(int(child[0][-1]))
    mu, rho, beta = _lib.TRIO_MU, _lib.TRIO_RHO, _lib.TRIO_BETA
    before = clocks()
    ctx = _lib.Context(0)

    def evaluate():
        ctx.trio(n_items, child, father, mother, ploidy, f_inf, m_inf, status, call, values, J, mu=mu, rho=rho, beta=beta)

    def timed():
        ctx.reset_timing()
        t0 = time.perf_counter()
        evaluate()
        return ctx.get_timing(_lib.KERNEL_TRIO)[1], (time.perf_counter() - t0) * 1e3

    evaluate()
    assert not (status != _lib.TRIO_OK).any(), "an item was refused or degenerate"
    runs = [timed() for _ in range(repeats)]
    after = clocks()
    ctx.close()

    table = transmission_table(_lib.TRIO_MAX_ALLELE, mu, rho, beta)
    t0 = time.perf_counter()
    model = [numpy_trio(*((m[i].a.astype(np.int64), m[i].b.astype(np.int64), m[i].lw) for m in members), table,
                        _lib.TRIO_MAX_ALLELE, mu) for i in range(n_items)]
    numpy_ms = (time.perf_counter() - t0) * 1e3
    worst = {"J": 0.0, "Jmax": 0.0, "log S": 0.0, "denovo": 0.0, "paternal": 0.0}
    for i, (best, Jmax, S, denovo, paternal, Jm) in enumerate(model):
        assert best == call[i, 0], "the numpy model and the kernel call item {} differently".format(i)
        got = {"J": np.abs(J[child[0][i]:child[0][i + 1]] - Jm).max(), "Jmax": abs(values[i, 0] - Jmax),
               "log S": abs(np.log(values[i, 1]) - np.log(S)), "denovo": abs(values[i, 2] - denovo), "paternal": abs(values[i, 3] - paternal)}
        worst = {k: max(worst[k], float(got[k])) for k in worst}
    assert max(worst.values()) <= 1e-6, "the numpy model and the kernel disagree: {}".format(worst)
    alleles = [len(np.unique(np.concatenate([m.a, m.b]))) for m in members[0]]
    work = sum(a * (len(f) + len(m)) for a, f, m in zip(alleles, members[1], members[2]))
    dev, wall = median_range([r[0] for r in runs]), median_range([r[1] for r in runs])
    print(json.dumps({"tool": "tools/trio_bench.py", "items": n_items, "seed": seed, "fullsearch_items": n_full,
                      "child_pairs": int(child[0][-1]), "parent_pairs": int(father[0][-1] + mother[0][-1]),
                      "transmissions": int(work), "repeats": repeats, "device_ms": dev, "call_wall_ms": wall,
                      "numpy_one_core_ms": numpy_ms, "numpy_over_device": numpy_ms / dev["median"],
                      "transmissions_per_s_device": work / (dev["median"] * 1e-3), "largest_difference": worst,
                      "version": _lib.version(), "clocks_before": before, "clocks_after": after}))


if __name__ == "__main__":
    main()
