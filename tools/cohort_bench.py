#!/usr/bin/env python3
"""Device time of the cohort unit (tredcohort_evaluate, csrc/cohort.hip) beside a numpy restatement of the model on one core.

N_LOCI items of N_SAMPLES samples each, drawn with `seed`: the samples are the non-empty golden HD lists
(tests/golden/grid.npz; 1 to 5 460 pairs a list, hd_haploid at ploidy 1), and one sample in sixteen (at least one per locus)
is of crafted --fullsearch size: 300 alleles, 45 150 pairs.  get_timing's selector gives the device time (HIP events around
the call's launches -- 3 per iteration): the median of REPEATS calls after a warm-up, and their range; the wall time of the
call includes the host's incidence list, staging and read-back.  The clocks are read (rocm-smi, nothing is set) before and
after.  The same items then go through numpy on one core -- vectorised over all pairs of a locus, np.add.reduceat per sample,
np.bincount per allele --, whose frequencies, counts and posteriors must equal the kernel's within 1e-6.  With --numpy-loci K
only the first K loci go through numpy (the model needs minutes at the headline size) and the time is reported for those.
Fixes no target: one JSON line.

    python tools/cohort_bench.py N_SAMPLES N_LOCI [seed] [REPEATS] [--numpy-loci K] [--iters I]       (on the GPU)

--chunk N only labels the line: the chunk is a constant of the build (make EXTRA=-DTREDGPU_COHORT_CHUNK=N, loaded through
TREDGPU_LIB).
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def numpy_cohort(off, a, b, lw, ploidy, iters, alpha):
    """(alleles, f, n of the final E-step, r) of one locus whose samples all take part: off [n_samples + 1] into a, b, lw."""
    alleles, inv = np.unique(np.concatenate([a, b]), return_inverse=True)
    ia, ib = inv[:len(a)], inv[len(a):]
    A, C = len(alleles), float(ploidy.sum())
    start, size = off[:-1], np.diff(off)
    m = np.maximum.reduceat(lw, start)
    diploid = np.repeat(ploidy == 2, size)
    w = np.exp(lw - np.repeat(m, size)) * np.where(diploid & (ia != ib), 2.0, 1.0)
    second = diploid.astype(np.float64)                              # a ploidy-1 pair counts once
    f = np.full(A, 1.0 / A)
    for t in range(iters + 1):
        q = w * f[ia] * np.where(diploid, f[ib], 1.0)
        r = q / np.repeat(np.add.reduceat(q, start), size)
        n = np.bincount(ia, r, A) + np.bincount(ib, r * second, A)
        if t < iters:
            f = (n + alpha / A) / (C + alpha)
    return alleles, f, n, r


def main():
    from tredparse_amd import _lib
    from tredparse_amd.cohort import cohort_outputs, pack_cohort
    from tredparse_amd.trio import PairList
    argv = sys.argv[1:]
    opt = {"--numpy-loci": None, "--iters": _lib.COHORT_ITERS, "--chunk": _lib.COHORT_CHUNK}
    for name in list(opt):
        if name in argv:
            k = argv.index(name)
            opt[name] = int(argv[k + 1])
            del argv[k:k + 2]
    n_samples, n_loci = int(argv[0]), int(argv[1])
    seed = int(argv[2]) if len(argv) > 2 else 1
    repeats = int(argv[3]) if len(argv) > 3 else 15
    iters, alpha = opt["--iters"], _lib.COHORT_ALPHA
    numpy_loci = n_loci if opt["--numpy-loci"] is None else min(n_loci, opt["--numpy-loci"])
    rng = np.random.default_rng(seed)
    with open(os.path.join(ROOT, "tests", "golden", "grid.json")) as fp:
        cases = json.load(fp)["cases"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "grid.npz"))
    golden = [(PairList.from_grid(z["mls_%d" % i], 3), int(c["ploidy"])) for i, c in enumerate(cases)
              if c["locus"] == "HD" and "mls_%d" % i in z.files and len(z["mls_%d" % i])]

    def fullsearch():
        ia, ib = np.triu_indices(300)
        lw = -rng.random(len(ia)) * 30
        lw[rng.integers(len(lw))] = 0.0
        return PairList(ia + 1, ib + 1, lw), 2

    n_full = max(1, n_samples // 16)
    lists, ploidies = [], []
    for _ in range(n_loci):
        full = [fullsearch() for _ in range(min(n_full, 4))]        # (a few distinct ones per locus, drawn again and again)
        picks = [full[i % len(full)] if i < n_full else golden[rng.integers(len(golden))] for i in range(n_samples)]
        lists.append([p[0] for p in picks])
        ploidies.append([p[1] for p in picks])
    t0 = time.perf_counter()
    item_off, samples, ploidy, allele_off, _ = pack_cohort(lists, ploidies)
    pack_ms = (time.perf_counter() - t0) * 1e3
    n_pairs = int(samples[0][-1])
    out = cohort_outputs(n_loci, n_loci * n_samples, n_pairs, int(allele_off[-1]), iters)
    before = clocks()
    ctx = _lib.Context(0)

    def evaluate():
        ctx.cohort(n_loci, item_off, samples, ploidy, allele_off, *out, iters=iters, alpha=alpha)

    def timed():
        ctx.reset_timing()
        t0 = time.perf_counter()
        evaluate()
        return ctx.get_timing(_lib.KERNEL_COHORT)[1], (time.perf_counter() - t0) * 1e3

    print("{} pairs packed in {:.0f} ms".format(n_pairs, pack_ms), file=sys.stderr, flush=True)
    evaluate()
    print("warm-up done", file=sys.stderr, flush=True)
    status, n_alleles, alleles, freq, count, trace, call, values, r = out
    assert not (status != _lib.COHORT_OK).any(), "an item was refused or empty"
    runs = [timed() for _ in range(repeats)]
    after = clocks()
    ctx.close()
    print("{} timed calls done".format(repeats), file=sys.stderr, flush=True)

    off = samples[0]
    worst = {"f": 0.0, "count": 0.0, "r": 0.0}
    t0 = time.perf_counter()
    model = []
    for i in range(numpy_loci):
        lo, hi = int(item_off[i]), int(item_off[i + 1])
        p0, p1 = int(off[lo]), int(off[hi])
        model.append(numpy_cohort(off[lo:hi + 1] - p0, samples[1][p0:p1].astype(np.int64), samples[2][p0:p1].astype(np.int64),
                                  samples[3][p0:p1], ploidy[lo:hi], iters, alpha))
    numpy_ms = (time.perf_counter() - t0) * 1e3
    for i, (al, f, n, rr) in enumerate(model):
        j0, p0 = int(allele_off[i]), int(off[item_off[i]])
        assert n_alleles[i] == len(al) and np.array_equal(alleles[j0:j0 + len(al)], al), "the support of locus {} differs".format(i)
        got = {"f": np.abs(freq[j0:j0 + len(al)] - f).max(), "count": np.abs(count[j0:j0 + len(al)] - n).max(),
               "r": np.abs(r[p0:p0 + len(rr)] - rr).max()}
        worst = {k: max(worst[k], float(got[k])) for k in worst}
    assert max(worst.values()) <= 1e-6, "the numpy model and the kernel disagree: {}".format(worst)
    visits = n_pairs * (iters + 1)
    dev, wall = median_range([x[0] for x in runs]), median_range([x[1] for x in runs])
    numpy_pairs = int(off[item_off[numpy_loci]])
    numpy_all_ms = numpy_ms * n_pairs / max(1, numpy_pairs)
    print(json.dumps({"tool": "tools/cohort_bench.py", "samples": n_samples, "loci": n_loci, "seed": seed, "iters": iters,
                      "fullsearch_samples_per_locus": n_full, "pairs": n_pairs, "pair_visits": visits, "chunk": opt["--chunk"],
                      "repeats": repeats, "device_ms": dev, "call_wall_ms": wall, "pack_ms": pack_ms,
                      "numpy_loci": numpy_loci, "numpy_one_core_ms": numpy_ms, "numpy_one_core_ms_scaled_to_all_pairs": numpy_all_ms,
                      "numpy_over_device": numpy_all_ms / dev["median"], "pair_visits_per_s_device": visits / (dev["median"] * 1e-3),
                      "largest_difference": worst, "version": _lib.version(), "clocks_before": before, "clocks_after": after}))


if __name__ == "__main__":
    main()
