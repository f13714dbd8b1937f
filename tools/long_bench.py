"""Time the long-read kernel (tredlong_sw_classify): 256 reads per length against a period-3 (HD) ladder of ceil(L/3)
units, three calls each; prints the call's wall time.  Run under `rocprofv3 --kernel-trace --stats -- python
tools/long_bench.py` for the kernel's own time (sw_long_kernel<16> for 513-1 024 bp, <32> for 1 025-2 048 bp)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
try:
    import torch               # (torch's HIP runtime first, as in the tests)
    torch.cuda.init()
except Exception:
    pass
from tredparse_amd import _lib, synth


def main(lengths=(600, 1000, 2048), n=256):
    hd = [l for l in synth.load_loci() if l["name"] == "HD"][0]
    ctx = _lib.Context(0)
    ctx.set_long_reads(True)
    rng = np.random.default_rng(1)
    rand = lambda k: "".join("ACGT"[i] for i in rng.integers(0, 4, k))
    for L in lengths:
        mu = -(-L // 3)
        lad = (hd["prefix"], "CAG", hd["suffix"], mu)
        g = rand(L) + hd["prefix"] + "CAG" * (mu // 2) + hd["suffix"] + rand(L)
        reads = [g[s:s + L] for s in rng.integers(0, len(g) - L, n)]
        ctx.set_ladders([lad])
        packed, woff, rlen = _lib.pack_reads(reads)
        tag = np.zeros(n, np.uint8); h = np.zeros(n, np.int16); sc = np.zeros(n, np.int16)
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.sw_classify(_lib.MEM_HOST, packed, woff, rlen, n, np.array([0, n], np.int32), np.array([0], np.int32), 1,
                            _lib.default_sw_params(), tag, h, sc, None, 0)
            dt = time.perf_counter() - t0
        print("L={} units={} reads={} call {:.1f} ms -> {:.0f} reads/s".format(L, mu, n, dt * 1e3, n / dt), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
