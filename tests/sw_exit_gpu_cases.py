"""The batches of tests/test_sw_exit_gpu.py and the one routine that runs them through tredgpu_sw_classify.

A case is a list of quads: four reads of four different kinds (so that one open read holds the others in the strand), each
quad registered as a ladder and a unit of its own -- whatever order the device packs a unit's reads in, a (ladder, level)
bin then holds at most those four reads, and the wavefronts are the ones tests/sw_exit_model.pack_quads forms.

Run as a program it prints, as one JSON line, every case's results and trunk-column counter from the library TREDGPU_LIB
names: the test starts it once with the library that has the bounded-gain exit compiled out.

    python -m tests.sw_exit_gpu_cases
"""
import json
import sys

import numpy as np

from oracle import pyoracle as po

HD = ("GAGTCCCTCAAGTCCTTC", "CAG", "CAACAGCCGCCACCGCCG")
OPMD = ("CCAGTCTGAGCGGCGATG", "GCN", "GGGGCTGCGGGCGGTCGG")
SCA10 = ("TGGTTCATCGAGTTTCCA", "ATTCT", "GGCATTAGCCGTTCAAGG")
LONGB = ("GAGTCCCTCAAGTCCTTC", "CAG", "CAACAGCCGCCACCGCCGTTAGACCTGAATCGTCAAGGA")      # a 39-base branch: the GENERIC kernel
DEFAULT = (1, 5, 7, 2)
LOOSE = (1, 4, 6, 1)        # mismatch < 5 * match: outside the 6-mer premise; match 1 keeps the production kernel

# name: (ladder, read length, scoring, clip)
CASES = {
    "hd150": (HD, 150, DEFAULT, 0),
    "hd100": (HD, 100, DEFAULT, 0),
    "hd250": (HD, 250, DEFAULT, 0),
    "opmd150": (OPMD, 150, DEFAULT, 0),
    "sca10_150": (SCA10, 150, DEFAULT, 0),
    "longb150": (LONGB, 150, DEFAULT, 0),
    "clip150": (HD, 150, DEFAULT, 1),
    "loose150": (HD, 150, LOOSE, 0),
    "inside150": (HD, 150, DEFAULT, 0),     # reads inside the repeat and random ones: no wave has an old alignment to wait for
}
FLANK = 9


def _junk(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _fill(rng, s):
    return "".join("ACGT"[int(rng.integers(0, 4))] if c == "N" else c for c in s)


def _sub(rng, s, k):
    s = list(s)
    for i in rng.choice(len(s), k, replace=False):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def quads_of(name):
    """[[four reads]] of one case: FULL reads with right flanks of 0 / 10 / 40 / 100 bases, PREF, POST, REPT, mutated and
    reverse-complemented ones, dealt so that every quad holds four different kinds."""
    lad, L, _, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    a, rep, b = lad
    p = len(rep)
    if name.startswith("inside"):
        rept = [_fill(rng, rep * (L // p + 2))[k:L + k] for k in range(3)]
        return [[rept[0], rept[1], rept[2], _junk(rng, L)], [rept[1], _junk(rng, L), _junk(rng, L), po.rc(rept[0])]]
    kinds = []
    for flank in (0, 10, 40, 100):
        units = max(2, (L - flank - 30) // p)
        body = _junk(rng, 300) + _fill(rng, a + rep * units + b) + _junk(rng, 300)
        end = 300 + len(a) + p * units + flank
        kinds.append(body[end - L:end])
    units = L // p + 3
    hap = _junk(rng, L) + _fill(rng, a + rep * units + b) + _junk(rng, L)
    kinds.append(hap[L + len(a) - 30:][:L])                                        # PREF
    kinds.append(hap[L + len(a) + p * units + len(b) + 12 - L:][:L])               # POST
    kinds.append(_fill(rng, rep * (L // p + 2))[1:L + 1])                          # REPT
    kinds.append(_sub(rng, kinds[2], 2))
    q = int(rng.integers(20, L - 20))
    kinds.append(kinds[1][:q] + kinds[1][q + 1:] + "A")                            # a deletion
    kinds.append(po.rc(kinds[0]))
    kinds.append(po.rc(kinds[4]))
    kinds.append(_sub(rng, kinds[4], 3))
    return [kinds[0:4], kinds[4:8], kinds[8:12], [kinds[0], kinds[5], kinds[6], kinds[9]]]


def ladders_of(name):
    lad, L, _, _ = CASES[name]
    return [(lad[0], lad[1], lad[2], -(-L // len(lad[1])))] * len(quads_of(name))


def run_case(ctx, name, dump=False):
    """-> (results [n, 3], trunk columns of the call, dump or None)"""
    import torch
    from tredparse_amd import _lib
    lad, L, scoring, clip = CASES[name]
    quads = quads_of(name)
    reads = [r for q in quads for r in q]
    n = len(reads)
    ladders = ladders_of(name)
    ctx.set_ladders(ladders)
    dev = torch.device("cuda", 0)
    packed, woff, rlen = _lib.pack_reads(reads)
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    uro = np.arange(0, n + 1, 4, dtype=np.int32)
    ul = np.arange(len(quads), dtype=np.int32)
    nt = 2 * ladders[0][3] if dump else 0
    tag = torch.zeros(n, dtype=torch.uint8, device=dev); h = torch.zeros(n, dtype=torch.int16, device=dev)
    sc = torch.zeros(n, dtype=torch.int16, device=dev)
    dmp = torch.zeros((n, nt, 6), dtype=torch.int16, device=dev) if dump else None
    torch.cuda.synchronize()
    ctx.reset_timing()
    ctx.sw_classify(_lib.MEM_DEVICE, dv(packed.view(np.int32)), dv(woff), dv(rlen), n, dv(uro), dv(ul), len(ul),
                    _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], FLANK, clip, L, 0), tag, h, sc, dmp, nt)
    ctx.sync()
    cols = ctx.get_sw_counters()["trunk_cols"]
    res = np.stack([tag.cpu().numpy(), h.cpu().numpy(), sc.cpu().numpy()], 1).astype(np.int64)
    return res, int(cols), dmp.cpu().numpy() if dump else None


def main():
    import torch          # before the library: PyTorch-ROCm ships its own HIP runtime (tests/conftest.py)
    torch.cuda.init()
    from tredparse_amd import _lib
    ctx = _lib.Context(0)
    out = {"lib": _lib.LIB_PATH}
    for name in CASES:
        res, cols, _ = run_case(ctx, name)
        out[name] = {"res": res.tolist(), "trunk_cols": cols}
    ctx.close()
    print("SW_EXIT_CASES " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
