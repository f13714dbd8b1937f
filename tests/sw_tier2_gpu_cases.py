"""The batches of tests/test_sw_exit_tier2_gpu.py: the nine cases of tests/sw_exit_gpu_cases.py and four more that look at
the second tier's table (SwArgs::read_tail), each a list of quads of four reads, run as sw_exit_gpu_cases.run_case runs them.

    pad131    131-base reads in the 10-row kernel: the last two lanes hold padding rows only, lane 13 one read row -- their
              tail counts are 0
    subs150   FULL reads with 1, 3 and 8 substitutions inside the repeat beside the clean read: absent windows in the tail
    ntail150  reads with Ns in their last 30 bases: windows with an N count as present
    opmd100   the N ladder at 100 bp (the 7-row kernel)

Run as a program it prints, as one JSON line, every case's results and trunk-column counter from the library TREDGPU_LIB
names: the test starts it once with the library that holds the first tier only (libtredgpu_tier1.so).

    python -m tests.sw_tier2_gpu_cases
"""
import json
import sys

import numpy as np

from oracle import pyoracle as po

from . import sw_exit_gpu_cases as cs

# name: (ladder, read length of the call, scoring, clip)
MORE = {
    "pad131": (cs.HD, 150, cs.DEFAULT, 0),
    "subs150": (cs.HD, 150, cs.DEFAULT, 0),
    "ntail150": (cs.HD, 150, cs.DEFAULT, 0),
    "opmd100": (cs.OPMD, 100, cs.DEFAULT, 0),
}
CASES = dict(cs.CASES, **MORE)


def _kinds(rng, lad, L):
    """FULL reads with right flanks of 0 / 10 / 40 / 100 bases (where the read has room), PREF, POST, REPT and the first FULL
    read reverse-complemented: eight reads of length L"""
    a, rep, b = lad
    p = len(rep)
    out = []
    for flank in (0, 10, 40, 100 if L >= 140 else 25):
        units = max(2, (L - flank - 30) // p)
        body = cs._junk(rng, 300) + cs._fill(rng, a + rep * units + b) + cs._junk(rng, 300)
        end = 300 + len(a) + p * units + flank
        out.append(body[end - L:end])
    units = L // p + 3
    hap = cs._junk(rng, L) + cs._fill(rng, a + rep * units + b) + cs._junk(rng, L)
    out.append(hap[L + len(a) - 30:][:L])
    out.append(hap[L + len(a) + p * units + len(b) + 12 - L:][:L])
    out.append(cs._fill(rng, rep * (L // p + 2))[1:L + 1])
    out.append(po.rc(out[0]))
    return out


def _sub_repeat(rng, read, lad, k):
    """k substitutions at positions inside the read's repeat stretch (behind the ladder's prefix, before its suffix)"""
    a, rep, b = lad
    lo = read.find(a[-8:]) + 8
    hi = read.find(b[:8], lo)
    hi = len(read) if hi < 0 else hi
    assert lo >= 8 and hi - lo >= 3 * k, (lo, hi, k)
    s = list(read)
    for i in rng.choice(np.arange(lo, hi), k, replace=False):
        s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def _n_tail(rng, read, k):
    """k Ns among the read's last 30 bases"""
    s = list(read)
    for i in rng.choice(np.arange(len(s) - 30, len(s)), k, replace=False):
        s[i] = "N"
    return "".join(s)


def quads_of(name):
    if name in cs.CASES:
        return cs.quads_of(name)
    lad, L, _, _ = MORE[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "pad131":
        k = _kinds(rng, lad, 131)
        return [k[0:4], k[4:8], [k[0], k[5], k[6], k[3]]]
    if name == "subs150":
        k = _kinds(rng, lad, L)
        quads = []
        for base in (k[0], k[1], k[2]):
            quads.append([base] + [_sub_repeat(rng, base, lad, n) for n in (1, 3, 8)])
        return quads
    if name == "ntail150":
        k = _kinds(rng, lad, L)
        return [[_n_tail(rng, k[0], 3), _n_tail(rng, k[1], 6), k[2], _n_tail(rng, k[6], 10)],
                [_n_tail(rng, k[4], 4), k[5], _n_tail(rng, k[3], 12), _n_tail(rng, k[7], 5)]]
    k = _kinds(rng, lad, L)
    return [k[0:4], k[4:8], [k[0], k[5], k[6], cs._sub(rng, k[1], 3)]]


def ladders_of(name):
    lad, L, _, _ = CASES[name]
    return [(lad[0], lad[1], lad[2], -(-L // len(lad[1])))] * len(quads_of(name))


def run_case(ctx, name, dump=False):
    """-> (results [n, 3], trunk columns of the call, dump or None), as sw_exit_gpu_cases.run_case"""
    if name in cs.CASES:
        return cs.run_case(ctx, name, dump)
    import torch
    from tredparse_amd import _lib
    lad, L, scoring, clip = MORE[name]
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
                    _lib.SwParams(scoring[0], scoring[1], scoring[2], scoring[3], cs.FLANK, clip, L, 0), tag, h, sc, dmp, nt)
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
    print("SW_TIER2_CASES " + json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
