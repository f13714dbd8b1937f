#!/usr/bin/env python3
"""tests/golden/engine_units.json: what the Engine's Unit-list entry points (classify, genotype, winners, alignments,
consensus, grid_from_counts) give on a handful of small unit lists, recorded on an MI355X.

Only the public Unit-list API is used, so the same script runs on any commit that has it:
tests/test_engine_units_gpu.py calls record() and compares with the file this script wrote at the commit before the
Unit lists became PackedUnits.  Floats are recorded as float.hex(): the comparison is bit for bit.

    python tools/gen_golden_engine_units.py [out.json]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tredparse_amd import _lib, synth                                     # noqa: E402
from tredparse_amd.bam_parser import rc                                   # noqa: E402
from tredparse_amd.engine import Engine, Unit                             # noqa: E402
from tredparse_amd.meta import TREDsRepo                                  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "engine_units.json")
FLANK = 200
ODD_READ = "odd"         # the key under which record() keeps the text of the read with a lower-case and an IUPAC letter


# ---- the unit lists -----------------------------------------------------------------------------------------------------
def _genome(t, a, seed):
    """FLANK random letters + prefix + repeat * a + suffix + FLANK random letters."""
    rng = np.random.default_rng(seed)
    left, right = (synth.decode(rng.integers(0, 4, FLANK)) for _ in range(2))
    return left + t.prefix + t.repeat * a + t.suffix + right


def _cut(G, starts, n=150, strands="+"):
    """The n letters of G from FLANK + s for every s of starts; strand k % len(strands) of read k ('-': reverse complement)."""
    out = []
    for k, s in enumerate(starts):
        r = G[FLANK + s:FLANK + s + n]
        assert len(r) == n
        out.append(rc(r) if strands[k % len(strands)] == "-" else r)
    return out


def _edit(read, **at):
    """read with the letter at position int(key[1:]) replaced by the value (keys p<position>)."""
    s = list(read)
    for k, v in at.items():
        s[int(k[1:])] = v
    return "".join(s)


def _lens(seed, n, mean):
    return [int(x) for x in np.random.default_rng(seed).normal(mean, 60, n).astype(np.int64).clip(160, 900)]


def unit_lists():
    """{case: (long_reads, [Unit])} and the text of the odd read."""
    repo = TREDsRepo(ref="hg38")
    hd, sca10, dm1 = repo["HD"], repo["SCA10"], repo["DM1"]
    assert (len(hd.repeat), len(sca10.repeat)) == (3, 5)
    g15, g17, g20, g41, g60 = (_genome(hd, a, 100 + a) for a in (15, 17, 20, 41, 60))
    random_read = synth.decode(np.random.default_rng(7).integers(0, 4, 150))
    odd = _edit(_cut(g20, [-25])[0], p38="a", p70="R")       # (letter 13 of the prefix, a letter of the tract)
    reads_a = (_cut(g15, [-60, -50, -40, -30, -20], strands="+-") +           # FULL, 15 units, both strands
               _cut(g20, [-45, -35, -15, -5], strands="-+") +                 # FULL, 20 units
               _cut(g41, [-40, -31]) +                                        # prefix and part of the tract
               _cut(g60, [18 + 3]) +                                          # nothing but repeat
               [random_read,
                _edit(_cut(g15, [-33])[0], p5="N", p60="N"),
                odd])
    reads_b = (_cut(g20, [-50, -41, -32, -23, -14], strands="-+") + _cut(g17, [-60, -44, -28, -12], strands="+-") +
               _cut(g41, [-37]) + _cut(g41, [18 + 41 * 3 + 18 + 40 - 150]) + _cut(g60, [18 + 6], strands="-"))
    s12, s14, s40 = (_genome(sca10, a, 200 + a) for a in (12, 14, 40))
    reads_c = (_cut(s12, [-48, -40, -32, -24, -16, -8], strands="+-") + _cut(s14, [-44, -33, -22, -11], strands="-+") +
               _cut(s40, [-50]) + [synth.decode(np.random.default_rng(8).integers(0, 4, 150))])
    assert (len(reads_a), len(reads_b), len(reads_c)) == (15, 12, 12)

    def four(clip):
        return [Unit(hd, 150, reads_a, 30.0, 2, _lens(1, 40, 350), _lens(2, 6, 380), clip=clip),
                Unit(sca10, 150, reads_c, 24.5, 2, _lens(3, 30, 350), _lens(4, 4, 360), clip=clip),
                Unit(dm1, 150, [], 12.0, 1, [], [], clip=clip),
                Unit(hd, 150, reads_b, 41.0, 2, _lens(5, 25, 340), [], maxinsert=120, clip=clip)]

    rept = _cut(g60, [18 + 3, 18 + 9, 18 + 12], strands="+-")
    ids_a = list(range(9)) + [20, 20, 21]                                     # two repeat-only reads under one id
    paired = [Unit(hd, 150, reads_a[:9] + rept, 30.0, 2, _lens(1, 40, 350), _lens(2, 6, 380), read_pair_ids=ids_a),
              Unit(hd, 150, reads_b, 41.0, 2, _lens(5, 25, 340), [], read_pair_ids=list(range(100, 110)) + [110, 110]),
              Unit(sca10, 150, reads_c, 24.5, 2, _lens(3, 30, 350), _lens(4, 4, 360))]
    g100 = _genome(hd, 100, 300)
    long_ = [Unit(hd, 600, _cut(g100, [-120], n=600), 30.0, 2, _lens(6, 20, 900), []),
             Unit(sca10, 150, reads_c, 24.5, 2, _lens(3, 30, 350), _lens(4, 4, 360))]
    return {"four": (False, four(False)), "four_clip": (False, four(True)), "paired": (False, paired),
            "long": (True, long_)}, odd


# ---- what is recorded ---------------------------------------------------------------------------------------------------
def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _hex(x):
    return float(x).hex()


def _unit_result(r):
    out = {"tags": np.asarray(r.tags).tolist() if r.tags is not None else None,
           "hs": np.asarray(r.hs).tolist() if r.hs is not None else None,
           "scores": np.asarray(r.scores).tolist() if r.scores is not None else None,
           "full": {str(k): int(v) for k, v in sorted(r.full.items())},
           "pref": {str(k): int(v) for k, v in sorted(r.pref.items())},
           "rept_hist": {str(k): int(v) for k, v in sorted(r.rept_hist.items())},
           "rept": int(r.rept), "call": r.call.tobytes().hex(),
           "P_h1": {str(i): _hex(v) for i, v in enumerate(r.P_h1) if v != 0}, "P_h2": {str(i): _hex(v) for i, v in enumerate(r.P_h2) if v != 0},
           "marg_len": [len(r.P_h1), len(r.P_h2)], "joint": None, "total": None}
    if r.joint is not None:
        trip, total = r.joint
        out["joint"] = [[_hex(v) for v in row] for row in sorted(map(tuple, np.asarray(trip).tolist()))]
        out["total"] = _hex(total)
    out["grid"] = None if r.grid is None else _sha(r.grid)
    return out


def _refusal(call):
    try:
        call()
    except Exception as e:                     # (the kind and the text are what is recorded)
        return [type(e).__name__, str(e)]
    return None


def record_case(engine, units):
    tag, h, sc, uro, dump = engine.classify(units, want_dump=True)
    out = {"classify": _sha(tag, h, sc, uro, dump), "dump_shape": list(dump.shape), "uro": np.asarray(uro).tolist()}
    res = engine.genotype(units)
    out["genotype"] = [_unit_result(r) for r in res]
    out["genotype_no_grid"] = [[r.call.tobytes().hex(), r.joint is None] for r in engine.genotype(units, want_grid=False)]
    w = engine.winners(units)
    out["winners"] = {"items": np.asarray(w.items).tolist(), "win": np.asarray(w.win).tolist(),
                      "fields": np.asarray(w.fields).tolist(), "n_ops": np.asarray(w.n_ops).tolist(),
                      "ops": [row[:n].tolist() for row, n in zip(np.asarray(w.ops), np.asarray(w.n_ops).tolist())]}
    al = engine.alignments(units, winners=w)
    out["alignments"] = [{str(i): x.verbose() for i, x in sorted(a.items())} for a in al]
    alleles = [sorted(int(k) for k in r.full) + [41, 0] for r in res]
    co = engine.consensus(units, alleles, winners=w)
    out["consensus"] = [{str(a): x.to_dict() for a, x in sorted(c.items())} for c in co]
    return out


def record(engine, long_engine):
    """Everything the fixture holds, from an Engine and an Engine(long_reads=True)."""
    lists, odd = unit_lists()
    out = {ODD_READ: odd, "cases": {}}
    for name, (long_reads, units) in lists.items():
        out["cases"][name] = record_case(long_engine if long_reads else engine, units)
    four = lists["four"][1]
    # the odd read is unit 0's last one: it is tagged, and its aligned part stands verbatim in its block
    out["odd_in_block"] = odd[38:71] in out["cases"]["four"]["alignments"][0][str(len(four[0].reads) - 1)]
    hd = four[0]
    r = engine.grid_from_counts(Unit(hd.tred, 150, (), 30.0, 2, hd.global_lens, hd.target_lens), {15: 10, 41: 3}, {20: 2}, 1)
    assert r.tags is None and r.joint is None
    r.tags = r.hs = r.scores = None
    out["grid_from_counts"] = _unit_result(r)
    mixed = [four[0], lists["four_clip"][1][1]]
    too_long = [Unit(hd.tred, 150, [_genome(hd.tred, 100, 300)[FLANK - 50:FLANK + 450]], 30.0, 2, [], [])]
    out["refusals"] = {"mixed_clip_classify": _refusal(lambda: engine.classify(mixed)),
                       "mixed_clip_genotype": _refusal(lambda: engine.genotype(mixed)),
                       "read_500_classify": _refusal(lambda: engine.classify(too_long)),
                       "read_500_genotype": _refusal(lambda: engine.genotype(too_long))}
    return out


def main(argv):
    path = argv[0] if argv else OUT
    engine, long_engine = Engine(0), Engine(0, long_reads=True)
    try:
        got = record(engine, long_engine)
    finally:
        engine.close()
        long_engine.close()
    got["version"] = _lib.version()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fp:
        json.dump(got, fp, sort_keys=True, indent=0, separators=(",", ":"))
        fp.write("\n")
    print("wrote {} ({} bytes)".format(path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1:])
