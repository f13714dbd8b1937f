"""CPU: tests/cigar_rowpar_model.py -- the row-parallel form of the banded pass that tredparse_amd/csrc/sw_cigar_long.hip
runs -- against the serial model tests/cigar_model.py on small rectangles, both models against the reference's long goldens
(tests/golden/sw_cigar_long.npz), and the fixture's own conditions."""
import os
import random

import numpy as np
import pytest

from . import cigar_model as cm
from . import cigar_rowpar_model as rp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASSES = ("La", "Lb", "Lc", "Ld", "Le", "Lf")


def _rectangle(rng, it):
    """(ref codes, read codes): random, periodic with substitutions and N, or a copy with indels."""
    rl, ql = rng.randint(1, 70), rng.randint(1, 70)
    if it % 3 == 0:
        return [rng.randint(0, 4) for _ in range(rl)], [rng.randint(0, 4) for _ in range(ql)]
    if it % 3 == 1:
        unit = [rng.randint(0, 3) for _ in range(rng.randint(1, 6))]
        read = (unit * 80)[rng.randint(0, 5):][:ql]
        return (unit * 80)[:rl], [c if rng.random() > 0.05 else rng.randint(0, 4) for c in read]
    ref = [rng.randint(0, 3) for _ in range(rl)]
    read = list(ref)
    for _ in range(rng.randint(0, 3)):
        p = rng.randint(0, len(read))
        if rng.random() < 0.5:
            read[p:p + rng.randint(1, 8)] = []
        else:
            read[p:p] = [rng.randint(0, 3) for _ in range(rng.randint(1, 8))]
    return ref, read[:70] or [0]


@pytest.mark.parametrize("seed", range(4))
def test_row_parallel_model_equals_the_serial_one(seed):
    """100 rectangles per seed: every pass (band and banded maximum), the status and the operations.  Scorings over the
    accepted range, gap_open == gap_extend in every fifth; scores from within the first band's reach to out of reach."""
    rng = random.Random("rowpar {}".format(seed))
    n_pass, statuses = 0, set()
    for it in range(100):
        m, x, go = rng.randint(1, 8), rng.randint(0, 16), rng.randint(1, 16)
        ge = go if it % 5 == 0 else rng.randint(1, go)
        ref, read = _rectangle(rng, it)
        top = m * min(len(ref), len(read))
        score = rng.choice([1, m * 5, top // 2, top, 4000])
        p1, p2 = [], []
        a = cm.banded_cigar(ref, read, score, m, x, go, ge, p1)
        b = rp.banded_cigar(ref, read, score, m, x, go, ge, p2)
        assert a == b and p1 == p2, (it, (m, x, go, ge), len(ref), len(read), score)
        n_pass += len(p1)
        statuses.add(a[0])
    assert n_pass >= 150 and statuses >= {cm.OK, cm.NO_PATH}


def test_row_parallel_model_needs_gap_extend_not_above_gap_open():
    with pytest.raises(AssertionError):
        rp.banded_cigar([0, 1], [0, 1], 1, 1, 5, 2, 3)


def test_row_parallel_model_reproduces_every_long_golden():
    g = rp.golden_long()
    for k in range(len(g["reads"])):
        st, ops = rp.cigar_of(g["refs"][k], g["reads"][k], g["fields"][k], *g["scoring"][k])
        assert (st, ops) == (cm.OK, g["ops"][k]), (k, g["cls"][k])


def _largest_pass(g, k):
    """Cells of the largest pass of golden k, from the bands the row-parallel model ran."""
    f = g["fields"][k]
    ref_len, read_len = int(f[2]) - int(f[1]) + 1, int(f[4]) - int(f[3]) + 1
    bands = [b for b, _ in rp.passes_of(g["refs"][k], g["reads"][k], f, *g["scoring"][k])[2]]
    return max(min(2 * b + 1, ref_len) * read_len for b in bands)


def test_serial_model_reproduces_the_long_goldens_with_small_passes():
    g = rp.golden_long()
    small = [k for k in range(len(g["reads"])) if _largest_pass(g, k) < 300000]
    assert len(small) >= 40 and {g["cls"][k] for k in small} >= {"La", "Lb", "Lc", "Ld"}
    for k in small:
        st, ops, passes = cm.passes_of(g["refs"][k], g["reads"][k], g["fields"][k], *g["scoring"][k])
        assert (st, ops) == (cm.OK, g["ops"][k]), (k, g["cls"][k])
        assert passes == rp.passes_of(g["refs"][k], g["reads"][k], g["fields"][k], *g["scoring"][k])[2]


def test_fixture_keeps_its_conditions():
    g = rp.golden_long()
    meta, n = g["meta"], len(g["reads"])
    assert os.path.getsize(os.path.join(GOLD, "sw_cigar_long.npz")) < 150 * 1024
    assert n >= 60 and not meta["excluded"] and meta["kept"] == meta["total"]
    assert all(g["cls"].count(c) == meta["kept"][c] >= 8 for c in CLASSES) and set(g["cls"]) == set(CLASSES)
    assert set(g["scoring"]) == {(1, 5, 7, 2), (2, 2, 3, 1), (8, 16, 16, 1)}
    assert {s for s, c in zip(g["scoring"], g["cls"]) if c in ("Lb", "Lc", "Ld")} == {(1, 5, 7, 2), (2, 2, 3, 1)}
    assert {s for s, c in zip(g["scoring"], g["cls"]) if c == "Le"} == {(2, 2, 3, 1), (8, 16, 16, 1)}
    assert meta["with_gap"] == sum(1 for o in g["ops"] if any(v & 15 for v in o)) >= 40
    assert meta["more_than_3_ops"] == sum(1 for o in g["ops"] if len(o) > 3) >= 15
    assert len(g["texts"]) == 8 and meta["reference_cpu_seconds"] > 0 and meta["largest_item_cpu_seconds"] > 0
    lens = {len(r) for r, c in zip(g["reads"], g["cls"]) if c == "Lb"}
    assert lens >= {300, 481, 512, 600, 1000, 1024, 1025, 2048}
    # every item is beyond tredcigar_sw_cigar's range: the read or the ladder's longest template
    for k in range(n):
        l = g["ladders"][g["ladder"][k]]
        longest = len(l[0]) + len(l[2]) + len(l[1]) * l[3] if l[3] else len(l[0])
        assert len(g["reads"][k]) > 480 or longest > 511, k
        assert cm.consumed(g["ops"][k]) == (g["fields"][k][4] - g["fields"][k][3] + 1, g["fields"][k][2] - g["fields"][k][1] + 1)
    # Le: one gap each, and the gaps cross one and two 64-lane chunks
    gaps = sorted(max(v >> 4 for v in g["ops"][k] if v & 15) for k in range(n) if g["cls"][k] == "Le")
    assert set(gaps) == {70, 100, 130, 200} and sum(64 < x <= 128 for x in gaps) >= 3 and sum(x > 128 for x in gaps) >= 3
    assert {v & 15 for k in range(n) if g["cls"][k] == "Le" for v in g["ops"][k]} == {0, 1, 2}
    # Ld: the band doubles two to five times
    doublings = {len(rp.passes_of(g["refs"][k], g["reads"][k], g["fields"][k], *g["scoring"][k])[2]) - 1
                 for k in range(n) if g["cls"][k] == "Ld"}
    assert doublings >= {2, 3, 5}
    # Lf: the rectangle of the limits in one band
    k = meta["largest_item"]
    f = g["fields"][k]
    assert g["cls"][k] == "Lf" and (f[2] - f[1] + 1, f[4] - f[3] + 1) == (4095, 2048) and g["scoring"][k] == (8, 16, 16, 1)
    assert g["ops"][k] == [1024 << 4, 2047 << 4 | 2, 1024 << 4]
    assert any(g["cls"][k] == "Lf" and (g["fields"][k][2] - g["fields"][k][1], g["fields"][k][4] - g["fields"][k][3]) == (2047, 2047)
               and g["ops"][k] == [2048 << 4] for k in range(n))


def test_alignment_report_golden_names_details_reads():
    import json
    rep = json.load(open(os.path.join(GOLD, "alignments_synlong600.json")))["loci"]
    run = json.load(open(os.path.join(GOLD, "run_long.json")))["samples"]["synlong600"]["tredCalls"]
    assert "HD" in rep and len(rep) == 2
    for name, rows in rep.items():
        assert [[r["id"], r["tag"], r["h"]] for r in rows] == [[d[0], d[1], int(d[2])] for d in run[name + ".details"]]
        assert all(len(r["block_sha256"]) == 64 and r["strand"] in "+-" and len(r["fields"]) == 5 and r["cigar_string"] for r in rows)
