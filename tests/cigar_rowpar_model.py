"""NumPy restatement of the banded pass of tests/cigar_model.py in the row-parallel form that
tredparse_amd/csrc/sw_cigar_long.hip runs, plus the serial traceback: the CPU yardstick for rectangles the pure-Python
model is too slow for (a 2 048 x 4 095 pass has 8.4 M cells).

The pass keeps the reference's storage -- the row arrays h_b / e_b and their index arithmetic (set_u, ssw.c:55-58) --
because what a cell above the band's end reads depends on it.  Per row, in this order:
  1. entries 0 and `edge` of h_b and e_b are zeroed (ssw.c:596-597);
  2. ALL loads: h_b[e], e_b[e] (0 in row 0) and h_b[d] of every band column.  The serial loop never reads an entry it has
     written in the same row (it writes e_b[u] with u <= e and h_b only after the row), so this is the serial order;
  3. E and the diagonal term per column, H~ = max(e1, diag);
  4. F as ONE max-scan along the row.  F_j = max(H_{j-1} - gO, F_{j-1} - gE) and H_{j-1} = max(H~_{j-1}, F_{j-1}); since
     gE <= gO (the scoring check enforces it) the F_{j-1} - gO term never wins, so with G_j = F_j + j * gE
         G_j = max(G_beg, max_{beg <= k < j} (H~_k - gO + (k + 1) * gE)),   G_beg = -gE + beg * gE
     (the row's first F is 0 - gE: h_c[0] = 0 and f = 0, and the extension wins the tie);
  5. H = max(e1, f1, diag); the F direction is 5 where opening won strictly, H_{j-1} - gO > F_{j-1} - gE, which is
     G_j > G_{j-1}, and 4 at `beg`;
  6. ALL stores: e_b[u], then h_b[u] = H (the serial loop's h_c and its copy after the row).
The arrays are poisoned at the start of a pass wherever the kernel does not initialise them, so a read of an entry that
neither this pass nor step 1 has written would show as a difference from the serial model.
"""
import numpy as np

from .cigar_model import NO_PATH, OFF_EDGE, OK

POISON = -20000
NEG = -(1 << 29)


def banded_pass(ref, read, bw, match, mismatch, gap_open, gap_extend):
    """One pass at band bw over code arrays ref / read: (maximum H, plane, stride).  plane[i * stride + (j - beg_i)] is the
    kernel's byte of cell (i, j): bit 0 E's code - 2, bit 1 F's code - 4, bits 2-4 H's code."""
    ref_len, read_len = len(ref), len(read)
    width = 2 * bw + 3
    stride = min(2 * bw + 1, ref_len)
    n_row = ref_len + 3
    h_b = np.full(n_row, POISON, np.int64)
    e_b = np.full(n_row, POISON, np.int64)
    h_b[:min(width - 1, n_row)] = 0                       # ssw.c:577: h_b[1 .. width - 2] = 0 (entry 0 per row)
    plane = np.zeros(stride * read_len, np.uint8)
    best = 0
    gO, gE = gap_open, gap_extend
    for i in range(read_len):
        beg, end = max(0, i - bw), min(ref_len - 1, i + bw)
        edge = min(end + 1, width - 1)
        h_b[0] = e_b[0] = h_b[edge] = e_b[edge] = 0
        s = beg - max(i - 1 - bw, 0)                      # 0 or 1: the band origin moved with this row
        j = np.arange(beg, end + 1)
        u = j - beg + 1
        e = u + s
        he = np.zeros(len(j), np.int64) if i == 0 else h_b[e]
        ee = np.zeros(len(j), np.int64) if i == 0 else e_b[e]
        hd = h_b[e - 1]
        t1, t2 = he - gO, ee - gE
        ev = np.maximum(t1, t2)
        de = np.where(t1 > t2, 3, 2)
        e1 = np.maximum(ev, 0)
        a, q = ref[beg:end + 1], read[i]
        sc = np.where((a == 4) | (q == 4), 0, np.where(a == q, match, -mismatch))
        diag = hd + sc
        ht = np.maximum(e1, diag)
        src = ht - gO + (j + 1) * gE
        g = np.empty(len(j), np.int64)
        g[0] = -gE + beg * gE
        if len(j) > 1:
            g[1:] = np.maximum(g[0], np.maximum.accumulate(src[:-1]))
        f = g - j * gE
        df = np.full(len(j), 4)
        df[1:] = np.where(g[1:] > g[:-1], 5, 4)
        f1 = np.maximum(f, 0)
        t = np.maximum(e1, f1)
        h = np.maximum(t, diag)
        dh = np.where(t <= diag, 1, np.where(e1 > f1, de, df))
        best = max(best, int(h.max()))
        plane[stride * i + (j - beg)] = (de - 2) | ((df - 4) << 1) | (dh << 2)
        e_b[u] = ev
        h_b[u] = h
    return best, plane, stride


def traceback(plane, stride, bw, ref_len, read_len):
    """ssw.c:636-715 over the plane of the last pass: (status, [ops])."""
    i, j, e, which, op, prev = read_len - 1, ref_len - 1, 0, 2, 0, 0
    out = []
    while i > 0:
        beg = max(0, i - bw)
        if j < beg or j > i + bw:
            return OFF_EDGE, []
        c = int(plane[stride * i + (j - beg)])
        step = 2 + (c & 1) if which == 0 else 4 + ((c >> 1) & 1) if which == 1 else c >> 2
        if step == 1:
            i, j, which, op = i - 1, j - 1, 2, 0
        elif step == 2:
            i, which, op = i - 1, 0, 1
        elif step == 3:
            i, which, op = i - 1, 2, 1
        elif step == 4:
            j, which, op = j - 1, 1, 2
        else:
            j, which, op = j - 1, 2, 2
        if op == prev:
            e += 1
        else:
            out.append(e << 4 | prev)
            prev, e = op, 1
    if op == 0:
        out.append((e + 1) << 4)
    else:
        out.append(e << 4 | op)
        out.append(1 << 4)
    return OK, out[::-1]


def banded_cigar(ref, read, score, match=1, mismatch=5, gap_open=7, gap_extend=2, passes=None):
    """cigar_model.banded_cigar's signature and results: ref, read are code sequences of the sub-rectangle."""
    assert 1 <= gap_extend <= gap_open
    ref, read = np.asarray(ref, np.int64), np.asarray(read, np.int64)
    ref_len, read_len = len(ref), len(read)
    cover = max(ref_len, read_len) - 1
    bw = abs(ref_len - read_len) + 1
    best = 0
    while True:
        m, plane, stride = banded_pass(ref, read, bw, match, mismatch, gap_open, gap_extend)
        best = max(best, m)
        if passes is not None:
            passes.append((bw, best))
        if best >= score:
            break
        if bw >= cover:
            return NO_PATH, []
        bw = min(bw * 2, cover)
    return traceback(plane, stride, bw, ref_len, read_len)


_CODE = np.full(256, 4, np.int64)
for _k, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _k


def encode(seq):
    return _CODE[np.frombuffer(seq.encode("latin-1"), np.uint8)]


def passes_of(ref_seq, query_seq, fields, match=1, mismatch=5, gap_open=7, gap_extend=2):
    """(status, [ops], [(band, banded maximum so far)]) as cigar_model.passes_of gives them."""
    score, rb, re_, qb, qe = (int(v) for v in fields[:5])
    passes = []
    st, ops = banded_cigar(encode(ref_seq)[rb:re_ + 1], encode(query_seq)[qb:qe + 1], score, match, mismatch, gap_open,
                           gap_extend, passes)
    return st, ops, passes


def cigar_of(ref_seq, query_seq, fields, match=1, mismatch=5, gap_open=7, gap_extend=2):
    return passes_of(ref_seq, query_seq, fields, match, mismatch, gap_open, gap_extend)[:2]


# ---- the long golden items (tests/golden/sw_cigar_long.npz, tools/gen_golden_cigar_long.py) ----------------------------------
_golden_long = {}


def golden_long():
    """The long golden items, loaded once: as cigar_model.golden_scorings(), with texts ({item index: {cigar_string,
    alignment, str}} for the 8 items that carry them)."""
    if not _golden_long:
        import json
        import os
        from .cigar_model import template
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_cigar_long.npz"))
        meta = json.loads(str(g["meta"]))
        ladders = [(l[0], l[1], l[2], int(l[3])) for l in meta["ladders"]]
        off = g["ops_off"]
        _golden_long.update(
            ladders=ladders, cls=[str(c) for c in g["cls"]], ladder=g["ladder"].astype(np.int32),
            template=g["template"].astype(np.int32), reads=[str(r) for r in g["reads"]], fields=g["fields"].astype(np.int16),
            scoring=[tuple(int(v) for v in row) for row in g["scoring"]], meta=meta,
            texts={int(k): v for k, v in meta["texts"].items()},
            ops=[[int(v) for v in g["ops"][off[k]:off[k + 1]]] for k in range(len(off) - 1)])
        _golden_long["refs"] = [template(ladders[l], int(t)) for l, t in zip(_golden_long["ladder"], _golden_long["template"])]
    return _golden_long
