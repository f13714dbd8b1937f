"""Plain-Python restatement of the reference's banded_sw (src/ssw.c:549-736) on the sub-rectangle
ref[ref_begin..ref_end] x read[read_begin..read_end] that ssw_align hands it (ssw.c:852-867): the CPU yardstick of
tredparse_amd/csrc/sw_cigar.hip and the executable statement of the quirks the kernel keeps.

The banded pass is kept line for line, arrays and index macros included (set_u / set_d, ssw.c:55-58), because three
of its habits only show through them:
  * h_b[edge] / e_b[edge] are zeroed at the start of every row (:596-597).  That is the "outside the band reads 0"
    rule -- and, while the band still starts at column 0 and already ends at the last column, it also wipes the real
    H and E above the last column.
  * E and F are stored unfloored (:608-617); only e1 / f1, the copies compared with the diagonal, are floored.
  * ties: the diagonal wins (temp1 <= temp2, :627), F wins over E unless e1 > f1 (:628), a gap extends unless opening
    is strictly better (:612, :617).
The traceback (:636-715) starts at the last cell, runs until i == 0 whatever H is, emits a zero-length M when the
first step is a gap, and closes with e+1 M or with `e op` + 1M.

Where the reference would run off its buffers the model returns a status instead:
  NO_PATH   the band covers the whole rectangle and the maximum is still below `score`
  OFF_EDGE  the traceback steps to a cell outside the band's storage of its row (j < 0 included)
Operations are (length << 4 | op), M=0 I=1 D=2 (to_cigar_int, ssw.h:132-156), oldest first.
"""

OK, NO_PATH, OFF_EDGE, OVERFLOW, TOO_LONG, BAD_ITEM = 0, 1, 2, 3, 4, 5
OPS = "MID"
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def encode(seq):
    """Aligner._DNA_to_int_mat (ssw_wrap.py:229-244): anything but ACGT is 4."""
    return [CODE.get(ch, 4) for ch in seq.upper()]


def _set_u(w, i, j):
    x = i - w
    return j - (x if x > 0 else 0) + 1


def _set_x(w, i, j):
    x = i - w
    return j - (x if x > 0 else 0)


def banded_cigar(ref, read, score, match=1, mismatch=5, gap_open=7, gap_extend=2, passes=None):
    """ref, read: code lists of the sub-rectangle.  Returns (status, [ops]).  passes: a list that receives (band, banded
    maximum so far) of every pass the model ran, in order."""
    ref_len, read_len = len(ref), len(read)
    cover = max(ref_len, read_len) - 1
    bw = abs(ref_len - read_len) + 1
    best = 0
    while True:
        width, width_d = bw * 2 + 3, bw * 2 + 1
        h_b, e_b, h_c = [0] * (width + 1), [0] * (width + 1), [0] * (width + 1)
        dirs = [None] * (width_d * read_len)          # (de, df, dh) per cell
        for i in range(read_len):
            beg, end = max(0, i - bw), min(ref_len - 1, i + bw)
            edge = min(end + 1, width - 1)
            f = 0
            h_b[0] = e_b[0] = h_b[edge] = e_b[edge] = h_c[0] = 0
            u = 0
            for j in range(beg, end + 1):
                u, e = _set_u(bw, i, j), _set_u(bw, i - 1, j)
                b, d = _set_u(bw, i, j - 1), _set_u(bw, i - 1, j - 1)
                t1 = -gap_open if i == 0 else h_b[e] - gap_open
                t2 = -gap_extend if i == 0 else e_b[e] - gap_extend
                e_b[u] = max(t1, t2)
                de = 3 if t1 > t2 else 2
                t1, t2 = h_c[b] - gap_open, f - gap_extend
                f = max(t1, t2)
                df = 5 if t1 > t2 else 4
                e1, f1 = max(e_b[u], 0), max(f, 0)
                t1 = max(e1, f1)
                a, q = ref[j], read[i]
                t2 = h_b[d] + (0 if a == 4 or q == 4 else match if a == q else -mismatch)
                h_c[u] = max(t1, t2)
                best = max(best, h_c[u])
                dh = 1 if t1 <= t2 else (de if e1 > f1 else df)
                dirs[width_d * i + _set_x(bw, i, j)] = (de, df, dh)
            for j in range(1, u + 1):
                h_b[j] = h_c[j]
        if passes is not None:
            passes.append((bw, best))
        if best >= score:
            break
        if bw >= cover:
            return NO_PATH, []
        bw = min(bw * 2, cover)                        # any band that covers the rectangle computes the same cells

    i, j, e, which = read_len - 1, ref_len - 1, 0, 2
    op = prev = "M"
    out = []
    while i > 0:
        x = _set_x(bw, i, j)
        if j < max(0, i - bw) or j > i + bw:           # a cell this pass never wrote
            return OFF_EDGE, []
        step = dirs[width_d * i + x][which]
        if step == 1:
            i, j, which, op = i - 1, j - 1, 2, "M"
        elif step == 2:
            i, which, op = i - 1, 0, "I"
        elif step == 3:
            i, which, op = i - 1, 2, "I"
        elif step == 4:
            j, which, op = j - 1, 1, "D"
        else:
            j, which, op = j - 1, 2, "D"
        if op == prev:
            e += 1
        else:
            out.append(e << 4 | OPS.index(prev))
            prev, e = op, 1
    if op == "M":
        out.append((e + 1) << 4)
    else:
        out.append(e << 4 | OPS.index(op))
        out.append(1 << 4)
    return OK, out[::-1]


def cigar_of(ref_seq, query_seq, fields, match=1, mismatch=5, gap_open=7, gap_extend=2):
    """The CIGAR ssw_align attaches to the alignment {score, ref_begin, ref_end, read_begin, read_end} of the pair."""
    score, rb, re_, qb, qe = (int(v) for v in fields[:5])
    return banded_cigar(encode(ref_seq)[rb:re_ + 1], encode(query_seq)[qb:qe + 1], score, match, mismatch, gap_open,
                        gap_extend)


def passes_of(ref_seq, query_seq, fields, match=1, mismatch=5, gap_open=7, gap_extend=2):
    """(status, [ops], [(band, banded maximum so far)] of every pass the model ran for the item)."""
    score, rb, re_, qb, qe = (int(v) for v in fields[:5])
    passes = []
    st, ops = banded_cigar(encode(ref_seq)[rb:re_ + 1], encode(query_seq)[qb:qe + 1], score, match, mismatch, gap_open,
                           gap_extend, passes)
    return st, ops, passes


def bands_of(ref_seq, query_seq, fields, match=1, mismatch=5, gap_open=7, gap_extend=2):
    """The sequence of bands the model ran for the item (band 1, 2, 4 ... while the banded maximum is below the score)."""
    return [b for b, _ in passes_of(ref_seq, query_seq, fields, match, mismatch, gap_open, gap_extend)[2]]


_limits = {}


def narrow_limits():
    """(NARROW_ROW, NARROW_PLANE) as tredparse_amd/csrc/sw_cigar.hip declares them."""
    if not _limits:
        import os
        import re
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        src = open(os.path.join(root, "tredparse_amd", "csrc", "sw_cigar.hip")).read()
        for name in ("NARROW_ROW", "NARROW_PLANE"):
            _limits[name] = int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))
    return _limits["NARROW_ROW"], _limits["NARROW_PLANE"]


def is_wide(bands, read_len):
    """The tier the kernel finishes an item in, predicted from the bands the model ran over its read_len rows: the narrow
    kernel hands the item on at the first pass whose row (2 * band + 3 entries) or plane ((2 * band + 1) * read_len
    cells) does not fit its storage."""
    row, plane = narrow_limits()
    return any(2 * b + 3 > row - 1 or (2 * b + 1) * read_len > plane for b in bands)


def consumed(ops):
    """(query bases, reference bases) the operations consume."""
    q = sum(v >> 4 for v in ops if v & 15 in (0, 1))
    r = sum(v >> 4 for v in ops if v & 15 in (0, 2))
    return q, r


def rescore(ref_seq, query_seq, fields, ops, match=1, mismatch=5, gap_open=7, gap_extend=2):
    """Score of the alignment the operations spell (a gap of n bases costs gap_open + (n - 1) * gap_extend)."""
    ref, read = encode(ref_seq), encode(query_seq)
    j, i, s = int(fields[1]), int(fields[3]), 0
    for v in ops:
        n, op = v >> 4, v & 15
        if op == 0:
            for k in range(n):
                a, q = ref[j + k], read[i + k]
                s += 0 if a == 4 or q == 4 else match if a == q else -mismatch
            i, j = i + n, j + n
        elif n > 0:
            s -= gap_open + (n - 1) * gap_extend
            if op == 1:
                i += n
            else:
                j += n
    return s


# ---- the golden items (tests/golden/sw_cigar.npz, tools/gen_golden_cigar.py) --------------------------------------------
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def template(ladder, t):
    """Template t of a ladder (prefix, repeat, suffix, max_units) in db order; max_units 0: the plain reference."""
    prefix, repeat, suffix, mu = ladder
    if mu == 0:
        return prefix
    s = prefix + repeat * (t // 2 + 1) + suffix
    return "".join(_COMP[c] for c in reversed(s)) if t % 2 else s


_golden = {}


def golden():
    """The golden items, loaded once: dict with ladders, cls, ladder, template, reads, refs, fields, ops (list of lists)
    and texts ({cigar_string, alignment, str} per item)."""
    if not _golden:
        import json
        import os
        import numpy as np
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_cigar.npz"))
        meta = json.loads(str(g["meta"]))
        ladders = [(l[0], l[1], l[2], int(l[3])) for l in meta["ladders"]]
        off = g["ops_off"]
        _golden.update(ladders=ladders, cls=[str(c) for c in g["cls"]], ladder=g["ladder"].astype(np.int32),
                       template=g["template"].astype(np.int32), reads=[str(r) for r in g["reads"]],
                       fields=g["fields"].astype(np.int16), texts=meta["texts"], meta=meta,
                       ops=[[int(v) for v in g["ops"][off[k]:off[k + 1]]] for k in range(len(off) - 1)])
        _golden["refs"] = [template(ladders[l], int(t)) for l, t in zip(_golden["ladder"], _golden["template"])]
    return _golden


_golden_scorings = {}


def golden_scorings():
    """tests/golden/sw_cigar_scorings.npz (tools/gen_golden_cigar.py --scoring), loaded once: as golden(), with scoring
    ((match, mismatch, gap_open, gap_extend) per item) and cigar_string (the reference's text per item)."""
    if not _golden_scorings:
        import json
        import os
        import numpy as np
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sw_cigar_scorings.npz"))
        meta = json.loads(str(g["meta"]))
        ladders = [(l[0], l[1], l[2], int(l[3])) for l in meta["ladders"]]
        off = g["ops_off"]
        _golden_scorings.update(
            ladders=ladders, cls=[str(c) for c in g["cls"]], ladder=g["ladder"].astype(np.int32),
            template=g["template"].astype(np.int32), reads=[str(r) for r in g["reads"]], fields=g["fields"].astype(np.int16),
            scoring=[tuple(int(v) for v in row) for row in g["scoring"]], cigar_string=meta["cigar_string"], meta=meta,
            ops=[[int(v) for v in g["ops"][off[k]:off[k + 1]]] for k in range(len(off) - 1)])
        _golden_scorings["refs"] = [template(ladders[l], int(t)) for l, t in
                                    zip(_golden_scorings["ladder"], _golden_scorings["template"])]
    return _golden_scorings
