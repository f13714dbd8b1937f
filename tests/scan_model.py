"""The tandem-repeat scan (include/tredscan.h) restated in numpy and plain Python: the definition every test of the kernel,
the binding and the site builder checks against.  Nothing here comes from tredparse_amd.

Letters map by a 256-entry table (Aa 0, Cc 1, Gg 2, Tt 3, anything else 4).  For a period p and a segment s of n letters,
e_p[i] = 1 iff i + p < n, s[i] <= 3 and s[i] == s[i + p]; a maximal run of ones [i0, i1) of e_p is the maximal substring
[i0, i1 + p) of period p: length L = i1 - i0 + p, L // p whole copies, motif s[i0 : i0 + p].  It is a record iff
L // p >= min_copies[p - 1] and the motif has no period d with d | p, d < p.  Records are (segment, start, length, period)
in ascending (segment, start, period) order.
"""
import numpy as np

MAX_PERIOD = 6
MIN_COPIES = (10, 6, 5, 4, 4, 4)          # the defaults of the command line: a choice, not a measurement

TABLE = np.full(256, 4, np.uint8)
for _code, _letters in enumerate(("Aa", "Cc", "Gg", "Tt")):
    for _ch in _letters:
        TABLE[ord(_ch)] = _code


def codes_of(letters):
    """bytes / str / uint8 array -> the codes 0 .. 4."""
    if isinstance(letters, str):
        letters = letters.encode()
    return TABLE[np.frombuffer(bytes(letters), np.uint8)] if not isinstance(letters, np.ndarray) else TABLE[letters]


def primitive(motif):
    p = len(motif)
    return not any(p % d == 0 and all(motif[j] == motif[j + d] for j in range(p - d)) for d in range(1, p))


def scan_segment(letters, min_copies=MIN_COPIES):
    """[(start, length, period)] of one segment, ascending (start, period)."""
    s = codes_of(letters).astype(np.int16)
    n = len(s)
    out = []
    for p in range(1, MAX_PERIOD + 1):
        need = min_copies[p - 1]
        if need == 0 or n <= p:
            continue
        e = (s[:n - p] <= 3) & (s[:n - p] == s[p:])
        edge = np.diff(np.concatenate(([0], e.astype(np.int8), [0])))
        i0, i1 = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
        enough = (i1 - i0 + p) // p >= need
        for a, b in zip(i0[enough], i1[enough]):
            if primitive(list(s[a:a + p])):
                out.append((int(a), int(b - a) + p, p))
    return sorted(out, key=lambda r: (r[0], r[2]))


def scan(letters, seg_off, min_copies=MIN_COPIES):
    """The call: letters of all segments, seg_off [n_seg + 1] -> [(segment, start, length, period)]."""
    buf = letters.encode() if isinstance(letters, str) else letters
    buf = buf if isinstance(buf, np.ndarray) else np.frombuffer(bytes(buf), np.uint8)
    out = []
    for k in range(len(seg_off) - 1):
        out += [(k,) + r for r in scan_segment(buf[int(seg_off[k]):int(seg_off[k + 1])], min_copies)]
    return out


def arrays(records):
    """[(segment, start, length, period)] as the four arrays of the call."""
    r = np.asarray(records, np.int64).reshape(-1, 4)
    return r[:, 0].astype(np.int32), r[:, 1].copy(), r[:, 2].astype(np.int32), r[:, 3].astype(np.int32)


_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def canonical(motif):
    """The smallest rotation of the motif over both strands (upper-case str)."""
    m = motif.upper()
    rc = m.encode().translate(_COMPLEMENT)[::-1].decode()
    return min(x[k:] + x[:k] for x in (m, rc) for k in range(len(m)))
