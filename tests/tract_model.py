"""The interrupted-tract scan (include/tredtract.h) restated in numpy and plain Python, by ALL PAIRS of seeds and connected
components -- not by the predecessor shortcut the kernels take: the definition every test of the kernel, the binding and
the catalogue checks against.  Nothing here comes from tredparse_amd.

Letters, codes, segments, e_p, maximal runs, whole copies and "primitive" are scan_model's.  Parameters per period
p = 1 .. 6 at [p - 1]: min_copies (0: the period is off), seed_copies, max_gap.

A seed of period p is a maximal period-p run [a, a + L) with L // p >= seed_copies[p - 1] and a primitive motif (what
scan_model.scan_segment gives with seed_copies in the place of min_copies); its template is T(x) = s[a + (x - a) % p].  Two
seeds [a1, b1), [a2, b2) of one segment and period, a1 < a2, are linked iff 1 <= a2 - b1 <= max_gap[p - 1] and
s[a2 + j] == s[a1 + (a2 - a1 + j) % p] for j < p (codes, not bytes).  A tract is a connected component of the links: from
its first seed's start to its last seed's end (start, L), `seeds` seeds, `mismatch` positions x of it with s[x] != T(x) (an N
counts).  It is a record iff L // p >= min_copies[p - 1].  Records are (segment, start, L, period, seeds, mismatch) in
ascending (segment, start, period) order.

Argument rules, per period that is on: 2 <= seed_copies <= min_copies, 0 <= max_gap <= MAX_GAP_LIMIT, and
seed_copies * p > max_gap + 2 p - 2 (then no seed fits between two linked seeds).
"""
import numpy as np

from . import scan_model as sm

MAX_PERIOD = sm.MAX_PERIOD
MAX_GAP_LIMIT = 64
SEED_COPIES = (5, 3, 3, 3, 3, 3)          # the defaults of the command line: a choice, not a measurement
MAX_GAP = (1, 2, 3, 4, 5, 6)              # one unit: a choice, not a measurement


def rule_violation(min_copies, seed_copies, max_gap):
    """None where the parameters are within the rules, else the text of the first one broken."""
    if len(min_copies) != MAX_PERIOD or len(seed_copies) != MAX_PERIOD or len(max_gap) != MAX_PERIOD:
        return "six entries each"
    if any(m == 1 or m < 0 for m in min_copies):
        return "min_copies: 0 or 2 and above"
    if not any(min_copies):
        return "every period is off"
    for p in range(1, MAX_PERIOD + 1):
        m, c, g = min_copies[p - 1], seed_copies[p - 1], max_gap[p - 1]
        if m == 0:
            continue
        if not 2 <= c <= m:
            return "period {}: 2 <= seed_copies <= min_copies".format(p)
        if not 0 <= g <= MAX_GAP_LIMIT:
            return "period {}: 0 <= max_gap <= {}".format(p, MAX_GAP_LIMIT)
        if not c * p > g + 2 * p - 2:
            return "period {}: seed_copies * p > max_gap + 2 p - 2".format(p)
    return None


def seeds_of(letters, min_copies, seed_copies):
    """{period: [(start, length)] ascending} of one segment; periods that are off have no seeds."""
    sc = [c if m else 0 for m, c in zip(min_copies, seed_copies)]
    out = {}
    if any(sc):
        for a, length, p in sm.scan_segment(letters, sc):
            out.setdefault(p, []).append((a, length))
    return out


def linked(s, p, r1, r2, max_gap):
    (a1, l1), (a2, _) = r1, r2
    g = a2 - (a1 + l1)
    return 1 <= g <= max_gap and all(s[a2 + j] == s[a1 + (a2 - a1 + j) % p] for j in range(p))


def tracts_segment(letters, min_copies=sm.MIN_COPIES, seed_copies=SEED_COPIES, max_gap=MAX_GAP):
    """[(start, length, period, seeds, mismatch)] of one segment, ascending (start, period)."""
    s = sm.codes_of(letters).astype(np.int16)
    out = []
    for p, seeds in sorted(seeds_of(letters, min_copies, seed_copies).items()):
        parent = list(range(len(seeds)))

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i

        # every pair (i, j), i < j: maximal runs of one period ascend in start AND end, so the gap from seed i only grows
        # with j and the pairs behind the first gap above max_gap cannot be linked
        for i in range(len(seeds)):
            for j in range(i + 1, len(seeds)):
                if seeds[j][0] - (seeds[i][0] + seeds[i][1]) > max_gap[p - 1]:
                    break
                if linked(s, p, seeds[i], seeds[j], max_gap[p - 1]):
                    parent[find(j)] = find(i)
        groups = {}
        for i in range(len(seeds)):
            groups.setdefault(find(i), []).append(seeds[i])
        for members in groups.values():
            a = min(m[0] for m in members)
            b = max(m[0] + m[1] for m in members)
            if (b - a) // p < min_copies[p - 1]:
                continue
            x = np.arange(a, b)
            mismatch = int(np.count_nonzero(s[x] != s[a + (x - a) % p]))
            out.append((int(a), int(b - a), p, len(members), mismatch))
    return sorted(out, key=lambda r: (r[0], r[2]))


def tracts(letters, seg_off, min_copies=sm.MIN_COPIES, seed_copies=SEED_COPIES, max_gap=MAX_GAP):
    """The call: letters of all segments, seg_off [n_seg + 1] -> [(segment, start, length, period, seeds, mismatch)]."""
    buf = letters.encode() if isinstance(letters, str) else letters
    buf = buf if isinstance(buf, np.ndarray) else np.frombuffer(bytes(buf), np.uint8)
    out = []
    for k in range(len(seg_off) - 1):
        out += [(k,) + r for r in tracts_segment(buf[int(seg_off[k]):int(seg_off[k + 1])], min_copies, seed_copies, max_gap)]
    return out


def arrays(records):
    """[(segment, start, length, period, seeds, mismatch)] as the six arrays of the call."""
    r = np.asarray(records, np.int64).reshape(-1, 6)
    return (r[:, 0].astype(np.int32), r[:, 1].copy(), r[:, 2].astype(np.int32), r[:, 3].astype(np.int32), r[:, 4].astype(np.int32),
            r[:, 5].astype(np.int32))


# ---- inputs the tests share ------------------------------------------------------------------------------------------------
FMR1 = "CGG" * 9 + "AGG" + "CGG" * 9 + "AGG" + "CGG" * 10
SCA1 = "CAG" * 12 + "CATCAGCAT" + "CAG" * 15


def random_params(rng):
    """(min_copies, seed_copies, max_gap) within the rules, every period on."""
    mc, sc, mg = [], [], []
    for p in range(1, MAX_PERIOD + 1):
        c = int(rng.integers(2, 6))
        g = int(rng.integers(0, min(MAX_GAP_LIMIT, c * p - 2 * p + 1) + 1))     # c p > g + 2 p - 2
        m = c + int(rng.integers(0, 4))
        mc.append(m), sc.append(c), mg.append(g)
    assert rule_violation(mc, sc, mg) is None
    return mc, sc, mg


def planted(rng, alphabet, n_lo=20, n_hi=160):
    """Random letters of `alphabet` with repeats of random motifs planted in them, some letters of which are substituted."""
    n = int(rng.integers(n_lo, n_hi + 1))
    s = rng.choice(list(alphabet), n)
    for _ in range(int(rng.integers(1, 4))):
        p = int(rng.integers(1, MAX_PERIOD + 1))
        motif = rng.choice(list(alphabet), p)
        length = int(rng.integers(2 * p, 60))
        at = int(rng.integers(0, max(1, n - length)))
        length = min(length, n - at)
        piece = np.resize(motif, length)
        for _ in range(int(rng.integers(0, 4))):
            piece[int(rng.integers(0, length))] = rng.choice(list(alphabet))
        s[at:at + length] = piece
    return "".join(s)
