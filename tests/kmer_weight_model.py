"""The 6-mer tables of a ladder strand and a read's 6-mer weight, restated in plain Python (tredparse_amd/csrc/kmer_host.h,
kmer_counts / kmer_weight in csrc/sw_ladder.hip).  Shared by tests/test_kmer_weight_host.py, tests/test_kmer_cap_model.py and
tests/test_sw_ncap_gpu.py."""
import itertools

COMP = str.maketrans("ACGTN", "TGCAN")


def letters(s):
    return "".join(c if c in "ACGT" else "N" for c in s.upper())


def rc(s):
    return letters(s)[::-1].translate(COMP)


def strand_templates(prefix, repeat, suffix, max_units):
    """[strand 0 templates, strand 1 templates], u = 1 .. max_units (bam_parser.py:92-93)."""
    p, r, s = letters(prefix), letters(repeat), letters(suffix)
    return [[p + r * u + s for u in range(1, max_units + 1)], [rc(s) + rc(r) * u + rc(p) for u in range(1, max_units + 1)]]


def strand_table(templates):
    """{6-mer: j}: the 6-mers some template window produces under some filling of its N, with the fewest N of such a window."""
    windows = set(t[i:i + 6] for t in templates for i in range(len(t) - 5))
    table = {}
    for w in windows:
        j = w.count("N")
        for fill in itertools.product("ACGT", repeat=j):
            it = iter(fill)
            k = "".join(next(it) if c == "N" else c for c in w)
            if table.get(k, 7) > j:
                table[k] = j
    return table


def ladder_tables(prefix, repeat, suffix, max_units):
    """(flag, [table of strand 0, table of strand 1]); flag: some template holds an N."""
    tt = strand_templates(prefix, repeat, suffix, max_units)
    return any("N" in t for ts in tt for t in ts), [strand_table(ts) for ts in tt]


def read_weight(read, table, with_n=True):
    """(cnt, J, W): present windows (a window with a read N counts), the sum of their classes, W = cnt - ceil(J / 6).  with_n =
    False: the ladder has no class table (J = 0, W = cnt)."""
    read = letters(read)
    cnt = J = 0
    for i in range(len(read) - 5):
        w = read[i:i + 6]
        if "N" in w:
            cnt += 1
        elif w in table:
            cnt += 1
            J += table[w] if with_n else 0
    return cnt, J, cnt - (J + 5) // 6


def index_of(kmer):
    """the 6-mer's index in the device tables: 2 bits per base, the first base in the low bits"""
    return sum("ACGT".index(c) << (2 * k) for k, c in enumerate(kmer))
