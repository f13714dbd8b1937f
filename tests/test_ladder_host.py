"""CPU: tredparse_amd/csrc/ladder_host.h, the HIP-free host code the five opt-in units share, through the stand-alone
driver tests/ladder_host_main.cpp built with the address and undefined-behaviour sanitizers: the strand templates against a
restatement in Python, the two refusals, the scoring check at every edge of its range, the key of a ladder table, its
records and letter pool, every refusal's code and text, and the counting sort of items into buckets."""
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LONG_TEXT = ("scoring out of the supported range (match 1..8, mismatch 0..16, 1 <= gap_extend <= gap_open <= 16, "
             "flank 0..255)")
CIGAR_TEXT = "scoring out of the supported range (match 1..8, mismatch 0..16, 1 <= gap_extend <= gap_open <= 16)"


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ladder_host") / "ladder_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "ladder_host_main.cpp")])

    def call(*args):
        r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr        # the sanitizers report nothing
        return r.stdout.splitlines()
    return call


def letters(s):
    return "".join(c if c in "ACGT" else "N" for c in s.upper())


def rc(s):
    return letters(s)[::-1].translate(str.maketrans("ACGT", "TGCA"))


def expected(prefix, repeat, suffix, mu):
    if mu == 0:
        return ["strands 1 period {} max_units 0".format(len(repeat)), "{}\t0\t{}\t".format(len(prefix), letters(prefix))]
    return ["strands 2 period {} max_units {}".format(len(repeat), mu),
            "{}\t{}\t{}\t{}".format(len(prefix), len(suffix), letters(prefix + repeat * mu), letters(suffix)),
            "{}\t{}\t{}\t{}".format(len(suffix), len(prefix), rc(suffix) + rc(repeat) * mu, rc(prefix))]


LADDERS = [
    ("ACGTTGCA", "CAG", "TGACCT", 0),            # a plain reference
    ("ACGTTGCA", "CAG", "TGACCT", 1),
    ("ACGTTGCA", "CAG", "TGACCT", 4),
    ("", "CAG", "TGACCT", 3),                    # empty prefix
    ("ACGTTGCA", "CAG", "", 3),                  # empty suffix
    ("", "CAG", "", 2),                          # both empty
    ("", "", "", 0),                             # a plain reference of no letters: the callers' limits refuse it
    ("ACGTT", "A", "GGC", 5),                    # period 1
    ("ACGTT", "GGCCTG", "TTAGC", 3),             # period 6
    ("acgTtgca", "cAg", "tgacct", 2),            # lower case
    ("ACNGT", "CAG", "TGAC", 2),                 # N and a non-ACGT character in each part
    ("ACGT", "CNG", "TGAC", 2),
    ("ACGT", "CAG", "TGNAC", 2),
    ("AC-GT", "CAG", "TGAC", 2),
    ("ACGT", "C*G", "TGAC", 2),
    ("ACGT", "CAG", "TGxAC", 2),
    ("nR", "yn", "N.", 3),
    ("ACNGT", "", "TGAC", 0),                    # a plain reference takes no repeat
]


@pytest.mark.parametrize("ladder", LADDERS)
def test_strands_equal_the_restatement(run, ladder):
    assert run("L", *ladder) == expected(*ladder)


def test_refusals_and_ladder_numbering(run):
    out = run("L", "ACGT", "CAG", "TGAC", -1, "L", "ACGT", "", "TGAC", 2, "L", "", "", "", -3, "L", "ACGT", "CAG", "TGAC", 1)
    assert out[:3] == ["refused -2 ladder 0: negative max_units", "refused -2 ladder 1: empty repeat",
                       "refused -2 ladder 2: negative max_units"]
    assert out[3:] == expected("ACGT", "CAG", "TGAC", 1)     # a refusal leaves nothing behind in the next record


BASE = dict(match=1, mismatch=5, gap_open=7, gap_extend=2, flank=9)
EDGES = [   # one field (or two) moved to an edge of its range: just inside, just outside
    (dict(match=1), True), (dict(match=0), False), (dict(match=8), True), (dict(match=9), False),
    (dict(mismatch=0), True), (dict(mismatch=-1), False), (dict(mismatch=16), True), (dict(mismatch=17), False),
    (dict(gap_open=16), True), (dict(gap_open=17), False),
    (dict(gap_open=1, gap_extend=1), True), (dict(gap_open=0, gap_extend=0), False), (dict(gap_open=0, gap_extend=1), False),
    (dict(gap_extend=1), True), (dict(gap_extend=0), False), (dict(gap_extend=7), True), (dict(gap_extend=8), False),
    (dict(gap_open=16, gap_extend=16), True), (dict(gap_open=16, gap_extend=17), False),
]


def scoring(run, with_flank, **kw):
    p = dict(BASE, **kw)
    out = run("S", p["match"], p["mismatch"], p["gap_open"], p["gap_extend"], p["flank"], int(with_flank))
    assert len(out) == 1 and out[0].startswith("scoring ")
    return out[0][len("scoring "):]


@pytest.mark.parametrize("with_flank", [False, True])
def test_scoring_edges(run, with_flank):
    text = LONG_TEXT if with_flank else CIGAR_TEXT
    for kw, ok in EDGES:
        assert scoring(run, with_flank, **kw) == ("ok" if ok else text), kw
    for flank, ok in ((0, True), (-1, False), (255, True), (256, False)):
        assert scoring(run, with_flank, flank=flank) == ("ok" if ok or not with_flank else text), flank


# ---- what the two CIGAR units share --------------------------------------------------------------------------------------
TWO = [("ACGTTGCA", "CAG", "TGACCT", 2), ("ACNGT", "", "TGAC", 0)]     # a two-strand ladder and a plain reference


def flat(ladders):
    return [len(ladders)] + [x for l in ladders for x in l]


def test_key_tells_tables_apart(run):
    key = lambda ladders: run("K", *flat(ladders))
    assert key(TWO) == key(list(TWO)) and key(TWO)[0].startswith("key ")
    other = [TWO[0][:3] + (3,), TWO[1]]                                # differs in one max_units only
    assert key(other)[0].startswith("key ") and key(other) != key(TWO)
    assert key([TWO[0], TWO[1][:3] + (1,)]) != key(TWO)
    assert key(TWO[:1]) != key(TWO)
    assert key([("AC", "G", "T", 1)]) != key([("A", "CG", "T", 1)])    # the parts are kept apart
    assert run("K", 2, *TWO[0], "ACGT", "NULL", "TGAC", 1) == ["refused -2 ladder 1: NULL sequence"]
    assert run("K", 1, "NULL", "CAG", "TGAC", 1) == ["refused -2 ladder 0: NULL sequence"]
    assert run("K", 1, "ACGT", "CAG", "NULL", 1) == ["refused -2 ladder 0: NULL sequence"]


def expected_pool(ladders):
    """The records and the pool as the restatement gives them: per ladder and strand the trunk, then the branch."""
    pool, lines = "", []
    for l in ladders:
        strands = [x.split("\t") for x in expected(*l)[1:]]
        lines.append("{}\t{}".format(len(l[1]), l[3]))
        for alen, blen, trunk, branch in strands:
            lines.append("{}\t{}\t{}\t{}".format(alen, blen, len(pool), len(pool) + len(trunk)))
            pool += trunk + branch
        lines += ["0\t0\t0\t0"] * (2 - len(strands))                  # a plain reference has no second strand
    return ["pool " + pool + "N" * 16] + lines


@pytest.mark.parametrize("ladders", [TWO, TWO[::-1], TWO[:1], TWO[1:], [LADDERS[6]], LADDERS])
def test_pool_equals_the_restatement(run, ladders):
    assert run("P", 0, *flat(ladders)) == expected_pool(ladders)


def test_pack_refusals(run):
    long_one = ("A" * 2048, "C", "G" * 2047, 1)                        # its longest template has 4 096 letters
    text = "refused -2 ladder 1: longest template 4096 exceeds TREDGPU_MAX_LONG_TEMPLATE_LEN=4095"
    assert run("P", 4095, *flat([TWO[0], long_one])) == [text]
    assert run("P", 4096, *flat([TWO[0], long_one])) == expected_pool([TWO[0], long_one])
    assert run("P", 0, *flat([TWO[0], long_one])) == expected_pool([TWO[0], long_one])      # 0: no limit
    assert run("P", 4095, *flat([("A" * 4096, "", "", 0)])) == ["refused -2 ladder 0: longest template 4096 exceeds "
                                                                "TREDGPU_MAX_LONG_TEMPLATE_LEN=4095"]
    assert run("P", 0, *flat([TWO[0], ("ACGT", "", "TGAC", 2)])) == ["refused -2 ladder 1: empty repeat"]
    assert run("P", 0, *flat([("ACGT", "CAG", "TGAC", -1)])) == ["refused -2 ladder 0: negative max_units"]


def test_plain_reference_limits(run):
    """The switch sw_long.hip packs with: a plain reference must have 1 .. max_template letters, in words of its own, and
    nothing else changes."""
    plain = lambda n: [("A" * n, "", "", 0)]
    assert run("Q", 4095, *flat(plain(0))) == ["refused -2 ladder 0: reference length 0 not in [1,4095]"]
    assert run("Q", 4095, *flat(plain(4096))) == ["refused -2 ladder 0: reference length 4096 not in [1,4095]"]
    assert run("Q", 4095, *flat([TWO[0]] + plain(0))) == ["refused -2 ladder 1: reference length 0 not in [1,4095]"]
    for ladders in (plain(1), plain(4095), TWO, LADDERS[:6]):
        assert run("Q", 4095, *flat(ladders)) == expected_pool(ladders)
    long_one = ("A" * 2048, "C", "G" * 2047, 1)                        # a ladder keeps the text it has without the switch
    assert run("Q", 4095, *flat([long_one])) == run("P", 4095, *flat([long_one]))
    assert run("P", 4095, *flat(plain(0))) == expected_pool(plain(0))  # without the switch an empty reference passes


def bucket_order(run, n_buckets, keys):
    out = run("B", n_buckets, len(keys), *keys)
    assert len(out) == 2 and out[0].split()[0] == "order" and out[1].split()[0] == "off"
    return [int(x) for x in out[0].split()[1:]], [int(x) for x in out[1].split()[1:]]


RNG = random.Random(7)
BUCKET_CASES = [
    (3, []),                                                            # n = 0
    (0, []),
    (1, [0, 0, 0, 0, 0]),                                               # one bucket
    (1, [0, -1, 0]),
    (4, [-1, -7, -2147483648, -1]),                                     # all keys negative
    (6, [5, -1, 0, 3, -2147483648, 3, 0, -1000, 5, 5, 2, -3, 0]),       # negatives of any size mixed in
    (6, [RNG.randrange(6) for _ in range(1000)]),
    (4200, [RNG.randrange(4200) for _ in range(1000)]),
    (6, [RNG.randrange(-3, 6) for _ in range(1000)]),
    (4200, [RNG.choice([-1, -2 ** 31, RNG.randrange(4200)]) for _ in range(1000)]),
]


@pytest.mark.parametrize("n_buckets,keys", BUCKET_CASES, ids=lambda v: str(v) if isinstance(v, int) else "n{}".format(len(v)))
def test_bucket_order_is_a_stable_sort(run, n_buckets, keys):
    order, off = bucket_order(run, n_buckets, keys)
    kept = [k for k in range(len(keys)) if keys[k] >= 0]
    assert order == sorted(kept, key=lambda k: keys[k])                 # (sorted is stable: the caller's order within a bucket)
    assert off == [sum(1 for k in kept if keys[k] < b) for b in range(n_buckets + 1)]


ARGS_TEXT = "n_items, n_ladders and cap must be positive"
GOOD_CALL = dict(ctx=1, mem_ok=1, n_items=1, n_ladders=1, cap=8, null_table=0, params="1,5,7,2", null_array=-1)
CALLS = [    # in the order of the checks: an earlier one wins
    (dict(), 0, ""),
    (dict(n_items=0, null_array=0), 0, ""),                             # no items: the arrays are not looked at
    (dict(n_items=0x7fffffff), 0, ""),
    (dict(ctx=0, mem_ok=0, n_items=-1), -2, "ctx is NULL"),
    (dict(mem_ok=0, n_items=-1), -2, "mem must be TREDGPU_MEM_HOST or TREDGPU_MEM_DEVICE"),
    (dict(n_items=-1, null_table=1), -2, ARGS_TEXT),
    (dict(n_items=0x80000000), -2, ARGS_TEXT),
    (dict(n_ladders=0), -2, ARGS_TEXT),
    (dict(n_ladders=-1), -2, ARGS_TEXT),
    (dict(cap=0, params="NULL"), -2, ARGS_TEXT),
    (dict(null_table=1, params="NULL"), -2, "NULL ladder argument"),
    (dict(null_table=2), -2, "NULL ladder argument"),
    (dict(null_table=3), -2, "NULL ladder argument"),
    (dict(null_table=4), -2, "NULL ladder argument"),
    (dict(params="NULL", null_array=0), -2, "params is NULL"),
    (dict(params="0,5,7,2", null_array=0), -2, CIGAR_TEXT),
    (dict(params="1,5,7,8"), -2, CIGAR_TEXT),
] + [(dict(null_array=k), -2, "NULL array argument") for k in range(9)]


@pytest.mark.parametrize("kw,rc,text", CALLS)
def test_call_refusals(run, kw, rc, text):
    c = dict(GOOD_CALL, **kw)
    out = run("C", c["ctx"], c["mem_ok"], c["n_items"], c["n_ladders"], c["cap"], c["null_table"], c["params"], c["null_array"])
    assert out == ["call {} {}".format(rc, text)]


INSIDE = "item {}: its read does not lie inside packed[0 .. read_off[n_items])"
READS = [    # max_read, read_off (n + 1), read_len (n): a read of L letters has (L + 15) // 16 + (L + 31) // 32 words
    (2048, [0, 3], [20], 0, ""),
    (2048, [0, 2], [20], -2, INSIDE.format(0)),
    (2048, [3, 0], [20], -2, "read_off must be monotone"),
    (2048, [-1, 3], [20], -2, "read_off must be monotone"),
    (-1, [3, 0], [20], -2, "read_off must be monotone"),
    (-1, [0, 2], [20], 0, ""),                                          # max_read < 0: the reads are not looked at
    (-1, [5, 5], [20], 0, ""),
    (2048, [0, 3, 6], [20, 33], -2, INSIDE.format(1)),                  # 33 letters: 3 + 2 words
    (2048, [0, 3, 8], [20, 33], 0, ""),
    (2048, [0, 5, 8], [20, 20], 0, ""),                                 # the offsets say where a read begins, in any order
    (2048, [5, 0, 8], [20, 20], 0, ""),
    (2048, [0, -1, 8], [20, 20], -2, INSIDE.format(1)),
    (2048, [0, 0, 0], [0, 0], 0, ""),                                   # an empty read has no words
    (2048, [0, 0, 2], [-1, 2049], 0, ""),                               # reads the kernel refuses are not read
    (2048, [0, 0, 2], [0, 2048], -2, INSIDE.format(1)),
    (2048, [0, 0, 192], [0, 2048], 0, ""),                              # 128 + 64 words
    (480, [0, 0, 2], [0, 481], 0, ""),
]


@pytest.mark.parametrize("max_read,off,length,rc,text", READS)
def test_reads_refusals(run, max_read, off, length, rc, text):
    assert run("R", max_read, len(length), *off, *length) == ["reads {} {}".format(rc, text)]
