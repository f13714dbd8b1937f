"""CPU: tredparse_amd/csrc/ladder_host.h, the host code sw_long.hip and sw_cigar.hip share, through the stand-alone driver
tests/ladder_host_main.cpp built with the address and undefined-behaviour sanitizers: the strand templates against a
restatement in Python, the two refusals, and the scoring check at every edge of its range."""
import os
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
