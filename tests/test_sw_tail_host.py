"""CPU: the per-lane tail counts of tredparse_amd/csrc/kmer_host.h (tail_entry / tail_count / tail_pack: what
read_class_kernel stores in SwArgs::read_tail for the second tier of sw_cont_kernel's bounded-gain exit), through the
stand-alone driver tests/sw_tail_main.cpp.  For every read, strand and lane the count equals the `wtail` of
tests/sw_exit_model.gain_bounds; the same program is built and run once more with the address and undefined-behaviour
sanitizers.  A count above 254 is not possible for a read the table is built for (at most 155 windows): the saturation is
checked with masks given directly."""
import os
import subprocess

import numpy as np
import pytest

from . import sw_exit_model as xm

HERE = os.path.dirname(os.path.abspath(__file__))
HD = ("GAGTCCCTCAAGTCCTTC", "CAG", "CAACAGCCGCCACCGCCG", 50)
OPMD = ("CCAGTCTGAGCGGCGATG", "GCN", "GGGGCTGCGGGCGGTCGG", 50)
LENGTHS = {7: (5, 6, 16, 17, 100, 112), 10: (5, 6, 16, 17, 100, 105, 106, 112, 150, 160)}


def _reads(ladder, R):
    """reads of the lengths above: a FULL read (flank, repeat, flank) cut to length, its reverse complement, one with
    substitutions, then the named edge cases at the longest length."""
    rng = np.random.default_rng(7 * R + len(ladder[1]))
    a, rep, b, _ = ladder
    fill = lambda s: "".join("ACGT"[int(rng.integers(0, 4))] if c == "N" else c for c in s)
    out = [""]
    for L in LENGTHS[R]:
        units = max(1, (L - 24) // len(rep))
        full = fill(a[-12:] + rep * units + b + "".join("ACGT"[i] for i in rng.integers(0, 4, 200)))[:L]
        sub = list(full)
        for i in rng.choice(L, min(3, L), replace=False):
            sub[i] = "ACGT"[("ACGT".index(sub[i]) + 1) % 4]
        out += [full, xm.km.rc(full), "".join(sub)]
    L = LENGTHS[R][-1]
    base = fill(rep * (L // len(rep) + 2))[:L]
    out.append("N" + base[1:])                              # an N in the first window
    out.append(base[:-1] + "N")                             # an N in the last window
    out.append(base[:14] + "NNNN" + base[18:])              # Ns across the boundary of the first two 16-base words
    out.append(base[:L - 40] + "N" * 40)                    # an N tail: every window there counts
    out.append("A" * 3 + "T" * (L - 3) if "TTTTTT" not in (a + rep * 3 + b) else "ACGT" * (L // 4))
    out.append("".join("ACGT"[i] for i in rng.integers(0, 4, L)))
    return out


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall"] + flags + ["-o", exe, os.path.join(HERE, "sw_tail_main.cpp")])
    return exe


def _run(exe, ladder, R, lines):
    r = subprocess.run([exe] + [str(x) for x in ladder] + [str(R)], input="".join(l + "\n" for l in lines), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sw_tail")
    return _build(tmp, "plain", ["-O1"]), _build(tmp, "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _model(ladder, R, reads):
    """wtail [strand][read][lane] from sw_exit_model: window_presence, then gain_bounds with match 1 and lengths so large
    that its first bound never is the smaller one -- G2 = 5 + wtail"""
    tables = xm.Tables(*ladder)
    lens = np.asarray([len(r) for r in reads], np.int64)
    codes = np.full((len(reads), 16 * R), 4, np.int64)
    for i, r in enumerate(reads):
        codes[i, :len(r)] = xm.encode(r)
    out = []
    for s in range(2):
        pres, _ = xm.window_presence(codes, lens, tables, s)
        _, g2 = xm.gain_bounds(np.full(len(reads), 1 << 20, np.int64), pres, R, 1, True)
        out.append(g2[:, ::R][:, :16] - 5)
    return out


@pytest.mark.parametrize("R", [7, 10])
@pytest.mark.parametrize("ladder", [HD, OPMD], ids=["hd", "opmd_n"])
def test_tail_counts_equal_the_model(exes, ladder, R):
    reads = _reads(ladder, R)
    plain, checked = (_run(e, ladder, R, reads) for e in exes)
    assert plain == checked              # the sanitizers report nothing (stderr empty, exit 0) and change nothing
    assert len(plain) == 2 * len(reads)
    want = _model(ladder, R, reads)
    for i, rd in enumerate(reads):
        for s in range(2):
            got = [int(x) for x in plain[2 * i + s].split()]
            assert got[0] == s
            assert got[1:] == want[s][i].tolist(), (rd, s)
    got = np.asarray([[int(x) for x in l.split()[1:]] for l in plain]).reshape(len(reads), 2, 16)
    # the cases are what they claim
    assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == 0).all()       # lengths 0 and 5: no window
    assert got[:, :, 0].max() > 0 and (np.diff(got, axis=2) <= 0).all()                 # suffix counts never grow along the lanes
    L = LENGTHS[R][-1]
    ntail = got[-3]                                          # the read with 40 Ns at its end
    for lane in range(16):
        if lane * R >= L - 45:
            assert ntail[0, lane] == ntail[1, lane] == max(0, L - 5 - lane * R)       # every window there holds an N
    if ladder is HD:
        assert got[-2, 0].tolist() == [0] * 16                                          # a read with no present window (strand 0)
    if R == 10:
        k = 1 + 3 * LENGTHS[10].index(105)
        assert got[k, :, 10:].max() == 0        # L = 105: the last window starts at row 99, the last of lane 9
        k = 1 + 3 * LENGTHS[10].index(106)
        assert (got[k:k + 3, :, 11:] == 0).all()               # L = 106: one window more, the first row of lane 10


@pytest.mark.parametrize("R", [7, 10])
def test_saturation_and_mask_edges(exes, R):
    lines = ["=" + " ".join(["ffff"] * 20),          # 320 windows: lane 0 would hold 315
             "=" + " ".join(["ffff"] * 16),
             "=0 0 0 8000",                          # one window, ending at position 63
             "=",                                    # no word at all
             "=1ffff"]                               # bits above the 16 positions of a word are not counted
    plain, checked = (_run(e, HD, R, lines) for e in exes)
    assert plain == checked
    rows = [[int(x) for x in l.split()[1:]] for l in plain]
    for k, nb in ((0, 20), (1, 16)):
        want = [min(254, max(0, 16 * nb - (lane * R + 5))) for lane in range(16)]
        assert rows[k] == want
    assert rows[0][0] == 254 and max(rows[0]) == 254
    assert rows[2] == [1 if lane * R + 5 <= 63 else 0 for lane in range(16)]
    assert rows[3] == [0] * 16
    assert rows[4] == [11, 11 - R] + [0] * 14
