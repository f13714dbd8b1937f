"""CPU: tredparse_amd/csrc/kmer_host.h, the host builder of a ladder strand's 6-mer tables (presence bitmap and, for a ladder
with an N in its templates, the class j(w) of every 6-mer: the fewest N of any template window that produces it), through the
stand-alone driver tests/kmer_weight_main.cpp.  Both strands' tables against the restatement in tests/kmer_weight_model.py;
the same program is built and run once more with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from . import kmer_weight_model as km

HERE = os.path.dirname(os.path.abspath(__file__))
OPMD = ("CCAGTCTGAGCGGCGATG", "GGGGCTGCGGGCGGTCGG")      # 18-base flanks of data/treds.json
BPES = ("GCCAGGGCTACCGGGGCC", "CATCTGGCAGGAGGCATA")

LADDERS = [
    (OPMD[0], "GCN", OPMD[1], 50),
    (BPES[0], "NGC", BPES[1], 50),
    (OPMD[0], "N", OPMD[1], 50),                          # every repeat window is all N: all 4096 6-mers, class 6 at most
    (OPMD[0], "GCNGCA", OPMD[1], 25),
    (BPES[0], "GCATNCGGATCN", BPES[1], 12),               # a 12-mer with two N
    ("CCAGTCTGANCGGCGATG", "CAG", "GGGGCTGCGGNCGGTCGG", 50),   # an N in the prefix and one in the suffix
    (OPMD[0], "CAG", OPMD[1], 50),                        # N-free: no table, flag 0
    (OPMD[0], "GCN", OPMD[1], 1),                         # max_units 1
    (OPMD[0], "CAG", OPMD[1], 1),
    ("", "GCN", "", 3),                                   # no flanks
    ("ACN", "G", "", 2),                                  # templates shorter than six letters: no windows at all
]


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall"] + flags + ["-o", exe, os.path.join(HERE, "kmer_weight_main.cpp")])
    return exe


def _run(exe, ladders):
    r = subprocess.run([exe] + [str(x) for l in ladders for x in l], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return r.stdout.splitlines()


def expected(ladder):
    flag, tables = km.ladder_tables(*ladder)
    lines = ["flag {}".format(3 if flag else 0)]
    for t in tables:
        bits, cls = ["0"] * 4096, ["0"] * 4096
        for k, j in t.items():
            bits[km.index_of(k)] = "1"
            cls[km.index_of(k)] = "0123456"[j]
        lines += ["bits " + "".join(bits), "cls " + ("".join(cls) if flag else "-")]
    return lines


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kmer_weight")
    plain = _run(_build(tmp, "plain", ["-O1"]), LADDERS)
    checked = _run(_build(tmp, "san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), LADDERS)
    assert plain == checked              # the sanitizers report nothing (stderr empty, exit 0) and change nothing
    assert len(plain) == 5 * len(LADDERS)
    return [plain[5 * k:5 * k + 5] for k in range(len(LADDERS))]


@pytest.mark.parametrize("k", range(len(LADDERS)), ids=["{}x{}".format(l[1], l[3]) + ("" if l[0] in (OPMD[0], BPES[0]) else "_flanks") for l in LADDERS])
def test_tables_equal_the_restatement(outputs, k):
    assert outputs[k] == expected(LADDERS[k])


def test_the_cases_are_what_they_claim(outputs):
    flags = [int(o[0].split()[1]) for o in outputs]
    assert flags == [3, 3, 3, 3, 3, 3, 0, 3, 0, 3, 3]
    by = {(l[1], l[3], l[0] == OPMD[0]): o for l, o in zip(LADDERS, outputs)}
    assert by[("N", 50, True)][1] == "bits " + "1" * 4096                       # the all-N repeat stands for every 6-mer
    assert set(by[("N", 50, True)][2][4:]) == set("0123456")                    # classes 0 (flank windows) .. 6
    gcn = by[("GCN", 50, True)]
    idx = km.index_of("GCAGCT")                                                 # a repeat window: two N under it, on both strands
    assert gcn[2][4 + idx] == "2" and gcn[4][4 + idx] == "2"                    # rc((GCN)n) = (NGC)n: the same cyclic pattern
    assert by[("CAG", 50, True)][2] == "cls -" and by[("CAG", 50, True)][4] == "cls -"
    assert by[("G", 2, False)][1] == "bits " + "0" * 4096                       # five-letter templates have no window
    # the N-free ladder's bitmaps are those of the GCN ladder's flanks plus its own repeat: the bitmap rule did not change
    assert by[("CAG", 1, True)][1].count("1") == len(km.strand_table(km.strand_templates(OPMD[0], "CAG", OPMD[1], 1)[0]))
