"""CPU: tests/second_model.c -- the scalar restatement of ssw_align's score1 / ref_end1 / score2 / ref_end2 (DESIGN,
"Second-best alignment") -- against the values of the compiled reference in tests/golden/sw_second.npz, what that fixture
holds and left out, the exported symbols of include/tredsecond.h and the texts of PyAlignRes."""
import os
import re
import subprocess

import numpy as np

from tredparse_amd import _lib, ssw

from . import second_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORINGS = ["1/5/7/2", "2/2/3/1", "1/16/16/1", "4/6/10/1", "8/16/16/16", "8/0/1/1", "1/1/1/1"]


def test_model_equals_the_reference_on_every_kept_pair():
    g = sm.golden()
    assert len(g["reads"]) > 400
    for k, (read, ref) in enumerate(zip(g["reads"], g["refs"])):
        got = sm.second(read, ref, g["scoring"][k], g["mask_len"][k])
        assert got == tuple(int(v) for v in g["expect"][k]), (k, g["cls"][k], list(g["scoring"][k]), got, list(g["expect"][k]))


def test_what_the_fixture_left_out():
    """Nothing where gap_open > gap_extend; at most 5 % of a scoring's pairs where the two are equal (the reference's word
    pass leaves its lazy-F loop early there, and the generator leaves out only pairs that rule explains)."""
    meta = sm.golden()["meta"]
    assert meta["scorings"] == SCORINGS
    for tag in SCORINGS:
        _, _, go, ge = (int(v) for v in tag.split("/"))
        total, kept, out = meta["total"][tag], meta["kept"][tag], meta["left_out"][tag]
        assert kept + out == total and total >= 60
        assert out <= 0.05 * total, (tag, out, total)
        if go > ge:
            assert out == 0, (tag, out)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sw_second.npz")) < 250 * 1024


def test_the_fixture_holds_the_crafted_shapes():
    g = sm.golden()
    tags = ["/".join(str(v) for v in s) for s in g["scoring"]]
    for tag in SCORINGS:                                   # about 60 random / periodic / ladder pairs per scoring
        assert sum(1 for t, c in zip(tags, g["cls"]) if t == tag and c in "rl") >= 55, tag
    lens = lambda cls: {len(r) for r, c in zip(g["reads"], g["cls"]) if c == cls}
    assert {15, 16, 17, 24, 25} <= lens("p") and lens("b") == {249, 250} and {30, 31, 32} <= lens("m")
    assert {64, 65, 128, 129, 256, 257, 480, 481, 512, 513, 1024, 1025, 2047, 2048} <= lens("c")
    assert max(len(r) for r in g["refs"]) == 4095
    e, m = g["expect"], g["mask_len"]
    assert ((m == 14) & (e[:, 2] == 0) & (e[:, 3] == -1)).any()                         # mask_len < 15
    assert ((m >= 15) & (e[:, 2] == 0) & (e[:, 3] == 0)).any()                          # nothing outside the mask
    assert (e[:, 1] - m <= 0).any() and np.any(e[:, 1] + m >= [len(r) for r in g["refs"]])
    b = [k for k, c in enumerate(g["cls"]) if c == "b"]
    assert sorted(int(e[k, 0]) + 5 for k in b) == [254, 254, 255, 255]                  # both sides of the pass boundary
    assert any(e[k, 3] == e[k, 1] + m[k] for k in b) and any(e[k, 3] == e[k, 1] + m[k] + 1 for k in b)
    # a value of the read's last row leaves the mask through the padding rows: the runner-up starts right behind the mask
    carried = [k for k, c in enumerate(g["cls"]) if c == "p" and m[k] == len(g["reads"][k]) and m[k] > 30]
    assert len(carried) >= 5 and all(e[k, 3] == e[k, 1] + m[k] + 1 and e[k, 2] >= 16 for k in carried)
    assert any(t % 2 for t in g["template"]) and any(l[3] > 0 for l in g["ladders"])    # ladders, both strands


def test_the_mask_rules_of_the_model():
    read = "ACGTTGCAAGGCTTAACCGGTTAGCATCGATCGGATCCA"[:36]
    ref = "T" * 30 + read + "G" * 30 + read[:20] + "C" * 9
    s1, e1, s2, e2 = sm.second(read, ref, (1, 5, 7, 2), 18)
    assert (s1, e1) == (36, 65) and (s2, e2) == (20, 30 + 36 + 30 + 19)
    assert sm.second(read, ref, (1, 5, 7, 2), 14)[2:] == (0, -1)
    assert sm.second(read, ref, (1, 5, 7, 2), 4000)[2:] == (0, 0)
    assert sm.second(read, "", (1, 5, 7, 2), 18) == (0, -1, 0, 0)
    assert sm.mask_len_of("A" * 30) == 15 and sm.mask_len_of("A" * 31) == 15 and sm.mask_len_of("A" * 32) == 16


def test_second_header_symbols_all_exported():
    """include/tredsecond.h: every declared entry point is exported by libtredgpu.so and listed in _lib.SECOND_EXPORTS."""
    lib = _lib.load()
    src = open(os.path.join(ROOT, "include", "tredsecond.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(tredsecond_[a-z_]+)\s*\(", src)))
    assert names == sorted(_lib.SECOND_EXPORTS) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r" T (tredsecond_[a-z_]+)", out)) == set(names)
    assert (_lib.SECOND_OK, _lib.SECOND_TOO_LONG, _lib.SECOND_BAD_ITEM, _lib.KERNEL_SECOND) == (0, 4, 5, 18)
    for name, value in re.findall(r"#define TREDGPU_(SECOND_[A-Z_]+|KERNEL_SECOND) (\d+)", src):
        assert getattr(_lib, name) == int(value), name


def test_the_texts_of_a_result_with_a_second_best():
    rec = [40, 30, 69, 0, 39]
    plain = ssw.PyAlignRes(rec, "A" * 40, "C" * 100)
    assert plain.score2 is None and plain.ref_end2 is None and "SUB-OPTIMAL" not in str(plain)
    a = ssw.PyAlignRes(rec, "A" * 40, "C" * 100, (40 << 4,), second=(19, 48))
    assert (a.score2, a.ref_end2) == (19, 48)
    assert str(a) == str(plain) + "Cigar_string     40M\nSUB-OPTIMAL MATCH\nScore 2           19\nRef_end2          48\n"
    none = ssw.PyAlignRes(rec, "A" * 40, "C" * 100, second=(0, 0))
    assert (none.score2, none.ref_end2) == (0, 0) and str(none) == str(plain)           # the reference prints it only if non-zero
