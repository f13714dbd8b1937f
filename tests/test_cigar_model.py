"""CPU: tests/cigar_model.py -- the plain-Python restatement of the reference's banded_sw -- against the CIGARs the
compiled reference gave (tests/golden/sw_cigar.npz, tools/gen_golden_cigar.py), and the text helpers of
tredparse_amd.ssw.PyAlignRes against the reference's own cigar_string / alignment / str()."""
import numpy as np

from . import cigar_model as cm
from tredparse_amd.ssw import PyAlignRes


def test_golden_set_is_what_the_generator_promises():
    g = cm.golden()
    kept = g["meta"]["kept"]
    assert kept["a"] == 100 and g["meta"]["excluded"].get("a", 0) == 0
    assert all(kept[c] >= 10 for c in "cdef") and len(g["reads"]) == sum(kept.values()) >= 400
    lens = {len(r) for r, c in zip(g["reads"], g["cls"]) if c == "b"}
    assert {36, 100, 150, 250, 480} <= lens
    n_ops = [len(o) for o in g["ops"]]
    assert max(n_ops) >= 5 and min(n_ops) == 1
    # the extremes: the 480 x 511 item and the single-M item of 15 bases
    assert any(len(r) == 480 and len(t) == 511 for r, t in zip(g["reads"], g["refs"]))
    assert [15 << 4] in [o for o, r in zip(g["ops"], g["reads"]) if len(r) == 15]


def test_model_reproduces_every_golden_cigar():
    g = cm.golden()
    for k, (ref, read, f, want) in enumerate(zip(g["refs"], g["reads"], g["fields"], g["ops"])):
        status, ops = cm.cigar_of(ref, read, f)
        assert status == cm.OK and ops == want, (k, g["cls"][k], status, ops, want)


def test_golden_operations_consume_the_rectangle_and_rescore():
    g = cm.golden()
    for k, (ref, read, f, ops) in enumerate(zip(g["refs"], g["reads"], g["fields"], g["ops"])):
        assert cm.consumed(ops) == (f[4] - f[3] + 1, f[2] - f[1] + 1), k
        assert cm.rescore(ref, read, f, ops) == f[0], k


SCORINGS = ((2, 2, 3, 1), (1, 1, 2, 1), (1, 4, 6, 1), (3, 5, 7, 2), (4, 9, 10, 10), (8, 16, 16, 16), (1, 0, 1, 1), (1, 5, 7, 7))


def test_scoring_goldens_are_what_the_generator_promises():
    g = cm.golden_scorings()
    meta = g["meta"]
    assert set(g["scoring"]) == set(SCORINGS) and meta["scorings"] == ["/".join(map(str, s)) for s in SCORINGS]
    for s in SCORINGS:
        text = "/".join(map(str, s))
        ks = [k for k, v in enumerate(g["scoring"]) if v == s]
        assert len(ks) == meta["kept"][text] >= 55
        assert meta["excluded"][text] <= 0.02 * (meta["kept"][text] + meta["excluded"][text])
        assert {g["cls"][k] for k in ks} == set("bcde")
        lens = [len(g["reads"][k]) for k in ks]
        assert min(lens) <= 36 and max(lens) == 250
        assert sum(1 for k in ks if any(v & 15 for v in g["ops"][k])) >= 10, text             # items with a gap
        assert sum(1 for k in ks if len(g["ops"][k]) > 3) >= 10, text
    assert len(g["cigar_string"]) == len(g["reads"])


def test_model_reproduces_every_golden_cigar_at_its_scoring():
    g = cm.golden_scorings()
    for k, (ref, read, f, want, s) in enumerate(zip(g["refs"], g["reads"], g["fields"], g["ops"], g["scoring"])):
        status, ops = cm.cigar_of(ref, read, f, *s)
        assert status == cm.OK and ops == want, (k, s, g["cls"][k], status, ops, want)
        assert cm.consumed(ops) == (f[4] - f[3] + 1, f[2] - f[1] + 1), (k, s)
        assert cm.rescore(ref, read, f, ops, *s) == f[0], (k, s)
        al = PyAlignRes(f, read, ref, ops)
        assert al.cigar_string == g["cigar_string"][k], (k, s)


def test_bands_helper_and_predicted_tier():
    """bands_of / is_wide: the band starts at |refLen - readLen| + 1 and doubles up to the rectangle's cover; the limits are
    the kernel's own constants."""
    row, plane = cm.narrow_limits()
    assert row >= 8 and plane >= 1024
    ref = "ACGTTGCAAGCTTAGGCTAACGTAGCTAGGATCCGATTACA" * 3
    read = ref[5:65]
    assert cm.bands_of(ref, read, (30, 5, 64, 0, 59)) == [1]
    assert cm.bands_of(ref, read, (30, 5, 74, 0, 59)) == [11]
    assert cm.bands_of(ref, read, (999, 5, 64, 0, 59)) == [1, 2, 4, 8, 16, 32, 59]             # NO_PATH at full cover
    st, ops, passes = cm.passes_of(ref, read, (999, 5, 64, 0, 59))
    assert (st, ops) == (cm.NO_PATH, []) and [b for _, b in passes] == [60] * 7
    top = (row - 4) // 2                                    # the widest band whose 2 * band + 3 entries fit a row of row - 1
    fit = plane // (2 * top + 1)
    assert not cm.is_wide([1, 2, top], fit) and cm.is_wide([top], fit + 1) and cm.is_wide([1, 2, top + 1], 10)
    assert not cm.is_wide([1], plane // 3) and cm.is_wide([1], plane // 3 + 1)


def test_band_doubles_for_compensating_indels():
    """Class d: refLen == readLen, so the band starts at 1; a 3-base deletion and a 3-base insertion need it at 4."""
    g = cm.golden()
    n = 0
    for ref, read, f, ops, c in zip(g["refs"], g["reads"], g["fields"], g["ops"], g["cls"]):
        if c == "d" and f[2] - f[1] == f[4] - f[3] and {v & 15 for v in ops} == {0, 1, 2}:
            n += 1
            assert max(v >> 4 for v in ops if v & 15) in (3, 6)
    assert n >= 10


def test_unreachable_score_is_no_path_not_a_walk_off_the_buffers():
    g = cm.golden()
    f = np.array(g["fields"][0])
    f[0] += 40                                     # a score the rectangle cannot give
    assert cm.cigar_of(g["refs"][0], g["reads"][0], f) == (cm.NO_PATH, [])


def test_text_helpers_give_the_references_text():
    g = cm.golden()
    for k, t in enumerate(g["texts"]):
        al = PyAlignRes(g["fields"][k], g["reads"][k], g["refs"][k], g["ops"][k])
        assert al.cigar_string == al.cigar == t["cigar_string"], k
        assert list(al.alignment) == t["alignment"], k
        assert str(al) == t["str"], k
        assert [(n, op) for n, op in al.iter_cigar] == [(v >> 4, "MID"[v & 15]) for v in g["ops"][k]]
    empty = PyAlignRes(g["fields"][0], g["reads"][0], g["refs"][0])
    assert empty.cigar_string == "" and empty.alignment == ("", "", "") and empty.score2 is None
    assert "Cigar_string" not in str(empty) and str(empty).startswith("OPTIMAL MATCH\nScore            ")


def test_cigar_header_symbols_all_exported():
    """include/tredcigar.h: every declared entry point is exported by libtredgpu.so and listed in _lib.CIGAR_EXPORTS."""
    import os
    import re
    import subprocess
    from tredparse_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "tredcigar.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tredcigar_[a-z_]+)\s*\(", src)))
    assert names == sorted(_lib.CIGAR_EXPORTS) and len(names) == 5
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r" T (tredcigar_[a-z_]+)", out)) == set(names)
    assert (_lib.CIGAR_NO_PATH, _lib.CIGAR_OFF_EDGE, _lib.CIGAR_OVERFLOW) == (cm.NO_PATH, cm.OFF_EDGE, cm.OVERFLOW)
    assert _lib.KERNEL_CIGAR == int(re.search(r"#define TREDGPU_KERNEL_CIGAR (\d+)", src).group(1))
