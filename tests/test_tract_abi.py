"""include/tredtract.h and the library: every entry point is exported and listed in _lib.TRACT_EXPORTS, the constants of
header, binding and model agree, and the unit is a side unit outside the source hash."""
import os
import re
import subprocess

from tredparse_amd import _lib

from . import scan_model as sm
from . import tract_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_tract_header_symbols_all_exported():
    lib = _lib.load()
    src = _header("tredtract.h")
    names = sorted(set(re.findall(r"\b(tredtract_[a-z_]+)\s*\(", src)))
    assert names == sorted(_lib.TRACT_EXPORTS) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r" T (tredtract_[a-z_]+)", out)) == set(names)
    assert not re.findall(r"\b(tred(?:scan|gpu|bam)_[a-z0-9_]+)\s*\(", src)           # nothing under the pinned prefixes
    defines = dict(re.findall(r"#define (TRED[A-Z_]+) (\d+)", src))
    assert int(defines["TREDGPU_KERNEL_TRACT"]) == _lib.KERNEL_TRACT == 23
    assert int(defines["TREDTRACT_MAX_GAP"]) == _lib.TRACT_MAX_GAP == tm.MAX_GAP_LIMIT == 64
    assert tuple(_lib.TRACT_SEED_COPIES) == tuple(tm.SEED_COPIES) == (5, 3, 3, 3, 3, 3)
    assert tuple(_lib.TRACT_MAX_GAP_DEFAULT) == tuple(tm.MAX_GAP) == (1, 2, 3, 4, 5, 6)
    assert tm.rule_violation(_lib.SCAN_MIN_COPIES, _lib.TRACT_SEED_COPIES, _lib.TRACT_MAX_GAP_DEFAULT) is None
    assert tm.MAX_PERIOD == _lib.SCAN_MAX_PERIOD == sm.MAX_PERIOD
    assert ("tredtract", "tredtract_get_timing", "tredtract_reset_timing", 23, "tredtract_last_error") in _lib.SIDE_UNITS
    assert len({unit[3] for unit in _lib.SIDE_UNITS}) == len(_lib.SIDE_UNITS)         # one selector per unit


def test_tract_unit_is_a_side_unit():
    make = open(os.path.join(_lib.HERE, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    side = re.search(r"^SIDE_SRCS := (.*)$", make, re.M).group(1).split()
    hdrs = re.search(r"^HDRS := (.*)$", make, re.M).group(1)
    assert "tract.hip" in side and "tract.hip" not in srcs and "scan.hip" in side
    assert "tredtract.h" not in hdrs and "scan_unit.h" not in hdrs
    for unit in ("scan.hip", "tract.hip"):                                             # the two scans share their device code
        assert '#include "scan_unit.h"' in open(os.path.join(_lib.HERE, "csrc", unit)).read()
