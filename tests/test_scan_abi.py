"""include/tredscan.h and the library: every entry point is exported and listed in _lib.SCAN_EXPORTS, the constants of
header, binding and model agree, and the unit added nothing under the prefixes whose export sets are pinned."""
import os
import re
import subprocess

from tredparse_amd import _lib

from . import scan_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_scan_header_symbols_all_exported():
    lib = _lib.load()
    src = _header("tredscan.h")
    names = sorted(set(re.findall(r"\b(tredscan_[a-z_]+)\s*\(", src)))
    assert names == sorted(_lib.SCAN_EXPORTS) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r" T (tredscan_[a-z_]+)", out)) == set(names)
    defines = dict(re.findall(r"#define (TRED[A-Z_]+) (\d+)", src))
    assert int(defines["TREDGPU_KERNEL_SCAN"]) == _lib.KERNEL_SCAN == 22
    assert int(defines["TREDSCAN_MAX_PERIOD"]) == _lib.SCAN_MAX_PERIOD == sm.MAX_PERIOD == 6
    assert int(defines["TREDSCAN_TILE"]) == _lib.SCAN_TILE
    assert int(defines["TREDSCAN_MAX_LETTERS"]) == _lib.SCAN_MAX_LETTERS >= 1 << 28       # one human chromosome is one call
    assert _lib.SCAN_MAX_LETTERS + 6 < 1 << 31                                            # out_len is an int32
    assert tuple(_lib.SCAN_MIN_COPIES) == tuple(sm.MIN_COPIES) and min(_lib.SCAN_MIN_COPIES) >= 2
    assert ("tredscan", "tredscan_get_timing", "tredscan_reset_timing", 22, "tredscan_last_error") in _lib.SIDE_UNITS


def test_scan_unit_adds_no_pinned_symbol():
    """tests/test_abi.py pins the exact export sets of tredgpu_* and tredbam_* (tredgpu.h is the ABI of the kernels the
    profiles were taken from, tredbam.h the host BAM layer's): the scan lives under tredscan_ alone, its FASTA handling is
    Python, and the source hash in tredgpu_version does not see csrc/scan.hip."""
    gpu = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r" T (tredgpu_[a-z_]+)", gpu)) == set(_lib.EXPORTS)
    bam = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.HERE, "libtredbam.so")]).decode()
    declared = set(re.findall(r"\b(tredbam_[a-z0-9_]+)\s*\(", _header("tredbam.h")))
    assert set(re.findall(r" T (tredbam_[a-z0-9_]+)", bam)) == declared
    assert not re.search(r"fasta|repeat", " ".join(sorted(declared) + list(_lib.EXPORTS)), re.I)
    make = open(os.path.join(_lib.HERE, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", make, re.M).group(1).split()
    side = re.search(r"^SIDE_SRCS := (.*)$", make, re.M).group(1).split()
    hdrs = re.search(r"^HDRS := (.*)$", make, re.M).group(1)
    assert "scan.hip" in side and "scan.hip" not in srcs and "tredscan.h" not in hdrs
