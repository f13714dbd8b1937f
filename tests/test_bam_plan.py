"""CPU: the tables of the BAM layer (csrc/bamread.cpp behind bamio.NativeAlignmentFile) are pinned byte for byte.

tests/golden/bam_plan.json (tools/gen_golden_bam_plan.py) holds a SHA-256 of everything the plan / scan family hands out
for the committed BAMs -- t001, t002 and synf through their .bai, t001 and synf again through a CSI-only copy at min_shift
14: plan, plan_blocks, the tasks and chunks of the three walk planners, what plan_fill writes, the units and pools of scan,
scan(pe=...) and scan(pe=..., alt=...).  The test recomputes them with the generator's own function.  Then the -3 contract
of the planners straight at the library, and the whole family once more in a stand-alone program (tests/bam_plan_main.cpp)
built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tredparse_amd import bamio
from tredparse_amd.bam_parser import _site_arrays, y_regions
from tredparse_amd.meta import TREDsRepo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))

needs_native = pytest.mark.skipif(bamio._native() is None, reason="no native BAM layer")


def _hd_window(repo):
    """A plain region with records in t001 (its reads lie at HD; none on chrY)."""
    t = repo["HD"]
    return (t.chr, t.repeat_start - 1000, t.repeat_end + 1000)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    import gen_golden_bam_plan as gen
    return gen, gen.committed_cases(str(tmp_path_factory.mktemp("bam_plan")))


@needs_native
def test_tables_equal_the_pinned_hashes(cases):
    gen, found = cases
    want = json.load(open(os.path.join(GOLD, "bam_plan.json")))["tables"]
    assert sorted(want) == sorted(c[0] for c in found) and len(want) == 5
    for case, path, repo, names in found:
        got = gen.table_hashes(path, repo, names)
        assert sorted(got) == sorted(want[case]), case
        assert [k for k in sorted(got) if got[k] != want[case][k]] == [], case


@needs_native
def test_the_pinned_tables_are_not_empty(cases):
    """Guard against hashes of nothing: on t001 the plan holds blocks, every planner writes chunks that start in planned
    blocks, and the scan selects reads and pair lengths."""
    _, found = cases
    case, path, repo, names = found[0]
    f = bamio.NativeAlignmentFile(path)
    sites, alts = _site_arrays(repo, names, [repo[n] for n in names], f)
    readlen = f.max_read_len(101)
    y = [_hd_window(repo)]                               # (t001 has no reads on chrY)
    assert f.plan(sites, alts, readlen, extra=y_regions(repo.ref) + y)[0] > 0
    for tasks, chunks in (f.plan_walks(sites, readlen), f.plan_alt_walks(sites, alts, readlen), f.plan_region_walks(y)):
        assert (tasks["n_chunks"] > 0).any() and len(chunks) > 0 and (chunks["begin_block"] >= 0).any()
    units, pools = f.scan(sites, alts, readlen)
    assert units["n_reads"].sum() > 0 and len(pools["global_lens"]) > 0 and len(pools["packed"]) > 0
    f.close()


@needs_native
def test_minus_three_exactly_when_the_chunks_do_not_fit(cases):
    """Straight at the library: with cap_chunks equal to the count a planner returned it returns that count, with one
    less -3 -- after a plan and, with every begin_block -1, before any."""
    _, found = cases
    lib = bamio._native()
    for case, path, repo, names in found[:1] + found[3:4]:           # t001 through its .bai and through the .csi
        f = bamio.NativeAlignmentFile(path)
        sites, alts = _site_arrays(repo, names, [repo[n] for n in names], f)
        ys = np.array([(f.tid(c), lo, hi) for c, lo, hi in y_regions(repo.ref) + [_hd_window(repo)]], bamio.REGION_DTYPE)
        o = bamio.ScanOpts(f.max_read_len(101), 1000, 9, 10000, 1000, 1, 1, 1)
        tasks = np.zeros(max(len(sites), len(alts), len(ys)), bamio.WALK_TASK_DTYPE)
        chunks = np.zeros(1 << 16, bamio.WALK_CHUNK_DTYPE)
        planners = [
            lambda cap: lib.tredbam_plan_walks(f._h, sites.ctypes.data, len(sites), C.byref(o), tasks.ctypes.data, chunks.ctypes.data, cap),
            lambda cap: lib.tredbam_plan_alt_walks(f._h, sites.ctypes.data, len(sites), alts.ctypes.data, len(alts), C.byref(o),
                                                   tasks.ctypes.data, chunks.ctypes.data, cap),
            lambda cap: lib.tredbam_plan_region_walks(f._h, ys.ctypes.data, len(ys), tasks.ctypes.data, chunks.ctypes.data, cap)]
        for planned in (False, True):
            if planned:
                f.plan(sites, alts, o.readlen, extra=y_regions(repo.ref) + [_hd_window(repo)])
            for call in planners:
                n = call(len(chunks))
                assert 0 < n < len(chunks), case
                assert call(n) == n and call(n - 1) == -3 and call(0) == -3, case
                assert call(len(chunks)) == n
                held = chunks["begin_block"][:n] >= 0
                assert held.any() if planned else not held.any(), case
        f.close()


def test_plan_family_under_the_sanitizers(tmp_path):
    """tests/bam_plan_main.cpp with bamread.cpp and emit.cpp, address and undefined-behaviour sanitizers on, over t001.bam
    and all loci of the no_sites repository: exit 0, nothing reported, and the counts it prints are the binding's."""
    csrc = os.path.join(ROOT, "tredparse_amd", "csrc")
    exe = str(tmp_path / "bam_plan_main")
    cxx = ["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    srcs = [os.path.join(HERE, "bam_plan_main.cpp"), os.path.join(csrc, "bamread.cpp"), os.path.join(csrc, "emit.cpp")]
    objs = [str(tmp_path / "{}.o".format(k)) for k in range(len(srcs))]
    jobs = [subprocess.Popen(cxx + ["-I", os.path.join(ROOT, "include"), "-c", s, "-o", o]) for s, o in zip(srcs, objs)]
    assert [j.wait() for j in jobs] == [0] * len(jobs)               # (side by side: bamread.cpp alone takes most of the time)
    subprocess.check_call(cxx + ["-o", exe] + objs + ["-lz"])
    repo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
    strip = "nochr" in repo.ref
    args = []
    for n in sorted(repo.names):
        t = repo[n]
        args.append("@".join(["{}:{}:{}".format(t.chr, t.repeat_start, t.repeat_end)] +
                             ["{}:{}:{}".format(c[3:] if strip else c, a, b) for c, a, b in t.alt]))
    bam = os.path.join(GOLD, "bam", "t001.bam")
    args += ["+{}:{}:{}".format(*g) for g in y_regions(repo.ref) + [_hd_window(repo)]]
    r = subprocess.run([exe, bam] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr            # the sanitizers report nothing
    out = r.stdout.splitlines()
    assert out[-1] == "closed" and sum(1 for line in out if line.startswith("scan_pe refused: pair-length slices of site 0")) == 1
    for when, held in (("unplanned", False), ("planned", True), ("cleared", False)):
        lines = [line.split() for line in out if line.startswith(when + " ")]
        assert [l[1] for l in lines] == ["walks", "alt_walks", "region_walks"]
        for l in lines:
            assert int(l[3]) > 0 and (int(l[5]) > 0) == held, l
    if bamio._native() is not None:                                  # the same counts through the binding
        f = bamio.NativeAlignmentFile(bam)
        names = sorted(repo.names)
        sites, alts = _site_arrays(repo, names, [repo[n] for n in names], f)
        plan = f.plan(sites, alts, 150, extra=y_regions(repo.ref) + [_hd_window(repo)])
        assert "plan {} {} {}".format(*plan) in out
        want = [len(f.plan_walks(sites, 150)[1]), len(f.plan_alt_walks(sites, alts, 150)[1])]
        assert [int(line.split()[3]) for line in out if line.startswith("planned ")][:2] == want
        _, pools = f.scan(sites, alts, 150)
        assert "scan reads {} global {} target {}".format(len(pools["read_len"]), len(pools["global_lens"]), len(pools["target_lens"])) in out
        f.close()
