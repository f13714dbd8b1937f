"""The long-read path's host side (no GPU): admit() bounds with the switch on, and the --long-reads flag from the
command line to the --gpus children."""
import os

from tredparse_amd import bam_parser, shard, tred as tredmod
from tredparse_amd.bam_parser import scan_sample
from tredparse_amd.meta import TREDsRepo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAM1 = os.path.join(GOLD, "bam", "t001.bam")


def test_admit_with_long_reads_keeps_long_units():
    repo = TREDsRepo("hg38")
    s = scan_sample(BAM1, repo, ["SCA1", "HD", "DM1"], long_reads=True)
    assert s.long_reads and not s.dropped
    a, _ = s.reads_of(1)
    s.read_len[a] = 500                                # beyond the short kernels' 480 bp: kept
    assert not bam_parser.admit(s)
    s.read_len[a] = 2048
    assert not bam_parser.admit(s)
    s.read_len[a] = 2049                               # beyond the long kernel: dropped, its unit only
    assert list(bam_parser.admit(s)) == [1] and "2049 bp" in s.dropped[1]
    s.read_len[a] = 150
    s.readlen = 500                                    # ladders of 36 + 3 * 167 columns: kept
    assert not bam_parser.admit(s)
    s.readlen = 2048
    assert not bam_parser.admit(s)
    # the same scan without the switch drops what it drops today
    off = scan_sample(BAM1, repo, ["SCA1", "HD", "DM1"])
    assert not off.long_reads
    off.read_len[a] = 500
    assert list(bam_parser.admit(off)) == [1] and "500 bp" in off.dropped[1]


def test_long_reads_flag_parses_and_reaches_the_children(tmp_path, monkeypatch):
    made, runs, cmds = [], [], []

    class Eng(object):
        def __init__(self, device=0, long_reads=False):
            made.append(long_reads)

        def close(self):
            pass

    monkeypatch.setattr("tredparse_amd.engine.Engine", Eng)
    monkeypatch.setattr(tredmod, "run_many", lambda *a, **kw: runs.append(kw.get("long_reads")))

    def fake_spawn(cmd, world, devices, env=None, cwd=None, **kw):
        cmds.append(list(cmd))
        for r in range(world):
            for k, v in (("RANK", str(r)), ("WORLD_SIZE", str(world)), ("TRED_SPAWNED_RANK", "1")):
                monkeypatch.setenv(k, v)
            tredmod.main(cmd[3:], quiet=True)
        for k in ("RANK", "WORLD_SIZE", "TRED_SPAWNED_RANK"):
            monkeypatch.delenv(k)
        return [0] * world

    monkeypatch.setattr(shard, "spawn_ranks", fake_spawn)
    monkeypatch.setattr(shard, "visible_gpus", lambda: 2)
    monkeypatch.chdir(tmp_path)
    bams = [BAM1, os.path.join(GOLD, "bam", "t002.bam")]
    (tmp_path / "samples.csv").write_text("".join("c{},{}\n".format(i, bams[i % 2]) for i in range(3)))
    tredmod.main(["samples.csv", "--workdir", str(tmp_path / "work"), "--gpus", "2", "--tred", "HD", "--long-reads"])
    assert cmds and all("--long-reads" in c for c in cmds)
    assert made == [True, True] and runs == [True, True]
    # without the flag: neither the engine nor run_many is asked for the path
    made.clear(); runs.clear(); cmds.clear()
    tredmod.main(["samples.csv", "--workdir", str(tmp_path / "work2"), "--gpus", "2", "--tred", "HD"])
    assert cmds and not any("--long-reads" in c for c in cmds)
    assert made == [False, False] and runs == [False, False]


def test_long_path_symbols_exported():
    """include/tredlong.h: every declared entry point is exported by libtredgpu.so (and listed in _lib.LONG_EXPORTS)."""
    import re
    import subprocess
    from tredparse_amd import _lib
    src = open(os.path.join(os.path.dirname(GOLD), "..", "include", "tredlong.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(tredlong_[a-z_]+)\s*\(", src)))
    assert names == sorted(_lib.LONG_EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r" T (tredlong_[a-z_]+)", out)) == set(names)
