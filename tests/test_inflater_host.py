"""CPU: tredparse_amd/csrc/inflater_host.h, the host arithmetic of inflater_api.hip, through the stand-alone driver
tests/inflater_host_main.cpp built with the address and undefined-behaviour sanitizers: how the buffers grow, what a call's
offsets, tasks and chunks must satisfy (with the refusals' texts), the record room and the name table of a walk, the runs
a fetch copies, and where the parts of the packed arrays lie.  The expected values are written out here, from the rules."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCKS = "block offsets: payloads start on 4-byte boundaries, ascend, and inflate to at most 64 KiB each"
BEYOND = "offsets beyond the reserved buffers"
TASK = "walk task outside its chunks / blocks"
CHUNK = "walk chunk starts outside a block"
GAP = 128 * 1024
# (past_need, past_cap) of: the staging, the per-block arrays, the walk's tables and device pools, the selection's places and
# the fetch pieces, the pinned pools, the fetched blocks
STAGING, PER_BLOCK, WALK, LISTS, HOST_POOLS, DENSE = (16, 8), (16, 2), (8, 2), (0, 2), (8, 8), (0, 8)
TASK_BYTES, CHUNK_BYTES, RESULT_BYTES, ALT_RESULT_BYTES, SELECT_TASK_BYTES, SELECT_RESULT_BYTES = 48, 16, 48, 56, 16, 32


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflater_host") / "inflater_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "inflater_host_main.cpp")])

    def call(*args):
        flat = []
        for a in args:
            flat += [str(x) for x in a] if isinstance(a, (list, tuple)) else [str(a)]
        r = subprocess.run([exe] + flat, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr        # the sanitizers report nothing
        return r.stdout.splitlines()
    return call


def test_struct_sizes_match_the_binding():
    from tredparse_amd import _lib
    assert [d.itemsize for d in (_lib.WALK_TASK_DTYPE, _lib.WALK_CHUNK_DTYPE, _lib.WALK_RESULT_DTYPE, _lib.ALT_RESULT_DTYPE,
                                 _lib.SELECT_TASK_DTYPE, _lib.SELECT_RESULT_DTYPE)] == \
        [TASK_BYTES, CHUNK_BYTES, RESULT_BYTES, ALT_RESULT_BYTES, SELECT_TASK_BYTES, SELECT_RESULT_BYTES]


# max(need + need / past_need, cap + cap / past_cap), integer divisions, 0: no slack on that side
@pytest.mark.parametrize("need,cap,slack,want", [
    (1000, 0, STAGING, 1062), (1000, 0, PER_BLOCK, 1062), (1000, 0, WALK, 1125), (1000, 0, LISTS, 1000),
    (1000, 0, HOST_POOLS, 1125), (1000, 0, DENSE, 1000),
    (1000, 960, STAGING, 1080), (1000, 960, PER_BLOCK, 1440), (1000, 960, WALK, 1440), (1000, 960, LISTS, 1440),
    (1000, 960, HOST_POOLS, 1125), (1000, 960, DENSE, 1080),
    (1001, 7, WALK, 1126), (9, 0, WALK, 10), (7, 3, LISTS, 7), (7, 6, LISTS, 9),         # (the divisions round down)
    # need == cap: the rule itself would grow -- that a call of the same size allocates nothing is grow()'s `need <= cap`
    (1000, 1000, STAGING, 1125), (1000, 1000, LISTS, 1500), (1000, 1000, DENSE, 1125),
    (15, 0, STAGING, 15), (16, 0, STAGING, 17), (300000064, 0, STAGING, 318750068), (300000064, 290000000, STAGING, 326250000),
])
def test_next_cap(run, need, cap, slack, want):
    assert run("N", need, cap, *slack) == [str(want)]


def test_check_blocks(run):
    coff, ooff, big = [0, 100, 200], [0, 65280, 130560], 1 << 20

    def B(c=coff, o=ooff, cap_comp=big, cap_out=big):
        return run("B", cap_comp, cap_out, len(c) - 1, c, o)
    assert B() == ["ok"]
    assert B(c=[0, 102, 200]) == [BLOCKS]                       # a payload off its 4-byte boundary
    assert B(c=[0, 100, 202]) == ["ok"]                         # (the end of the last payload need not be on one)
    assert B(c=[-4, 100, 200]) == [BLOCKS]
    assert B(c=[0, 200, 100]) == [BLOCKS]                       # descending
    assert B(o=[0, 65280, 65000]) == [BLOCKS]
    assert B(o=[-1, 65280, 130560]) == [BLOCKS]
    assert B(o=[0, 65536, 131072]) == ["ok"]
    assert B(o=[0, 65537, 131072]) == [BLOCKS]                  # a block of 65 537 bytes
    assert B(o=[0, 65280, 130817]) == [BLOCKS]
    # the buffers hold 64 bytes beyond the last offset
    assert B(cap_comp=200 + 64) == ["ok"] and B(cap_comp=200 + 63) == [BEYOND]
    assert B(cap_out=130560 + 64) == ["ok"] and B(cap_out=130560 + 63) == [BEYOND]
    assert B(c=[0, 102, 200], cap_comp=10) == [BLOCKS]          # the blocks are looked at first
    assert run("B", 64, 64, 0, [0], [0]) == ["ok"] and run("B", 64, 63, 0, [0], [0]) == [BEYOND]


def test_check_tasks_and_chunks(run):
    def T(*tasks):                                              # 6 blocks, 4 chunks; (chunk_first, n_chunks, block_first, block_end)
        return run("T", 6, 4, len(tasks), *tasks)
    assert T() == ["ok"] and T((0, 4, 0, 6), (3, 1, 6, 6), (4, 0, 0, 0)) == ["ok"]
    assert T((-5, -1, 9, 2)) == ["ok"]                          # not planned: accepted whatever else it holds
    assert T((0, 4, 0, 6), (7, -3, -1, -2)) == ["ok"]
    assert T((3, 2, 0, 6)) == [TASK] and T((5, 0, 0, 6)) == [TASK]      # one past the chunk list
    assert T((-1, 1, 0, 6)) == [TASK]
    assert T((0, 1, 0, 7)) == [TASK]                            # block_end = n_blocks + 1
    assert T((0, 1, -1, 6)) == [TASK]
    assert T((0, 1, 4, 3)) == [TASK]                            # block_first > block_end
    assert T((0, 4, 0, 6), (0, 1, 4, 3)) == [TASK]              # (the second task)
    assert run("T", 6, 0, 1, (2147483647, 2147483647, 0, 6)) == [TASK]  # (the sum does not wrap)
    assert run("C", 0) == ["ok"] and run("C", 3, 0, 65536, 12) == ["ok"]
    assert run("C", 1, -1) == [CHUNK] and run("C", 2, 0, 65537) == [CHUNK]


def test_plan_walk(run):
    # 6 blocks at 0, 100, 200 ... in their file, 65 280 bytes each; a chunk is (begin_block, the file offset its end lies at)
    a = (0, 1, 0, 6)              # its chunk ends inside block 2: blocks 0 .. 2, 3 * 65 280 / 64 records and 64 more
    b = (1, 1, 2, 6)              # its chunk begins at block 1, outside [2, 6): skipped, but planned: the 64 alone
    c = (0, -1, 0, 6)             # not planned: no room
    chunks = [(0, 200), (1, 400)]
    assert run("P", 6, 100, 65280, 3, a, b, c, len(chunks), *chunks) == ["0 3124 3188 3188 | 3188 0"]
    assert 3 * 65280 // 64 + 64 == 3124
    assert run("P", 6, 100, 65280, 0, 0) == ["0 | 0 0"]
    # a chunk that ends beyond the task's blocks stops at block_end; one that ends before its begin block spans nothing
    assert run("P", 6, 100, 65280, 2, (0, 1, 0, 4), (1, 1, 0, 6), 2, (2, 9999), (3, 100)) == ["0 2104 2168 | 2168 0"]
    # two chunks add up; an empty task (n_chunks = 0) gets no room
    assert run("P", 6, 100, 65280, 2, (0, 2, 0, 6), (2, 0, 0, 6), 2, (0, 0), (4, 500)) == ["0 3124 3124 | 3124 0"]
    # 50 blocks: a task of 40 blocks keeps the small table, one of 41 beside it asks for the large one
    forty, forty_one = (0, 1, 0, 50), (1, 1, 0, 50)
    assert run("P", 50, 100, 65280, 1, forty, 1, (0, 3900)) == ["0 40864 | 40864 0"]
    assert run("P", 50, 100, 65280, 2, forty, forty_one, 2, (0, 3900), (5, 4500)) == ["0 40864 82748 | 82748 1"]
    assert 40 * 65280 // 64 + 64 == 40864 and 41 * 65280 // 64 + 64 == 41884
    # (the blocks of a task's chunks add up: 2 * 21 blocks)
    assert run("P", 50, 100, 65280, 1, (0, 2, 0, 50), 2, (0, 2000), (25, 4500))[0].endswith("| 42904 1")


def test_wanted_runs_and_dense_off(run):
    def W(need, sizes, gap=GAP):
        ooff = [sum(sizes[:k]) for k in range(len(sizes) + 1)]
        return run("W", gap, len(need), need, ooff)
    assert W([], []) == ["| 0 | 0"]
    assert W([0, 0, 0], [100, 200, 300]) == ["| 0 0 0 0 | 0"]                       # no wanted block
    assert W([1, 1, 1], [100, 200, 300]) == ["0-2 | 0 100 300 600 | 600"]           # all of them: one run
    assert W([0, 0, 1], [100, 200, 300]) == ["2-2 | 0 0 0 300 | 300"]               # the last block
    assert W([1, 0, 0], [100, 200, 300]) == ["0-0 | 0 100 100 100 | 100"]
    # exactly GAP bytes between two wanted blocks: one run, the blocks between them are copied too
    assert W([1, 0, 0, 1], [1000, 65536, 65536, 500]) == ["0-3 | 0 1000 66536 132072 132572 | 132572"]
    # one byte more: two runs, and the unwanted blocks are empty (dense_off[k + 1] == dense_off[k])
    assert W([1, 0, 0, 0, 1], [1000, 65536, 65536, 1, 500]) == ["0-0 4-4 | 0 1000 1000 1000 1000 1500 | 1500"]
    assert W([1, 0, 1], [10, 20, 30], gap=19) == ["0-0 2-2 | 0 10 10 40 | 40"] and W([1, 0, 1], [10, 20, 30], gap=20)[0].startswith("0-2 ")
    # a run goes on from its LAST wanted block: 0, 2 and 4 are joined pairwise; trailing unwanted blocks are left out
    assert W([1, 0, 1, 0, 1, 0], [10, 20, 10, 20, 10, 5], gap=20) == ["0-4 | 0 10 30 40 60 70 70 | 70"]


@pytest.mark.parametrize("nb,n_tasks,n_chunks,n_alt", [(5, 3, 7, 2), (1, 1, 1, 0), (3, 0, 0, 0), (4097, 481, 1023, 37)])
def test_layouts(run, nb, n_tasks, n_chunks, n_alt):
    got = [[int(x) for x in part.split()] for part in run("L", nb, n_tasks, n_chunks, n_alt)[0].split("|")]
    rb_at = n_tasks * TASK_BYTES + n_chunks * CHUNK_BYTES
    assert got[0] == [nb * 8, nb * 12, nb * 16]
    assert got[1] == [n_tasks * TASK_BYTES, rb_at, rb_at + (n_tasks + 1) * 8]
    assert got[2] == [n_tasks * RESULT_BYTES, n_tasks * RESULT_BYTES + 16]
    assert got[3] == [n_alt * ALT_RESULT_BYTES, n_alt * ALT_RESULT_BYTES + nb]
    assert got[4] == [n_tasks * SELECT_TASK_BYTES, n_tasks * (SELECT_TASK_BYTES + SELECT_RESULT_BYTES)]
    # parts of 8-byte entries (the chunks, rec_base, the counters, the select results) lie on 8-byte boundaries, the 4-byte ones on 4
    assert all(v % 8 == 0 for v in (got[1][0], got[1][1], got[2][0], got[4][0])) and got[0][0] % 4 == 0 and got[0][1] % 4 == 0
