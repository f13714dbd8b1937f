"""GPU: what the device front end's entry points (csrc/inflater_api.hip: tredgpu_inflate_blocks_crc, tredgpu_inflate_walk,
tredgpu_inflater_fetch[_dense]) refuse from their arguments alone, and what a refusal leaves behind.

Every refusal by return code and the full text of tredgpu_inflater_last_error; the calls the binding cannot make wrong go
straight through ctypes.  None of them launches a kernel or allocates: after each one the valid decode and the valid walk
on the same inflater give what they gave before, and the page-locked memory the inflater holds is what it was."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from tredparse_amd import _lib

pytestmark = pytest.mark.gpu

RESERVE = "bad arguments (reserve first)"
BLOCKS = "block offsets: payloads start on 4-byte boundaries, ascend, and inflate to at most 64 KiB each"
BEYOND = "offsets beyond the reserved buffers"
NO_HOST_RUN = "this inflater keeps no host copy of the output (tredgpu_inflater_host_out): walk and fetch"
NO_HOST_FETCH = "this inflater keeps no host copy of the output: tredgpu_inflater_fetch_dense"
WALK = "bad walk arguments"
ALT = "bad walk arguments (alternative loci)"
TASK = "walk task outside its chunks / blocks"
CHUNK = "walk chunk starts outside a block"
SELECT = "select and selected go together"
SELECT_ALT = "select task outside the alternative loci's tasks"


def _record(name, pos, flag, mate_pos, tlen):
    """One BAM alignment record of contig 0: 36 bases, 36M."""
    body = struct.pack("<iiBBHHHiiii", 0, pos, len(name) + 1, 60, 4681, 1, flag, 36, 0, mate_pos, tlen)
    body += name.encode() + b"\0" + struct.pack("<I", 36 << 4) + bytes([0x12, 0x48] * 9) + bytes([30] * 36)
    return struct.pack("<i", len(body)) + body


def _blocks(n_pairs=4, first=1100):
    """Three blocks of three records each: n_pairs pairs 200 bp apart, by position, and a record beyond the region that ends the walk."""
    recs = [(first + 50 * k, _record("read%03d" % k, first + 50 * k, 99, first + 200 + 50 * k, 236)) for k in range(n_pairs)]
    recs += [(first + 200 + 50 * k, _record("read%03d" % k, first + 200 + 50 * k, 147, first + 50 * k, -236)) for k in range(n_pairs)]
    recs = [r for _, r in sorted(recs)] + [_record("beyond0", 5000, 0, -1, 0)]
    return [b"".join(recs[k:k + 3]) for k in range(0, len(recs), 3)]


class Call:
    """The valid call: the blocks' payloads and sizes, and the walk's tables over them (one task with one chunk, one
    alternative task, one select task)."""

    def __init__(self, copies=1):
        self.data = _blocks() * copies
        self.payloads = []
        for d in self.data:
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            self.payloads.append(c.compress(d) + c.flush())
        self.n = n = len(self.data)
        self.coff = np.zeros(n + 1, np.int64)
        for k, p in enumerate(self.payloads):
            self.coff[k + 1] = (self.coff[k] + len(p) + 3) & ~3
        self.ooff = np.concatenate([[0], np.cumsum([len(d) for d in self.data])]).astype(np.int64)
        self.crc = np.array([zlib.crc32(d) for d in self.data], np.uint32)
        # the blocks as they lie in their file, one behind the other
        self.blk_clen = np.array([len(p) + 26 for p in self.payloads], np.int32)
        self.blk_coffset = np.concatenate([[0], np.cumsum(self.blk_clen)[:-1]]).astype(np.int64)
        end = int(self.blk_coffset[2] + self.blk_clen[2]) << 16        # (the first file's three blocks)
        self.tasks = np.zeros(1, _lib.WALK_TASK_DTYPE)
        self.tasks[0] = (0, 1000, 2000, 1400, 1500, 1000, 0, 1, 0, 3, 1300, 1700)
        self.chunks = np.zeros(1, _lib.WALK_CHUNK_DTYPE)
        self.chunks[0] = (0, 0, end)
        self.alt_tasks = self.tasks.copy()
        self.alt_tasks[0] = (0, 1000, 2000, 0, 0, 0, 0, 1, 0, 3, 1300, 1320)
        self.alt_chunks = self.chunks.copy()
        self.select = np.zeros(1, _lib.SELECT_TASK_DTYPE)
        self.select[0] = (1200, 1400, 0, 1)

    def lay_out(self, inf):
        """reserve, and the payloads and offsets in the staging; returns the views (comp, out, coff, ooff)."""
        v = inf.reserve(int(self.coff[-1]), int(self.ooff[-1]), self.n)
        v[0][:] = 0
        for k, p in enumerate(self.payloads):
            v[0][self.coff[k]:self.coff[k] + len(p)] = np.frombuffer(p, np.uint8)
        v[2][:] = self.coff
        v[3][:] = self.ooff
        return v

    def decode(self, inf):
        """The valid tredgpu_inflate_blocks_crc: zlib's bytes in `out`, zlib's CRC-32 per block."""
        _, out, _, ooff = self.lay_out(inf)
        status, sums = inf.run(self.n, crc=True)
        assert status.tolist() == [0] * self.n
        assert [bytes(out[ooff[k]:ooff[k + 1]]) for k in range(self.n)] == self.data
        assert sums.tolist() == self.crc.tolist()

    def walk(self, inf):
        """The valid tredgpu_inflate_walk: every array it returns, as bytes."""
        self.lay_out(inf)
        got = inf.run_walk(self.n, self.blk_coffset, self.blk_clen, self.crc, self.tasks, self.chunks, alt_tasks=self.alt_tasks,
                           alt_chunks=self.alt_chunks, select=self.select)
        assert got[0].tolist() == [0] * self.n and got[1].tolist() == self.crc.tolist()
        return tuple(np.ascontiguousarray(a).tobytes() for a in got)


class Raw:
    """The entry points through ctypes, from the valid call's arguments with some of them changed."""

    def __init__(self, inf, call):
        self.lib, self.h, self.call, self.inf = inf._lib, inf._h, call, inf
        n = call.n
        self.status, self.sums = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        self.res, self.ares = np.zeros(1, _lib.WALK_RESULT_DTYPE), np.zeros(1, _lib.ALT_RESULT_DTYPE)
        self.selres, self.need = np.zeros(1, _lib.SELECT_RESULT_DTYPE), np.zeros(n, np.uint8)
        self.gp, self.tp = np.zeros(4096, np.int32), np.zeros(1024, np.int32)
        self.keep = []

    def text(self):
        return self.lib.tredgpu_inflater_last_error(self.h).decode()

    def run(self, n=None, status=True, staged=None):
        """tredgpu_inflate_blocks_crc over the staged call; staged(coff, ooff) changes the offsets in the staging."""
        _, _, coff, ooff = self.call.lay_out(self.inf)
        if staged:
            staged(coff, ooff)
        return self.lib.tredgpu_inflate_blocks_crc(self.h, self.call.n if n is None else n, self.status.ctypes.data if status else None,
                                                   self.sums.ctypes.data)

    def walk(self, null=(), walk=True, **change):
        """tredgpu_inflate_walk: the fields named in `null` NULL, arrays and counts of `change` instead of the call's."""
        c = self.call
        a = dict(blk_coffset=c.blk_coffset, blk_clen=c.blk_clen, blk_crc=c.crc, tasks=c.tasks, n_tasks=1, chunks=c.chunks, n_chunks=1,
                 results=self.res, global_pool=self.gp, cap_global=len(self.gp), target_pool=self.tp, cap_target=len(self.tp), n_global=0,
                 n_target=0, alt_tasks=c.alt_tasks, n_alt_tasks=1, alt_chunks=c.alt_chunks, n_alt_chunks=1, alt_results=self.ares,
                 need=self.need, select=c.select, selected=self.selres)
        a.update(change)
        self.keep = list(a.values())
        fields = {k: (None if k in null else v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in a.items()}
        args = _lib.WalkArgs(**fields)
        self.call.lay_out(self.inf)
        return self.lib.tredgpu_inflate_walk(self.h, c.n, self.status.ctypes.data, self.sums.ctypes.data, C.byref(args) if walk else None)

    def fetch(self, need=True):
        return self.lib.tredgpu_inflater_fetch(self.h, self.call.n, self.need.ctypes.data if need else None)

    def fetch_dense(self, need=True, host=True, off=True):
        host_p, dense_off = C.c_void_p(), np.zeros(self.call.n + 1, np.int64)
        return self.lib.tredgpu_inflater_fetch_dense(self.h, self.call.n, self.need.ctypes.data if need else None,
                                                     C.byref(host_p) if host else None, dense_off.ctypes.data if off else None)


def _changed(arr, **fields):
    a = arr.copy()
    for k, v in fields.items():
        a[0][k] = v
    return a


def _set(which, k, value):
    def staged(coff, ooff):
        (coff if which == "coff" else ooff)[k] = value
    return staged


def _table(c):
    """(the refused call, its text): each returns -2."""
    return [
        # tredgpu_inflate_blocks_crc
        (lambda r: r.run(n=1000), RESERVE),                                       # beyond the reservation
        (lambda r: r.run(n=-1), RESERVE),
        (lambda r: r.run(status=False), RESERVE),
        (lambda r: r.run(staged=_set("coff", 1, int(c.coff[1]) + 2)), BLOCKS),    # off its 4-byte boundary
        (lambda r: r.run(staged=_set("coff", 1, int(c.coff[2]) + 4)), BLOCKS),    # descending
        (lambda r: r.run(staged=_set("ooff", 2, int(c.ooff[1]) - 1)), BLOCKS),    # descending
        (lambda r: r.run(staged=_set("ooff", 3, int(c.ooff[2]) + 65537)), BLOCKS),
        (lambda r: r.run(staged=_set("coff", 3, 1 << 30)), BEYOND),
        (lambda r: r.run(staged=_set("ooff", 3, int(c.ooff[2]) + 65536)), BEYOND),
        # tredgpu_inflate_walk
        (lambda r: r.walk(walk=False), "walk is NULL"),
        (lambda r: r.walk(null=("blk_crc",)), WALK),
        (lambda r: r.walk(null=("blk_coffset",)), WALK),
        (lambda r: r.walk(null=("results",)), WALK),
        (lambda r: r.walk(null=("global_pool",)), WALK),
        (lambda r: r.walk(n_tasks=-1), WALK),
        (lambda r: r.walk(n_chunks=-1), WALK),
        (lambda r: r.walk(cap_target=-1), WALK),
        (lambda r: r.walk(tasks=_changed(c.tasks, chunk_first=1)), TASK),         # outside its chunks
        (lambda r: r.walk(tasks=_changed(c.tasks, block_end=4)), TASK),           # outside its blocks
        (lambda r: r.walk(tasks=_changed(c.tasks, block_first=3, block_end=2)), TASK),
        (lambda r: r.walk(chunks=_changed(c.chunks, begin_upos=65537)), CHUNK),
        (lambda r: r.walk(chunks=_changed(c.chunks, begin_upos=-1)), CHUNK),
        (lambda r: r.walk(null=("need",)), ALT),
        (lambda r: r.walk(null=("alt_results",)), ALT),
        (lambda r: r.walk(n_alt_tasks=-1), ALT),
        (lambda r: r.walk(alt_tasks=_changed(c.alt_tasks, block_end=4)), TASK),
        (lambda r: r.walk(alt_chunks=_changed(c.alt_chunks, begin_upos=65537)), CHUNK),
        (lambda r: r.walk(null=("selected",)), SELECT),
        (lambda r: r.walk(null=("select",)), SELECT),
        (lambda r: r.walk(select=_changed(c.select, alt_first=1)), SELECT_ALT),
        (lambda r: r.walk(select=_changed(c.select, n_alt=2)), SELECT_ALT),
        # ... two faults in one call: the blocks are looked at before the walk's arguments, the tasks before the alternative loci
        (lambda r: r.walk(null=("blk_crc",), tasks=_changed(c.tasks, block_end=4)), WALK),
        (lambda r: r.walk(null=("need",), chunks=_changed(c.chunks, begin_upos=65537)), CHUNK),
        # tredgpu_inflater_fetch / _fetch_dense
        (lambda r: r.fetch(need=False), "bad arguments"),
        (lambda r: r.fetch_dense(need=False), "bad arguments"),
        (lambda r: r.fetch_dense(host=False), "bad arguments"),
        (lambda r: r.fetch_dense(off=False), "bad arguments"),
    ]


def test_every_refusal_by_code_and_text_then_the_valid_calls():
    c = Call()
    assert c.n == 3 and all(200 < len(d) < 400 for d in c.data)
    inf = _lib.Inflater(0)
    try:
        c.decode(inf)
        first = c.walk(inf)
        held = inf.pinned_bytes()
        assert held > 0
        r = Raw(inf, c)
        rows = _table(c)
        for k, (refused, text) in enumerate(rows):
            assert (refused(r), r.text()) == (-2, text), k
            c.decode(inf)
            assert c.walk(inf) == first, k
        # an inflater without a host copy of the output: no plain decode, no fetch to its place
        assert inf._lib.tredgpu_inflater_host_out(inf._h, 0) == 0
        c.lay_out(inf)
        for k, (refused, text) in enumerate([(lambda r: r.run(), NO_HOST_RUN), (lambda r: r.fetch(), NO_HOST_FETCH)]):
            assert (refused(r), r.text()) == (-2, text), k
            assert c.walk(inf) == first, k
        assert inf._lib.tredgpu_inflater_host_out(inf._h, 1) == 0
        c.decode(inf)
        assert c.walk(inf) == first
        # a refusal allocates nothing; calls of the same size neither
        assert inf.pinned_bytes() == held
        for _ in range(3):
            c.decode(inf)
            assert c.walk(inf) == first
            assert inf.pinned_bytes() == held
        twice = Call(copies=2)
        assert twice.n == 6
        twice.decode(inf)
        assert twice.walk(inf)[2:6] == first[2:6]         # (the same walks over the first three of six blocks)
        assert inf.pinned_bytes() >= held
    finally:
        inf.close()
        inf.close()
    assert inf.pinned_bytes() == 0
