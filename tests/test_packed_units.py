"""CPU: the two ways into a PackedUnits give the same batch -- from_scans over the golden BAMs' scans against from_units
over Units built from the scans' own texts, depths, ploidies, pair lengths and name ids -- array for array, and text(i)
read for read.  (tests/test_host_frontend.py pins text packing equal to scan packing.)"""
import os

import numpy as np
import pytest

from tredparse_amd import _lib
from tredparse_amd.bam_parser import scan_sample
from tredparse_amd.engine import PackedUnits, Unit
from tredparse_amd.meta import TREDsRepo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPTIONS = dict(maxinsert=120, fullsearch=True)


@pytest.fixture(scope="module")
def scans():
    repo = TREDsRepo(ref="hg38")
    out = [scan_sample(os.path.join(GOLD, "bam", n + ".bam"), repo, repo.names) for n in ("t001", "t002")]
    assert all(s.opened and not s.dropped and len(s.names) == len(repo.names) for s in out)
    return out


def _units(picks, clip, with_ids):
    units = []
    for s, ks in picks:
        for k in ks:
            a, e = s.reads_of(k)
            gl, tl = s.pair_lengths(k)
            units.append(Unit(s.loci[k], s.readlen, [s.sequence(i) for i in range(a, e)], s.depth[k], s.ploidy[k], gl, tl, clip=clip,
                              read_pair_ids=s.name_id[a:e] if with_ids else None, **OPTIONS))
    return units


def _same(picks, clip=False, repeatpairs=True):
    a = PackedUnits.from_scans(picks, clip=clip, repeatpairs=repeatpairs, **OPTIONS)
    b = PackedUnits.from_units(_units(picks, clip, with_ids=not repeatpairs))
    n = a.n_reads
    assert (a.n_units, n) == (b.n_units, b.n_reads) and a.n_units == sum(len(ks) for _, ks in picks)
    assert np.array_equal(a.packed[:a.read_off[-1]], b.packed[:b.read_off[-1]]) and a.packed.dtype == b.packed.dtype == np.uint32
    for name in ("read_off", "read_len", "unit_read_off", "global_lens", "target_lens"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    assert a.params.dtype == b.params.dtype == _lib.UNIT_DTYPE
    for field in _lib.UNIT_DTYPE.names:
        assert np.array_equal(a.params[field], b.params[field]), field
    assert a.ladder_keys == b.ladder_keys and a.max_units == b.max_units and a.clip is b.clip is clip
    if repeatpairs:
        assert a.pair_id is None and b.pair_id is None
    else:
        assert a.pair_id.dtype == b.pair_id.dtype == np.int32 and np.array_equal(a.pair_id, b.pair_id)
    texts = [s.sequence(i) for s, ks in picks for k in ks for i in range(*s.reads_of(k))]
    assert len(texts) == n and [a.text(i) for i in range(n)] == texts == [b.text(i) for i in range(n)]
    return a


def test_every_locus_of_both_samples(scans):
    for s in scans:
        b = _same([(s, list(range(len(s.names))))])
        assert b.n_reads > 50 and (np.diff(b.unit_read_off) == 0).any()              # most loci of these BAMs have no read
    both = _same([(s, list(range(len(s.names)))) for s in scans])
    assert both.n_units == 2 * len(scans[0].names)


def test_pair_ids_and_clip(scans):
    picks = [(s, list(range(len(s.names)))) for s in scans]
    b = _same(picks, repeatpairs=False)
    assert len(b.pair_id) == b.n_reads > 0
    _same(picks, clip=True)


def test_picks_out_of_file_order_with_a_gap_and_an_empty_unit(scans):
    t001, t002 = scans
    assert t002.unit["n_reads"][0] > 0 and t002.unit["n_reads"][2] == 0 and t001.unit["n_reads"][7] > 0
    b = _same([(t002, [2, 0])])
    assert b.unit_read_off.tolist() == [0, 0, b.n_reads] and b.n_reads > 0
    _same([(t002, [2, 0])], repeatpairs=False)
    _same([(t001, [9, 7, 2]), (t002, []), (t002, [2, 0]), (t001, [7])], repeatpairs=False)     # reads of several scans, one twice
    empty = _same([(t002, [2])])
    assert empty.n_reads == 0 and empty.n_units == 1
    assert _same([]).n_units == 0


def test_a_list_that_mixes_clip_settings_is_refused(scans):
    units = _units([(scans[0], [7])], False, False) + _units([(scans[1], [0])], True, False)
    with pytest.raises(ValueError, match="all units of one batch must share the clip setting"):
        PackedUnits.from_units(units)
