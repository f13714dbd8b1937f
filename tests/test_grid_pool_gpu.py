"""GPU: a scratch pool smaller than one unit's largest slot (TREDGPU_GRID_POOL_MB=1).  The pool is then one slot room and is
used as ONE sub-pool -- every unit bumps the same counter, the sub-pool index of every unit is 0 -- which the 4 MiB pool of
test_fullsize_gpu.py does not reach.  The three entry points that share the grid passes (tredgpu_likelihood_grid,
tredgpu_likelihood_grid_joint, tredgpu_genotype_batch_joint) must give the calls of the default pool, record for record.
The batch: HD / DM1 / SCA1 x 4 samples of 38 to 60 units, seed 61 -- the CPU oracle (oracle/lik_oracle.py) evaluates every one
of its units (status 0), nine of them over 32 000 (h1, h2) pairs (axes of 255 or 256 entries at maxinsert 300).  The rectangle
of such a unit alone is 65 000 doubles, the pool one slot room of 436 784 (rows and columns capped at 353, 36 spanning pairs
at most): nine do not fit at once, so units are deferred and the one sub-pool is reused in a further pass."""
import numpy as np
import pytest

from oracle import lik_oracle as lo
from tredparse_amd import _lib, engine, synth

pytestmark = pytest.mark.gpu
JOINT_ROOM = 512


def _three_entry_points(b):
    """calls of the batch through each entry point, on a context of its own (the pool size is read when it is created);
    and the launches of grid_prepare_kernel each call made"""
    c = _lib.Context(0)
    try:
        step, w = lo.load_model()
        c.set_model(np.array([step[p] for p in range(1, 7)]), np.array(w))
        c.set_ladders(b.ladders)
        n, g, hs = b.n_reads, b.n_units, b.hist_stride
        ms = engine._marg_stride(b.units, hs)
        sw = _lib.default_sw_params(max_read_len=150)
        ngl, ntl = len(b.global_lens), len(b.target_lens)
        tag, h, sc = np.zeros(n, np.uint8), np.zeros(n, np.int16), np.zeros(n, np.int16)
        full, pref, rept = (np.zeros((g, hs), np.int32) for _ in range(3))
        joff = np.arange(g + 1, dtype=np.int64) * JOINT_ROOM
        out, passes = {}, {}

        def fresh():
            return (np.zeros(g, _lib.CALL_DTYPE), np.zeros((g, 2, ms), np.float64), np.zeros((g * JOINT_ROOM, 3), np.float64),
                    np.zeros(g, np.int32), np.zeros(g, np.float64))
        # the histograms of the batch (SW + tally)
        c.sw_classify(_lib.MEM_HOST, b.packed, b.read_off, b.read_len, n, b.unit_read_off, b.unit_ladder, g, sw, tag, h, sc)
        c.tally(_lib.MEM_HOST, tag, h, n, b.unit_read_off, g, None, hs, full, pref, rept)
        for name in ("grid", "grid_joint", "batch_joint"):
            calls, marg, joint, jn, jt = fresh()
            c.reset_timing()
            if name == "grid":
                c.likelihood_grid(_lib.MEM_HOST, b.units, g, hs, full, pref, rept, b.global_lens, ngl, b.target_lens, ntl, calls)
            elif name == "grid_joint":
                c.likelihood_grid_joint(_lib.MEM_HOST, b.units, g, hs, full, pref, rept, b.global_lens, ngl, b.target_lens, ntl,
                                        calls, marg, ms, joff, joint, jn, jt)
            else:
                c.genotype_batch_joint(b.packed, b.read_off, b.read_len, n, b.unit_read_off, b.unit_ladder, b.units, g, sw, None,
                                       b.global_lens, ngl, b.target_lens, ntl, tag, h, sc, hs, np.zeros((g, hs), np.int32), calls,
                                       marg, ms, joff, joint, jn, jt)
            out[name] = calls
            passes[name] = c.get_timing(_lib.KERNEL_GRID_PREPARE)[0]
            assert c.get_timing(_lib.KERNEL_GRID_KDE)[0] == 1 and c.get_timing(_lib.KERNEL_GRID)[0] == 1
            assert c.get_timing(_lib.KERNEL_GRID_PAIRS)[0] == c.get_timing(_lib.KERNEL_GRID_REDUCE)[0] == passes[name]
        return out, passes
    finally:
        c.close()


def test_pool_smaller_than_one_slot_is_one_sub_pool(loci, monkeypatch):
    sel = [l for l in loci if l["name"] in ("HD", "DM1", "SCA1")]
    b = synth.build_batch(61, sel, 4, synth.SynthParams(coverage=30, min_units=38, max_units=60), maxinsert=300)
    assert b.n_units == 12 and b.hist_stride == 52 and b.units["n_target"].max() == 36
    monkeypatch.delenv("TREDGPU_GRID_POOL_MB", raising=False)
    want, passes = _three_entry_points(b)
    assert set(passes.values()) == {1}                                # the default pool holds the batch at once
    monkeypatch.setenv("TREDGPU_GRID_POOL_MB", "1")
    got, small_passes = _three_entry_points(b)
    print("passes at 1 MiB", small_passes)
    ref = want["grid"]
    assert (ref["status"] == 0).all()
    assert (ref["n_pairs"] > 20000).sum() == 9
    assert min(small_passes.values()) >= 2                            # nine rectangles of 255 * 255 doubles exceed 436 784
    for name in ("grid", "grid_joint", "batch_joint"):
        assert np.array_equal(want[name], ref), name
        assert np.array_equal(got[name], ref), name
