"""bench.py --dump-outputs DIR: what the headline's last timed step computed, as DIR/<name>.npy (float32 / float64, at
most 64 MB: a fixed, seeded sample of units beyond that).  CPU: the sample, the cap and the launcher's wiring; GPU: two
runs with the same arguments dump the same arrays, whatever --steps is."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fake_outputs(g=3000, hs=52, seed=5):
    from tredparse_amd import _lib
    rng = np.random.default_rng(seed)
    uro = np.zeros(g + 1, np.int32)
    uro[1:] = np.cumsum(rng.integers(0, 200, g))
    n = int(uro[-1])
    calls = np.zeros(g, _lib.CALL_DTYPE)
    for f in ("status", "n_pairs", "h1", "h2", "run_pe"):
        calls[f] = rng.integers(0, 1000, g)
    calls["ci"] = rng.integers(0, 1000, (g, 4))
    calls["lik"], calls["pp"] = rng.normal(size=g), rng.random(g)
    tag = rng.integers(0, 6, n).astype(np.uint8)
    h = rng.integers(-1, 300, n).astype(np.int16)
    sc = rng.integers(0, 300, n).astype(np.int16)
    full, pref, rept = (rng.integers(0, 50, (g, hs)).astype(np.int32) for _ in range(3))
    return uro, tag, h, sc, full, pref, rept, calls


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_keeps_every_call_and_a_fixed_sample_under_the_cap(tmp_path):
    import bench
    uro, tag, h, sc, full, pref, rept, calls = _fake_outputs()
    everything = bench.dump_outputs(str(tmp_path / "all"), uro, tag, h, sc, full, pref, rept, calls)
    a = _load(tmp_path / "all")
    assert set(a) == set(everything) and np.array_equal(a["unit_index"], np.arange(len(calls)))
    assert np.array_equal(a["tag"], tag) and np.array_equal(a["h"], h) and np.array_equal(a["score"], sc)
    assert np.array_equal(a["full"], full) and np.array_equal(a["pref"], pref) and np.array_equal(a["rept"], rept)
    limit = 1 << 20
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), uro, tag, h, sc, full, pref, rept, calls, limit=limit)
    s1, s2 = _load(tmp_path / "s1"), _load(tmp_path / "s2")
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= limit
    assert all(np.array_equal(s1[k], s2[k]) for k in s1) and set(s1) == set(s2)          # the same sample every time
    assert all(v.dtype in (np.float32, np.float64) for v in s1.values())
    units = s1["unit_index"].astype(np.int64)
    assert 0 < len(units) < len(calls) and np.all(np.diff(units) > 0)
    for f in calls.dtype.names:
        if f != "pad":
            assert np.array_equal(s1["calls_" + f], calls[f])                                 # every unit's call
    reads = np.concatenate([np.arange(uro[u], uro[u + 1]) for u in units])
    assert np.array_equal(s1["tag"], tag[reads]) and np.array_equal(s1["h"], h[reads]) and np.array_equal(s1["score"], sc[reads])
    assert np.array_equal(s1["full"], full[units]) and np.array_equal(s1["rept"], rept[units])


def test_only_the_headline_ranks_dump(monkeypatch, tmp_path):
    """The sweep's other rank counts and the extra legs run without the option: DIR holds the --gpus run's step."""
    import bench
    seen = []

    def fake_run_ranks(args, n, n_devices, dump=None):
        seen.append((n, dump))
        return {"value": 1.0, "unit": "genotypes/s", "ms_per_step": 1.0, "n_gpus": n}, []

    monkeypatch.setattr(bench, "run_ranks", fake_run_ranks)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    args = argparse.Namespace(stub=True, e2e_only=False, gpus=2, no_sweep=False, e2e_samples=0, e2e_wgs_samples=0, legs="",
                              no_cpu_baseline=True, dump_outputs=str(tmp_path / "d"), full=True)
    bench.launcher_main(args)
    assert seen == [(1, None), (2, str(tmp_path / "d"))]


def test_a_plain_run_is_the_headline_alone(monkeypatch, tmp_path):
    """Without --full: the --gpus ranks once (they dump), and none of the sweep, the from-BAM legs, the extra legs or the
    CPU baseline, whatever their own options say."""
    import bench
    from tredparse_amd import shard
    seen = []

    def fake_run_ranks(args, n, n_devices, dump=None):
        seen.append((n, dump))
        return {"value": 1.0, "unit": "genotypes/s", "ms_per_step": 1.0, "n_gpus": n}, []

    def never(*a, **k):
        raise AssertionError("a plain run ran more than the headline")

    monkeypatch.setattr(bench, "run_ranks", fake_run_ranks)
    for name in ("run_e2e", "run_e2e_wgs", "cpu_baselines", "make_batch"):
        monkeypatch.setattr(bench, name, never)
    monkeypatch.setattr(shard, "visible_gpus", lambda: 1)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    args = argparse.Namespace(stub=False, e2e_only=False, gpus=1, no_sweep=False, e2e_samples=4096, e2e_wgs_samples=64,
                              legs="streamed:4,config5:150:200", no_cpu_baseline=False, dump_outputs=str(tmp_path / "d"),
                              full=False)
    bench.launcher_main(args)
    assert seen == [(1, str(tmp_path / "d"))]


def _bench(out, steps):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-sweep", "--steps", str(steps),
                        "--warmup", "1", "--samples", "40", "--e2e-samples", "0", "--legs", "", "--no-cpu-baseline",
                        "--dump-outputs", out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_two_runs_dump_the_same_outputs(tmp_path):
    a_line, b_line = _bench(str(tmp_path / "a"), 3), _bench(str(tmp_path / "b"), 2)
    assert a_line["steps"] == 3 and b_line["steps"] == 2 and a_line["ms_per_step"] > 0 and b_line["ms_per_step"] > 0
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(b) and {"tag", "h", "score", "full", "calls_h1", "calls_lik"} <= set(a)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert len(a["unit_index"]) == len(a["calls_h1"]) == 40 * 30                      # a small batch: every unit
    assert (a["calls_status"] == 0).mean() > 0.9 and (a["tag"] > 0).any()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
