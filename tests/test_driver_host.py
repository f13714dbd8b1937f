"""CPU: the driver between the scans and the writers (tred.run_many: grouping by kernel options, the GPU calls and their
failure ladder, formatting, the Emitter) seen from outside only -- the result dicts, the files an Emitter writes, the number
and size of the engine's calls and the logged errors -- with tests/fake_engine.FakeEngine in the kernels' place.

FakeEngine draws a call's arrays from (seed + 1000 * calls made so far) and the batch's shape, so a unit's values can be
had again from a plain FakeEngine of the matching seed over a batch of the same shape: that is how "the same values as a
run restricted to those units" is checked below."""
import gzip
import logging
import os

from tests.fake_engine import FakeEngine
from tredparse_amd import _lib
from tredparse_amd import tred as t

from .test_walk_host import cohort                      # noqa: F401  (the fixture: golden and synthetic BAMs, one that is missing)
from .walk_model import ModelInflater

SEED = 7


def _task(cohort, key):
    return next(a for a in cohort if a[0] == key)


def _unit_marks(arg):
    """[(ladder key, half the depth)] of the task's units as a batch shows them: tells a (sample, locus) apart from every other."""
    from tredparse_amd.engine import PackedUnits
    s = t.collect_sample(arg)
    assert s.opened and not s.dropped
    b = PackedUnits.from_scans([(s, list(range(len(s.names))))])
    return [(key, float(d)) for key, d in zip(b.ladder_keys, b.params["half_depth"])]


class Recording(FakeEngine):
    """Notes every genotype_packed call that comes from the driver itself (not from inside genotype_selected)."""
    def __init__(self, **kw):
        FakeEngine.__init__(self, **kw)
        self.packed, self.selected, self.inside = [], [], False

    def genotype_packed(self, b, dense=False):
        if not self.inside:
            self.packed.append(b)
        return FakeEngine.genotype_packed(self, b, dense)

    def genotype_selected(self, scans, **kw):
        self.selected.append([s.path for s in scans])
        self.inside = True
        try:
            return FakeEngine.genotype_selected(self, scans, **kw)
        finally:
            self.inside = False


class RejectsOneUnit(Recording):
    """Every batch that holds the unit `mark` fails as a whole, as a kernel refusal does."""
    def __init__(self, mark, **kw):
        Recording.__init__(self, **kw)
        self.mark = mark

    def genotype_packed(self, b, dense=False):
        if self.mark in [(key, float(d)) for key, d in zip(b.ladder_keys, b.params["half_depth"])]:
            self.packed.append(b)
            raise _lib.TredGpuError("the kernels refuse this unit")
        return Recording.genotype_packed(self, b, dense)


def _files(d):
    out = {}
    for p in sorted(os.listdir(d)):
        with open(os.path.join(d, p), "rb") as fp:
            raw = fp.read()
        out[p] = gzip.decompress(raw) if p.endswith(".gz") else raw
    return out


def _write(tasks, engine, out, repo, names, emit, seen=None):
    """The tasks' files in directory `out`: through an Emitter, or through the sink that the Emitter replaces."""
    os.makedirs(out)
    cwd = os.getcwd()
    os.chdir(out)
    try:
        if emit:
            em = t.Emitter("hg38", repo, names, workers=2, on_sample=None if seen is None else seen.append)
            try:
                t.run_many(tasks, engine, batch=len(tasks), threads=2, lazy_details=True, emit=em)
            finally:
                em.close()
        else:
            t.run_many(tasks, engine, batch=len(tasks), threads=2, lazy_details=True,
                       sink=lambda r: (t.write_vcf_json(r, "hg38", repo, names, quiet=True), seen is not None and seen.append(r)))
    finally:
        os.chdir(cwd)
    return _files(out)


# ---- the retry ladder: batch -> sample -> single unit ---------------------------------------------------------------------
def _ladder_case(cohort):
    """Three samples of one option group, and the mark of the second one's DM1."""
    tasks = [_task(cohort, "syn0000"), _task(cohort, "syn0001"), _task(cohort, "cut300")]
    assert [len(a[3]) for a in tasks] == [4, 4, 2]
    marks = [_unit_marks(a) for a in tasks]
    bad = marks[1][tasks[1][3].index("DM1")]
    assert sum(m == bad for ms in marks for m in ms) == 1
    return tasks, bad


def test_a_unit_the_kernels_reject_costs_only_itself(cohort, caplog):
    tasks, bad = _ladder_case(cohort)
    engine = RejectsOneUnit(bad, seed=SEED, odd_units=False)
    with caplog.at_level(logging.ERROR):
        got = t.run_many(tasks, engine, batch=3, threads=2, lazy_details=False)
    assert [g["samplekey"] for g in got] == [a[0] for a in tasks]                        # task order
    # the whole batch, then sample by sample, the bad one's units one by one as soon as it has failed
    assert [b.n_units for b in engine.packed] == [10, 4, 4, 1, 1, 1, 1, 2] and len(engine.packed) == 1 + 3 + len(tasks[1][3])
    lost = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Exception on")]
    assert len(lost) == 1 and "`{}` DM1 ".format(tasks[1][1]) in lost[0] and "the kernels refuse this unit" in lost[0]
    assert len([r for r in caplog.records if r.getMessage().startswith("GPU batch failed")]) == 1
    for g, a in zip(got, tasks):
        gone = ["DM1"] if a is tasks[1] else []
        assert [n for n in a[3] if n + ".1" not in g["tredCalls"]] == gone
        assert not any(k.startswith("DM1.") for k in g["tredCalls"]) or not gone
    # the engine's successful calls were: sample 0 (seed), the bad sample's other three loci on their own (seed + 1000 ...), then
    # sample 2 (seed + 4000): a plain engine of that seed over those units alone gives the same values
    assert got[0] == t.run_many([tasks[0]], FakeEngine(seed=SEED, odd_units=False), batch=1, lazy_details=False)[0]
    assert got[2] == t.run_many([tasks[2]], FakeEngine(seed=SEED + 4000, odd_units=False), batch=1, lazy_details=False)[0]
    kept = [n for n in tasks[1][3] if n != "DM1"]
    for j, name in enumerate(kept):
        alone = tasks[1][:3] + ([name],) + tasks[1][4:]
        want = t.run_many([alone], FakeEngine(seed=SEED + 1000 * (1 + j), odd_units=False), batch=1, lazy_details=False)[0]["tredCalls"]
        mine = {k: v for k, v in got[1]["tredCalls"].items() if k.startswith(name + ".")}
        assert mine and mine == {k: v for k, v in want.items() if k.startswith(name + ".")}, name
    whole = t.run_many([tasks[1]], FakeEngine(seed=SEED, odd_units=False), batch=1, lazy_details=False)[0]["tredCalls"]
    assert set(got[1]["tredCalls"]) == set(k for k in whole if not k.startswith("DM1."))
    for k in ("inferredGender", "depthY", "readLen"):
        assert got[1]["tredCalls"][k] == whole[k]


def test_a_batch_cut_to_single_units_is_written_by_the_python_path(cohort, tmp_path):
    """The same case through an Emitter: the sample whose batch was cut into pieces is not the native printers' (they print one
    piece); its files, like the others', are the sink path's."""
    tasks, bad = _ladder_case(cohort)
    repo, names = tasks[0][2], tasks[0][3]
    seen = []
    via_sink = _write(tasks, RejectsOneUnit(bad, seed=SEED, odd_units=False), str(tmp_path / "sink"), repo, names, emit=False)
    via_emit = _write(tasks, RejectsOneUnit(bad, seed=SEED, odd_units=False), str(tmp_path / "emit"), repo, names, emit=True, seen=seen)
    assert sorted(via_sink) == sorted(a[0] + ext for a in tasks for ext in (".json", ".tred.vcf.gz"))
    assert via_emit == via_sink
    text = via_emit["syn0001.json"].decode()
    assert '"DM1.1"' not in text and all('"{}.1"'.format(n) in text for n in names if n != "DM1")
    cut = next(s for s in seen if s["samplekey"] == "syn0001")
    assert cut["names"] == names and cut["printed"] == [n != "DM1" for n in names] and cut["first_allele"][names.index("DM1")] == -1


# ---- tasks of one call that differ in their kernel options ----------------------------------------------------------------
def test_each_option_group_is_one_call_and_each_sample_keeps_its_own_options(cohort):
    base = _task(cohort, "syn0000")
    other = _task(cohort, "syn0001")
    tasks = [base,
             ("short",) + other[1:4] + (60,) + other[5:],                     # --maxinsert 60
             ("nopairs",) + base[1:8] + (False,) + base[9:],                  # --norepeatpairs
             ("again",) + other[1:]]                                           # the first task's options once more
    class AllRepeat(Recording):                   # every read a repeat-only one: what --norepeatpairs then discards is not by chance
        def genotype_packed(self, b, dense=False):
            r = Recording.genotype_packed(self, b, dense)
            r.tag[:] = _lib.TAG_REPT
            return r
    engine = AllRepeat(seed=SEED, odd_units=False)
    got = t.run_many(tasks, engine, batch=4, threads=2, lazy_details=False)
    assert [g["samplekey"] for g in got] == ["syn0000", "short", "nopairs", "again"]
    # one call per group, in the order the groups first appear; --norepeatpairs alone sends the reads' pair ids
    assert [(sorted(set(b.params["maxinsert"].tolist())), b.pair_id is not None, b.n_units) for b in engine.packed] == \
        [([300], False, 8), ([60], False, 4), ([300], True, 4)]
    # every sample as a call of its own group alone gives it (the k-th call of an engine draws from seed + 1000 k)
    alone = [t.run_many([tasks[0], tasks[3]], AllRepeat(seed=SEED, odd_units=False), batch=2, lazy_details=False),
             t.run_many([tasks[1]], AllRepeat(seed=SEED + 1000, odd_units=False), batch=1, lazy_details=False),
             t.run_many([tasks[2]], AllRepeat(seed=SEED + 2000, odd_units=False), batch=1, lazy_details=False)]
    assert got == [alone[0][0], alone[1][0], alone[2][0], alone[0][1]]
    # and --norepeatpairs reaches the formatting: the same sample, the same arrays, pairs of repeat-only reads counted
    kept = t.run_many([("nopairs",) + base[1:]], AllRepeat(seed=SEED + 2000, odd_units=False), batch=1, lazy_details=False)[0]
    assert set(kept["tredCalls"]) == set(got[2]["tredCalls"])
    assert sum(kept["tredCalls"][n + ".RDP"] for n in base[3]) > sum(got[2]["tredCalls"][n + ".RDP"] for n in base[3])


# ---- a BAM that does not open ---------------------------------------------------------------------------------------------
def test_a_bam_that_does_not_open_gives_a_skeleton_and_no_unit(cohort, tmp_path, capsys):
    tasks = [_task(cohort, "noalts"), _task(cohort, "missing"), _task(cohort, "t002")]
    repo, names = tasks[2][2], tasks[2][3]
    units = len(tasks[0][3]) + len(tasks[2][3])
    assert not t.collect_sample(tasks[0]).dropped and not t.collect_sample(tasks[2]).dropped
    engine, results = Recording(seed=SEED, odd_units=False), []
    via_sink = _write(tasks, engine, str(tmp_path / "sink"), repo, names, emit=False, seen=results)
    assert [r["samplekey"] for r in results] == ["noalts", "missing", "t002"]
    assert results[1] == {"samplekey": "missing", "bam": tasks[1][1], "tredCalls": results[1]["tredCalls"]}
    assert sorted(results[1]["tredCalls"]) == ["depthY", "inferredGender"]
    assert "readLen" in results[0]["tredCalls"] and "HD.1" in results[0]["tredCalls"]
    assert [b.n_units for b in engine.packed] == [units]                     # (noalts and t002 share their kernel options)
    engine, seen = Recording(seed=SEED, odd_units=False), []
    via_emit = _write(tasks, engine, str(tmp_path / "emit"), repo, names, emit=True, seen=seen)
    assert [b.n_units for b in engine.packed] == [units]
    # a skeleton has no readLen for the VCF's head: neither path writes a file for it
    assert sorted(via_sink) == sorted(k + ext for k in ("noalts", "t002") for ext in (".json", ".tred.vcf.gz"))
    assert via_emit == via_sink
    gone = next(s for s in seen if s["samplekey"] == "missing")
    assert gone["names"] == ["HD"] and gone["printed"] == [False] and gone["first_allele"] == [-1]
    assert sorted(s["samplekey"] for s in seen) == ["missing", "noalts", "t002"]
    capsys.readouterr()


# ---- a record without a sequence among the reads the device selected ---------------------------------------------------------
def test_a_zero_length_read_sends_that_sample_alone_back_to_the_host(cohort, monkeypatch):
    monkeypatch.setattr("tredparse_amd._lib.Inflater", ModelInflater)
    t.release_inflaters()
    tasks = [_task(cohort, "syn0000"), _task(cohort, "syn0001"), _task(cohort, "cut300")]
    odd = tasks[1][1]

    class OneEmptyRead(Recording):
        def genotype_selected(self, scans, **kw):
            br = Recording.genotype_selected(self, scans, **kw)
            for s in scans:
                if s.path == odd:
                    s.read_len[0] = 0
            return br
    kw = dict(batch=3, threads=2, lazy_details=False)
    dev = dict(kw, inflate_device=0, gpu_walk=True, gpu_select=True)
    try:
        engine = OneEmptyRead(seed=SEED, odd_units=False)
        got = t.run_many(tasks, engine, **dev)
        plain = Recording(seed=SEED, odd_units=False)
        want = t.run_many(tasks, plain, **dev)
        host = t.run_many([tasks[1]], FakeEngine(seed=SEED + 1000, odd_units=False), batch=1, lazy_details=False)[0]
        t.release_inflaters()                                  # every lease was given back: the pool lets go of the inflaters
        again = t.run_many(tasks, Recording(seed=SEED, odd_units=False), **dev)     # ... and a second cohort goes through
    finally:
        t.release_inflaters()
    assert plain.selected == [[a[1] for a in tasks]] and plain.packed == []
    # one call over the device's reads for the chunk, then the odd sample alone, packed from the host's scan
    assert engine.selected == [[a[1] for a in tasks]]
    assert [b.n_units for b in engine.packed] == [len(tasks[1][3])]
    assert [g["samplekey"] for g in got] == [a[0] for a in tasks]
    assert got[0] == want[0] and got[2] == want[2]                # the others: as if nothing had happened
    assert got[1] == host                                         # the second call of the engine, over the host's scan of it
    assert again == want
