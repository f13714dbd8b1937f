"""GPU parity of the long-read path (Context.set_long_reads -> tredlong_sw_classify): reads beyond 480 bp and ladders beyond 511 columns,
per template against the restated ssw_align and the reference's compiled ssw.c, per read against the restated
_parseReadSW.  The path is opt-in (Context.set_long_reads, include/tredlong.h): with the switch off every call
keeps today's refusals."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tredparse_amd import _lib, synth

pytestmark = pytest.mark.gpu

NAMES = {3: "HD", 4: "DM2", 5: "SCA10", 6: "SCA36", 12: "ULD"}


@pytest.fixture(scope="module")
def lctx(ctx):
    """A context of its own, so that the switch never reaches the other test modules' session context (`ctx` first:
    torch's HIP runtime is loaded before the library's, conftest.py)."""
    c = _lib.Context(0)
    c.set_long_reads(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def by_period():
    return {len(l["repeat"]): l for l in synth.load_loci() if l["name"] in NAMES.values()}


def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _mutate(rng, s, rate=0.01):
    s = list(s)
    for k in np.nonzero(rng.random(len(s)) < rate)[0]:
        s[k] = "ACGTN"[rng.integers(0, 5)]
    return "".join(s)


def _reads(rng, locus, units, L):
    """Spanning, prefix, suffix and inside-the-repeat reads on both strands, a read with N, an all-N read."""
    pre, rep, suf = locus["prefix"], locus["repeat"], locus["suffix"]
    left, right = _rand(rng, L + 40), _rand(rng, L + 40)
    g = left + pre + rep * units + suf + right
    a = len(left)                              # first base of the prefix
    b = a + len(pre) + len(rep) * units        # first base of the suffix
    starts = [max(0, (a + b + len(suf)) // 2 - L // 2),   # spanning, if the allele fits
              a - L + len(pre) + 3 * len(rep),            # ends a few units into the repeat: prefix read
              b - 3 * len(rep),                           # starts a few units before the suffix: suffix read
              a + len(pre) + len(rep)]                    # starts inside the repeat
    out = []
    for k, s in enumerate(starts):
        s = min(max(s, 0), len(g) - L)
        r = _mutate(rng, g[s:s + L])
        out.append(po.rc(r) if k % 2 else r)
    out.append(po.rc(out[0]))
    n = list(out[1])
    for k in rng.integers(0, L, 12):
        n[k] = "N"
    out.append("".join(n))
    out.append("N" * L)
    return out


def _classify(ctx, ladders, reads, uro, ul, nt=0, clip=False, max_read_len=0):
    ctx.set_ladders(ladders)
    packed, woff, rlen = _lib.pack_reads(reads)
    n = len(reads)
    tag = np.zeros(n, np.uint8); h = np.zeros(n, np.int16); sc = np.zeros(n, np.int16)
    d = np.zeros((n, max(nt, 1), 6), np.int16) if nt else None
    ctx.sw_classify(_lib.MEM_HOST, packed, woff, rlen, n, np.asarray(uro, np.int32), np.asarray(ul, np.int32), len(ul),
                    _lib.default_sw_params(clip=clip, max_read_len=max_read_len), tag, h, sc, d, nt)
    return tag, h, sc, d


def _check_dump(reads, templates, dump, picks):
    """dump[r, k] against the restated ssw_align (and the compiled reference's) on the templates `picks`."""
    pr = np.repeat(np.arange(len(reads)), len(picks))
    pt = np.tile(np.asarray(picks), len(reads))
    got = dump[:, picks, :5].reshape(-1, 5).astype(np.int32)
    want = po.sw_pairs(reads, templates, pr, pt, threads=16)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "read {} template {}: gpu {} oracle {}".format(pr[bad[0]], pt[bad[0]], got[bad[0]], want[bad[0]])
    if po.have_ref():
        ref = po.ref_sw_pairs(reads, templates, pr, pt, threads=16)
        ok = ref[:, 0] != po.REF_CRASHED
        assert np.array_equal(got[ok], ref[ok])


@pytest.mark.parametrize("L,period,units,mu", [(481, 3, 60, None), (600, 4, 200, None), (600, 12, 30, None),
                                               (1000, 5, 120, None), (1000, 6, 300, None), (700, 3, 150, 1353),
                                               (2048, 3, 500, None)])
def test_dump_matches_ssw(lctx, by_period, L, period, units, mu):
    rng = np.random.default_rng(L * 31 + period)
    locus = by_period[period]
    mu = mu or -(-L // period)
    lad = (locus["prefix"], locus["repeat"], locus["suffix"], mu)
    assert len(lad[0]) + len(lad[2]) + period * mu <= _lib.MAX_LONG_TEMPLATE_LEN
    reads = _reads(rng, locus, min(units, mu), L)
    nt = 2 * mu
    tag, h, sc, dump = _classify(lctx, [lad], reads, [0, len(reads)], [0], nt=nt)
    templates = [t for _, t in po.build_ladder(*lad)]
    # every template of short ladders; ends, the region of the true allele and a random sample of long ones
    if nt <= 200:
        picks = list(range(nt))
    else:
        k0 = 2 * (min(units, mu) - 1)
        picks = sorted(set(range(0, 8)) | set(range(nt - 8, nt)) | set(range(max(0, k0 - 10), min(nt, k0 + 10))) |
                       set(rng.choice(nt, 40, replace=False).tolist()))
    _check_dump(reads, templates, dump, picks)
    if nt * L * len(templates[-1]) <= 4e9:   # the per-read arg-max over every template (oracle cost bound)
        cls = po.classify(reads, np.zeros(len(reads), np.int32), po.LocusSet([lad]), threads=16)
        assert np.array_equal(tag, cls[:, 0].astype(np.uint8))
        assert np.array_equal(h, cls[:, 1].astype(np.int16))
        assert np.array_equal(sc, cls[:, 2].astype(np.int16))
    assert (dump[:, :, 0] > 0).any()


@pytest.mark.parametrize("readlen", [600, 1000])
@pytest.mark.parametrize("clip", [False, True])
def test_tags_match_parse_read_sw(lctx, readlen, clip):
    loci = [l for l in synth.load_loci() if l["name"] in (("HD", "ULD") if readlen == 600 else ("SCA10",))]
    p = synth.SynthParams(coverage=4, readlen=readlen, sub=0.01, indel=0.002, nrate=0.005, min_units=5,
                          max_units=readlen // 4)
    b = synth.build_batch(readlen + int(clip), loci, 2, p)
    reads = [synth.decode(r) for r in b.codes]
    tag, h, sc, _ = _classify(lctx, b.ladders, reads, b.unit_read_off, b.unit_ladder, clip=clip)
    rl = np.repeat(b.unit_ladder, np.diff(b.unit_read_off))
    ls = po.LocusSet(b.ladders)
    cls = po.classify(reads, rl, ls, clip=clip, threads=16)
    assert np.array_equal(tag, cls[:, 0].astype(np.uint8))
    assert np.array_equal(h, cls[:, 1].astype(np.int16))
    assert np.array_equal(sc, cls[:, 2].astype(np.int16))
    assert (tag != 0).sum() > 0
    if po.have_ref():
        ref = po.ref_classify(reads, rl, ls, clip=clip, threads=16)
        ok = ref[:, 0] >= 0
        assert np.array_equal(cls[ok], ref[ok])


def test_mixed_batch_leaves_short_reads_alone(lctx, by_period):
    """150 bp and 700 bp reads in one call: the short ones' outputs are those of the same call without the switch."""
    rng = np.random.default_rng(150700)
    hd = by_period[3]
    lad = (hd["prefix"], hd["repeat"], hd["suffix"], 50)
    short = _reads(rng, hd, 30, 150)
    long_ = _reads(rng, hd, 120, 700)
    reads = [r for pair in zip(short, long_) for r in pair]
    is_short = np.array([len(r) == 150 for r in reads])
    t_on, h_on, s_on, d_on = _classify(lctx, [lad], reads, [0, len(reads)], [0], nt=100)
    off = _lib.Context(0)
    try:
        sub = [r for r in reads if len(r) == 150]
        t_off, h_off, s_off, d_off = _classify(off, [lad], sub, [0, len(sub)], [0], nt=100)
    finally:
        off.close()
    assert np.array_equal(t_on[is_short], t_off) and np.array_equal(h_on[is_short], h_off)
    assert np.array_equal(s_on[is_short], s_off) and np.array_equal(d_on[is_short], d_off)
    # the long reads against the oracle (the ladder is the short one: ceil(700/3) units would be long)
    cls = po.classify([r for r in reads if len(r) == 700], np.zeros(len(long_), np.int32), po.LocusSet([lad]), threads=16)
    assert np.array_equal(t_on[~is_short], cls[:, 0].astype(np.uint8))
    assert np.array_equal(h_on[~is_short], cls[:, 1].astype(np.int16))


def test_bounds(lctx, by_period):
    hd = by_period[3]
    rng = np.random.default_rng(2049)
    ok_lad = (hd["prefix"], "CAG", hd["suffix"], 1353)       # 4 095 columns
    too_long = (hd["prefix"], "CAG", hd["suffix"], 1354)     # 4 098 columns
    read = _rand(rng, 2049)
    with pytest.raises(_lib.TredGpuError, match="TREDGPU_MAX_LONG_READ_LEN"):
        _classify(lctx, [ok_lad], [read], [0, 1], [0])
    with pytest.raises(_lib.TredGpuError, match="TREDGPU_MAX_LONG_TEMPLATE_LEN=4095"):
        lctx.set_ladders([too_long])
    lctx.set_ladders([ok_lad])
    with pytest.raises(_lib.TredGpuError, match="host-memory calls"):
        lctx.sw_classify(_lib.MEM_DEVICE, 0, 0, 0, 1, 0, 0, 1, _lib.default_sw_params(), 0, 0, 0)
    with pytest.raises(_lib.TredGpuError, match="register shorter ladders"):
        lctx.set_long_reads(False)
    # hist_stride of the routed calls (a 600 bp read takes the long path): genotype_batch checks it against every registered
    # ladder (the library's max_ladder_units), genotype_batch_joint against the batch's own ladders (the fused call's per-unit check)
    lctx.set_ladders([(hd["prefix"], "CAG", hd["suffix"], 50), (hd["prefix"], "CAG", hd["suffix"], 300)])
    packed, woff, rlen = _lib.pack_reads([read[:600]])
    uro, ul, units, lens = np.array([0, 1], np.int32), np.zeros(1, np.int32), np.zeros(1, _lib.UNIT_DTYPE), np.zeros(1, np.int32)
    tag, h, sc, calls = np.zeros(1, np.uint8), np.zeros(1, np.int16), np.zeros(1, np.int16), np.zeros(1, _lib.CALL_DTYPE)
    hist = [np.zeros((1, 100), np.int32) for _ in range(3)]
    with pytest.raises(_lib.TredGpuError, match="^hist_stride 100 must exceed the max_units 300 of ladder 1$"):
        lctx.genotype_batch(_lib.MEM_HOST, packed, woff, rlen, 1, uro, ul, units, 1, _lib.default_sw_params(), None, lens, 0,
                            lens, 0, tag, h, sc, 100, *hist, calls)
    marg, joff, trip = np.zeros((1, 2, 302), np.float64), np.array([0, 8], np.int64), np.zeros((8, 3), np.float64)
    with pytest.raises(_lib.TredGpuError, match="^hist_stride 50 must exceed the max_units 50 of ladder 0$"):
        lctx.genotype_batch_joint(packed, woff, rlen, 1, uro, ul, units, 1, _lib.default_sw_params(), None, lens, 0, lens, 0,
                                  tag, h, sc, 50, hist[2], calls, marg, 302, joff, trip, np.zeros(1, np.int32), np.zeros(1))
    # switched off: today's refusals
    off = _lib.Context(0)
    try:
        with pytest.raises(_lib.TredGpuError, match="exceeds 511"):
            off.set_ladders([(hd["prefix"], "CAG", hd["suffix"], 200)])
        with pytest.raises(_lib.TredGpuError, match="TREDGPU_MAX_READ_LEN=480"):
            _classify(off, [(hd["prefix"], "CAG", hd["suffix"], 50)], [read[:490]], [0, 1], [0])
    finally:
        off.close()


@pytest.mark.parametrize("readlen,names", [(600, ("HD", "DM1", "ULD")), (1000, ("HD", "SCA10")), (2048, ("HD",))])
def test_genotype_batch_against_the_oracles(lctx, readlen, names):
    """The whole host-memory path with long reads (SW on the long kernel -> tally -> grid), and the grid at READLEN 600,
    1 000 (= SPAN) and 2 048 (hist_stride > 683 at period 3): calls against the likelihood oracle (lik_oracle.Caller with
    that READLEN) fed with the GPU's tags; at 600 bp the tags against the restated _parseReadSW as well."""
    from oracle import lik_oracle as lo
    loci = [l for l in synth.load_loci() if l["name"] in names]
    p = synth.SynthParams(coverage=6, readlen=readlen, flank=max(1200, readlen + 600), ins_mean=readlen + 300.0,
                          min_units=5, max_units=min(150, readlen // 3))
    b = synth.build_batch(600600 + readlen, loci, 2, p)
    lctx.set_ladders(b.ladders)
    step, w = lo.load_model()
    lctx.set_model(np.array([step[k] for k in range(1, 7)]), np.array(w))
    n, g, hs = b.n_reads, b.n_units, b.hist_stride
    assert hs > max(l[3] for l in b.ladders)
    tag = np.zeros(n, np.uint8); h = np.zeros(n, np.int16); sc = np.zeros(n, np.int16)
    full = np.zeros((g, hs), np.int32); pref = np.zeros((g, hs), np.int32); rept = np.zeros((g, hs), np.int32)
    calls = np.zeros(g, _lib.CALL_DTYPE)
    lctx.genotype_batch(_lib.MEM_HOST, b.packed, b.read_off, b.read_len, n, b.unit_read_off, b.unit_ladder, b.units, g,
                        _lib.default_sw_params(), None, b.global_lens, len(b.global_lens), b.target_lens,
                        len(b.target_lens), tag, h, sc, hs, full, pref, rept, calls)
    assert not (tag == _lib.TAG_INVALID).any()
    if readlen == 600:
        reads = [synth.decode(r) for r in b.codes]
        cls = po.classify(reads, np.repeat(b.unit_ladder, np.diff(b.unit_read_off)), po.LocusSet(b.ladders), threads=16)
        assert np.array_equal(tag, cls[:, 0].astype(np.uint8)) and np.array_equal(h, cls[:, 1].astype(np.int16))
    n_ok = 0
    for u in range(g):
        f, pp, rr = {}, {}, 0
        for t, hh in zip(tag[b.unit_read_off[u]:b.unit_read_off[u + 1]], h[b.unit_read_off[u]:b.unit_read_off[u + 1]]):
            if t == 1: f[int(hh)] = f.get(int(hh), 0) + 1
            elif t in (2, 3): pp[int(hh)] = pp.get(int(hh), 0) + 1
            elif t == 4: rr += 1
        up = b.units[u]
        res = lo.Caller(int(up["period"]), readlen, 2, 2 * float(up["half_depth"]), f, pp, rr,
                        b.global_lens[up["pe_off"]:up["pe_off"] + up["n_global"]],
                        b.target_lens[up["tl_off"]:up["tl_off"] + up["n_target"]], int(up["ref_len"]),
                        int(up["minpe"])).evaluate()
        assert calls[u]["status"] == res["status"], (u, calls[u], res)
        if res["status"] == 0:
            assert (calls[u]["h1"], calls[u]["h2"]) == tuple(res["alleles"]), (u, calls[u], res)
            assert abs(calls[u]["lik"] - res["lik"]) <= 1e-6
            n_ok += 1
    assert n_ok > 0
