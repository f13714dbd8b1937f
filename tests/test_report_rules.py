"""CPU: what the per-read reports (--alignments, --consensus, --consensus-partial, --spectrum) decide without a kernel --
which group a tagged read is counted in (engine.place_consensus against tests/pileup_anchored_model.place,
engine.place_spectrum against the class naming of tests/test_spectrum_engine_gpu.model_classes), the item list
_Winners.take cuts out of the winners, and the members of a run() argument tuple that carry the reports' flags."""
import itertools
import types

import numpy as np

from tredparse_amd import _lib
from tredparse_amd.engine import _Winners, place_consensus, place_spectrum
from tredparse_amd.runtime import REPORTS, _options, option_tail

from . import pileup_anchored_model as am
from .test_spectrum_engine_gpu import model_classes

TAGS = (_lib.TAG_NONE, _lib.TAG_FULL, _lib.TAG_PREF, _lib.TAG_POST, _lib.TAG_REPT, _lib.TAG_HANG)
NAME_OF = {**_lib.TAG_NAMES, _lib.TAG_NONE: "NONE"}
# every (tag, h in 1..8) once per unit of a two-unit batch
READS = [(t, h) for t in TAGS for h in range(1, 9)]
TAG = np.array([t for t, _ in READS] * 2, np.uint8)
H = np.array([h for _, h in READS] * 2, np.int16)
UNIT_OF = np.repeat(np.arange(2, dtype=np.int64), len(READS))
# every list of up to three alleles asked for out of -1 .. 6, duplicates included; case i: list i on unit 0 beside list
# -1 - i on unit 1, so that every list is seen on both
LISTS = [list(x) for n in range(4) for x in itertools.product(range(-1, 7), repeat=n)]
CASES = [[LISTS[i], LISTS[-1 - i]] for i in range(len(LISTS))]
KINDS = {"whole": "full", "partial": "partial", "ambiguous": "ambiguous", "beyond": "beyond"}


def _groups(alleles):
    return [(g, a) for g, want in enumerate(alleles) for a in sorted({int(x) for x in want if int(x) >= 1})]


def _consensus_case(alleles, partial):
    groups, gid, anchor, n = place_consensus(TAG, H, UNIT_OF, alleles, partial)
    assert groups == _groups(alleles)                           # units ascending, alleles ascending
    assert gid.dtype == np.int32 and anchor.dtype == np.int32 and gid.shape == anchor.shape == TAG.shape
    want_gid, want_anchor = [-1] * len(TAG), [0] * len(TAG)
    want_n = {k: [0] * len(groups) for k in KINDS.values()}
    for j, (g, t, h) in enumerate(zip(UNIT_OF.tolist(), TAG.tolist(), H.tolist())):
        kind, a = am.place(NAME_OF[t], h, alleles[g])
        if kind is None or (kind != "whole" and not partial):
            continue
        k = groups.index((g, a))
        want_n[KINDS[kind]][k] += 1
        if kind in ("whole", "partial"):
            want_gid[j], want_anchor[j] = k, am.ANCHOR_OF_TAG[NAME_OF[t]]
    assert gid.tolist() == want_gid and anchor.tolist() == want_anchor, alleles
    assert sorted(n) == sorted(want_n) and all(n[k].tolist() == want_n[k] for k in want_n), alleles


def test_the_anchors_are_the_models():
    assert (_lib.PILEUP_ANCHOR_WHOLE, _lib.PILEUP_ANCHOR_BEGIN, _lib.PILEUP_ANCHOR_END) == (am.WHOLE, am.BEGIN, am.END)
    assert len(LISTS) == 1 + 8 + 64 + 512


def test_consensus_places_the_full_reads_as_the_model_does():
    for alleles in CASES:
        _consensus_case(alleles, False)


def test_consensus_partial_places_every_read_as_the_model_does():
    for alleles in CASES:
        _consensus_case(alleles, True)


def test_no_winner_and_no_allele():
    none = (np.zeros(0, np.uint8), np.zeros(0, np.int16), np.zeros(0, np.int64))
    groups, gid, anchor, n = place_consensus(*none, [[2, 1], []], True)
    assert groups == [(0, 1), (0, 2)] and gid.shape == anchor.shape == (0,) and gid.dtype == np.int32
    assert all(n[k].tolist() == [0, 0] for k in KINDS.values())
    groups, gid, _, n = place_consensus(TAG, H, UNIT_OF, [[], [0, -1]], True)
    assert groups == [] and (gid == -1).all() and all(len(n[k]) == 0 for k in KINDS.values())
    groups, gid = place_spectrum(*none, [[3], [3]], [3, 12])
    assert groups == [(0, "full:3"), (0, "partial"), (0, "rept")] and gid.shape == (0,) and gid.dtype == np.int32


# ---- the spectrum's classes -------------------------------------------------------------------------------------------
# Unit 0 has period 3, unit 1 period 12 (no table: no group).  For model_classes every read of a unit shows ONE whole unit
# of its own, a 3-mer no other read of the unit shows: the `words` of a class then name the reads the model counted in it.
WORDS = ["".join(x) for x in itertools.product("ACGT", repeat=3)][:len(READS)]
LADDERS = [("TTTTT", "CAG", "GGGGG", 50), ("TTTTT", "CAGCAGCAGCAT", "GGGGG", 13)]


def _winners_for_the_model():
    w = types.SimpleNamespace()
    w.batch = types.SimpleNamespace(n_units=2, ladder_keys=LADDERS, text=lambda i: WORDS[i % len(READS)])
    w.items, w.unit_of, w.tag, w.h = np.arange(len(TAG)), UNIT_OF, TAG, H
    w.win = (2 * (H.astype(np.int32) - 1)).astype(np.int32)               # the forward template of h units
    w.fields = np.tile(np.array([3, 5, 7, 0, 2], np.int16), (len(TAG), 1))  # three columns from the tract's first on
    w.ops = np.full((len(TAG), 1), (3 << 4) | 0, np.uint32)
    w.n_ops = np.ones(len(TAG), np.int32)
    return w


def test_spectrum_classes_are_the_models():
    w = _winners_for_the_model()
    word_at = {x: j for j, x in enumerate(WORDS)}
    for alleles in CASES:
        groups, gid = place_spectrum(TAG, H, UNIT_OF, alleles, [3, 12])
        want = model_classes(w, alleles)
        # unit 0: every class of the model, full:a ascending, then partial, then rept; unit 1: nothing
        assert groups == [(0, "full:{}".format(a)) for a in sorted({x for x in alleles[0] if x >= 1})] + [(0, "partial"), (0, "rept")]
        assert sorted(name for _, name in groups) == sorted(want[0]), alleles
        want_gid = [-1] * len(TAG)
        for k, (_, name) in enumerate(groups):
            assert want[0][name]["reads"] == len(want[0][name]["words"])      # (one word per read, each its own)
            for x in want[0][name]["words"]:
                want_gid[word_at[x]] = k
        assert gid.dtype == np.int32 and gid.tolist() == want_gid, alleles


# ---- _Winners.take ----------------------------------------------------------------------------------------------------
def test_take_cuts_an_item_list_out_of_the_winners():
    rng = np.random.default_rng(5)
    texts = ["".join(rng.choice(list("ACGTN"), n)) for n in (1, 15, 16, 17, 32, 33)]
    m, cap = len(texts), 3
    w = _Winners()
    w.packed, w.read_off, w.read_len = _lib.pack_reads(texts)
    one = [_lib.pack_reads([t]) for t in texts]                             # every read packed on its own: its slice
    assert all(np.array_equal(w.packed[w.read_off[k]:w.read_off[k + 1]], one[k][0][:one[k][1][1]]) for k in range(m))
    # (strided sources of other dtypes: take must hand over contiguous arrays of the documented ones)
    w.item_ladder = np.arange(10, 10 + 2 * m, dtype=np.int64)[::2]
    w.win = rng.integers(0, 40, 2 * m)[::2]
    w.fields = rng.integers(0, 200, (m, 6)).astype(np.int64)[:, :5]
    w.ops = rng.integers(0, 1 << 12, (m, 2 * cap)).astype(np.uint64)[:, ::2]
    w.n_ops = rng.integers(0, cap + 1, m)
    w.cap = cap
    kinds = (np.uint32, np.int64, np.int32, np.int32, np.int32, np.int16, np.uint32, np.int32)
    for sel in ([], [4], list(range(m))[::-1], [5, 0, 5, 5, 2, 0], np.array([3, 1], np.int32)):
        got = w.take(sel)
        assert len(got) == len(kinds)
        assert all(x.dtype == dt and x.flags["C_CONTIGUOUS"] for x, dt in zip(got, kinds)), sel
        packed, read_off, read_len, item_ladder, win, fields, ops, n_ops = got
        idx = [int(k) for k in sel]
        assert read_off.shape == (len(idx) + 1,) and read_off[0] == 0 and read_off[-1] == len(packed)
        assert read_len.tolist() == [len(texts[k]) for k in idx]
        for j, k in enumerate(idx):
            assert np.array_equal(packed[read_off[j]:read_off[j + 1]], w.packed[w.read_off[k]:w.read_off[k + 1]]), (sel, j)
        ix = np.asarray(idx, np.int64)
        assert np.array_equal(item_ladder, w.item_ladder[ix]) and np.array_equal(win, w.win[ix])
        assert np.array_equal(n_ops, w.n_ops[ix])
        assert fields.shape == (len(idx), 5) and np.array_equal(fields, w.fields[ix])
        assert ops.shape == (len(idx), cap) and np.array_equal(ops, w.ops[ix])


# ---- the reports' members of a run() argument tuple ---------------------------------------------------------------------
def test_option_tail_and_options_agree_on_every_combination():
    base = ("s", "x.bam", None, ["HD"], 300, False, False, True, True, "INFO")
    names = ("alignments", "consensus", "consensus_partial", "spectrum")
    seen = 0
    for flags in itertools.product((False, True), repeat=4):
        want = dict(zip(names, flags))
        if want["consensus_partial"] and not want["consensus"]:
            continue
        seen += 1
        o = _options(base + option_tail(*flags))
        assert {k: o[k] for k in names} == want and all(type(o[k]) is bool for k in names)
        assert o["reports"] == [k for k in REPORTS if want[k]]
        assert o == _options(base + option_tail(**want))
    assert seen == 12 and REPORTS == ("alignments", "consensus", "spectrum")
    assert option_tail() == () and _options(base)["reports"] == []
