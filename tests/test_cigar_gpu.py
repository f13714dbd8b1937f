"""GPU: the CIGAR kernel (include/tredcigar.h, tredparse_amd/csrc/sw_cigar.hip) against the CIGARs of the compiled
reference (tests/golden/sw_cigar.npz) and against tests/cigar_model.py where the reference itself would run off its
buffers; and ssw.Aligner(report_cigar=True) against the reference's own texts."""
import numpy as np
import pytest

from tredparse_amd import _lib, ssw

from . import cigar_model as cm

pytestmark = pytest.mark.gpu
CAP = 32


def _params():
    return _lib.default_sw_params()


def _run(ctx, g, idx, fields=None, cap=CAP):
    reads = [g["reads"][k] for k in idx]
    packed, woff, rlen = _lib.pack_reads(reads)
    n = len(idx)
    ops, n_ops, status = np.full((n, cap), 7, np.uint32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    f = np.ascontiguousarray(g["fields"][idx] if fields is None else fields, np.int16)
    ctx.sw_cigar(_lib.MEM_HOST, packed, woff, rlen, n, np.ascontiguousarray(g["ladder"][idx]),
                 np.ascontiguousarray(g["template"][idx]), f, _params(), cap, ops, n_ops, status, ladders=g["ladders"])
    return ops, n_ops, status


def _check(g, idx, ops, n_ops, status):
    for i, k in enumerate(idx):
        want = g["ops"][k]
        assert status[i] == _lib.CIGAR_OK and n_ops[i] == len(want), (k, g["cls"][k], status[i], n_ops[i], want)
        assert list(ops[i, :n_ops[i]]) == want and not ops[i, n_ops[i]:].any(), (k, g["cls"][k], list(ops[i]), want)


def test_every_golden_item_host_memory(ctx):
    g = cm.golden()
    idx = np.arange(len(g["reads"]))
    assert max(len(o) for o in g["ops"]) <= CAP
    _check(g, idx, *_run(ctx, g, idx))


def test_every_golden_item_device_memory(ctx):
    import torch
    g = cm.golden()
    n = len(g["reads"])
    packed, woff, rlen = _lib.pack_reads(g["reads"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_in = [dev(packed.view(np.int32)), dev(woff), dev(rlen), dev(g["ladder"]), dev(g["template"]), dev(g["fields"])]
    ops = torch.full((n, CAP), 7, dtype=torch.int32, device="cuda")
    n_ops = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.sw_cigar(_lib.MEM_DEVICE, d_in[0], d_in[1], d_in[2], n, d_in[3], d_in[4], d_in[5], _params(), CAP, ops, n_ops, status,
                 ladders=g["ladders"])
    ctx.sync()
    _check(g, np.arange(n), ops.cpu().numpy().view(np.uint32), n_ops.cpu().numpy(), status.cpu().numpy())


def test_fields_of_sw_classify_hand_over(ctx):
    """Every synthetic item again, placed by sw_classify's own dump row instead of the recorded fields."""
    g = cm.golden()
    idx = np.array([k for k, c in enumerate(g["cls"]) if c != "a"])
    reads = [g["reads"][k] for k in idx]
    n = len(idx)
    ctx.set_ladders(g["ladders"])
    packed, woff, rlen = _lib.pack_reads(reads)
    nt = max(max(2 * l[3], 1) for l in g["ladders"])
    tag, h, sc = np.zeros(n, np.uint8), np.zeros(n, np.int16), np.zeros(n, np.int16)
    dump = np.zeros((n, nt, 6), np.int16)
    ctx.sw_classify(_lib.MEM_HOST, packed, woff, rlen, n, np.arange(n + 1, dtype=np.int32),
                    np.ascontiguousarray(g["ladder"][idx]), n, _params(), tag, h, sc, dump, nt)
    fields = np.ascontiguousarray(dump[np.arange(n), g["template"][idx], :5])
    assert np.array_equal(fields, g["fields"][idx])
    _check(g, idx, *_run(ctx, g, idx, fields=fields))


def test_overflow_reports_the_true_count_and_spares_the_neighbours(ctx):
    g = cm.golden()
    big = max(range(len(g["ops"])), key=lambda k: len(g["ops"][k]))
    cap = len(g["ops"][big]) - 1
    assert cap >= 2
    small = [k for k in range(len(g["ops"])) if len(g["ops"][k]) <= cap][:130]
    idx = np.array(small[:65] + [big] + small[65:])
    ops, n_ops, status = _run(ctx, g, idx, cap=cap)
    assert status[65] == _lib.CIGAR_OVERFLOW and n_ops[65] == cap + 1 and not ops[65].any()
    keep = np.arange(len(idx)) != 65
    _check(g, idx[keep], ops[keep], n_ops[keep], status[keep])


def test_fields_of_another_pair_are_no_path(ctx):
    """A score the rectangle cannot reach: the reference doubles its band until it runs off its buffers; here the band
    stops at the rectangle and the item gets NO_PATH -- an ordinary status, and the next call works."""
    g = cm.golden()
    idx = np.array([k for k, c in enumerate(g["cls"]) if c in "de"][:40])
    fields = np.array(g["fields"][idx])
    odd = np.arange(len(idx)) % 2 == 1
    fields[odd, 0] += 60
    for i in np.nonzero(odd)[0][:6]:
        assert cm.cigar_of(g["refs"][idx[i]], g["reads"][idx[i]], fields[i]) == (cm.NO_PATH, [])
    ops, n_ops, status = _run(ctx, g, idx, fields=fields)
    assert (status[odd] == _lib.CIGAR_NO_PATH).all() and not n_ops[odd].any() and not ops[odd].any()
    _check(g, idx[~odd], ops[~odd], n_ops[~odd], status[~odd])
    ctx.sync()
    _check(g, idx, *_run(ctx, g, idx))
    # items that name no pair at all: status, never an access
    bad = np.array(g["fields"][idx])
    bad[0, 2] = 600
    bad[1, 3] = -1
    bad[2, 4] = 500
    _, n_ops, status = _run(ctx, g, idx, fields=bad)
    assert list(status[:3]) == [_lib.CIGAR_BAD_ITEM] * 3 and (status[3:] == 0).all()


def test_aligner_report_cigar_gives_the_references_text(ctx):
    g = cm.golden()
    by_ref = {}
    for k, ref in enumerate(g["refs"]):
        by_ref.setdefault(ref, []).append(k)
    ctx.reset_timing()
    calls = 0
    for ref, ks in by_ref.items():
        al = ssw.Aligner(ref, 1, 5, 7, 2, report_cigar=True, ctx=ctx).align_many([g["reads"][k] for k in ks])
        calls += 1
        for k, a in zip(ks, al):
            t = g["texts"][k]
            assert a.cigar_string == a.cigar == t["cigar_string"], k
            assert list(a.alignment) == t["alignment"] and str(a) == t["str"], k
            assert a.score2 is None
    assert ctx.get_timing(_lib.KERNEL_CIGAR)[0] == calls            # ONE sw_cigar call per align_many
    # the default: nothing new is launched
    ctx.reset_timing()
    ref, ks = next(iter(by_ref.items()))
    a = ssw.Aligner(ref, 1, 5, 7, 2, ctx=ctx).align(g["reads"][ks[0]])
    assert ctx.get_timing(_lib.KERNEL_CIGAR)[0] == 0 and ctx.get_timing(_lib.KERNEL_SW)[0] == 1
    assert a.cigar_string == "" and a.alignment == ("", "", "") and "Cigar_string" not in str(a)
    # a filtered query gets None and no CIGAR work of its own
    assert ssw.Aligner(ref, 1, 5, 7, 2, report_cigar=True, ctx=ctx).align("ACGT", min_score=30) is None
