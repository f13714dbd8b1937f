"""The cohort model of DESIGN 4 ("Cohort frequencies") in plain Python / numpy: the reference the GPU unit (csrc/cohort.hip)
and the host layer (tredparse_amd/cohort.py) are tested against.  Written from the text of include/tredcohort.h, not from the
kernels: one item is one locus with its samples, a sample is a pair list (a, b, lw) as tests/trio_model.py builds them and a
ploidy; the allele frequencies of the item by EM over the samples' (h1, h2) surfaces, exactly `iters` iterations, and a last
E-step that gives every sample its posterior over its pairs and its cohort-aware call.  Every sum is sequential in the
stated order: the samples in order, the pairs of a sample in order, a before b.

Item statuses and their precedence are the header's: BAD_ITEM, then TOO_LONG, then EMPTY.

evaluate(..., dtype=np.longdouble) is the same model with the weights, f, every sum, exp and log in long double: the reference
of the relative comparison (tests/cohort_compare.py).  The steps a wrong kernel could get wrong -- the weights, the factor of
a heterozygous pair, the counts, the choice of the call -- are small functions of their own, so that tests/test_cohort_model.py
can put a deliberately wrong one in their place and show that the comparison notices."""
import math

import numpy as np

OK, EMPTY, TOO_LONG, BAD_ITEM = 0, 1, 4, 5
ITERS, ALPHA, TOL = 64, 1.0, 1e-6
MAX_ALLELE = 1024
MAX_ITERS = 4096


def _seq_sum(x, dtype=np.float64):
    """The sum of x in list order."""
    return dtype(np.cumsum(np.asarray(x, dtype))[-1]) if len(x) else dtype(0.0)


def _log(x, dtype):
    return dtype(math.log(x)) if dtype is np.float64 else np.log(x)


def _weights(lw, m):
    """w = exp(lw - m), in the type of lw."""
    return np.exp(lw - m)


def _het(ia, ib):
    """The factor of a diploid pair: 2 where it is heterozygous."""
    return np.where(ia != ib, 2.0, 1.0)


def _pick(qs, a):
    """The call: max by (q, -a), the first of a full tie wins."""
    best = 0
    for k in range(1, len(qs)):
        if (qs[k], -a[k]) > (qs[best], -a[best]):
            best = k
    return best


def _lists(samples):
    return [None if s is None or len(s[0]) == 0 else tuple(np.asarray(x) for x in s) for s in samples]


def refusal(samples, ploidy):
    """The status the item is refused with, OK where it is not.  The ploidy of every sample is looked at, a sample with an
    empty list included; its pairs only where it has some."""
    lists = _lists(samples)
    bad = any(int(p) not in (1, 2) for p in ploidy)
    long_ = False
    for s, p in zip(lists, ploidy):
        if s is None:
            continue
        a, b, lw = s
        bad = bad or bool(((a > b) | (a < 0) | (b < 0) | ~np.isfinite(lw) | (lw > 0)).any())
        bad = bad or (int(p) == 1 and bool((a != b).any()))
        long_ = long_ or bool(((a > MAX_ALLELE) | (b > MAX_ALLELE)).any())
    if bad:
        return BAD_ITEM
    if long_:
        return TOO_LONG
    return EMPTY if all(s is None for s in lists) else OK


def _e_step(lists, ploidy, w, m, pos, f, dtype=np.float64):
    """One E-step under f: per sample q, Z and logZ (None, 0, 0 for a sample that takes no part), and n, the expected
    allele counts, summed sample by sample, pair by pair, a before b."""
    n = np.zeros(len(f), dtype)
    q, Z, logZ = [], [], []
    for s, p, ws, ms, ps in zip(lists, ploidy, w, m, pos):
        if s is None:
            q.append(None), Z.append(dtype(0.0)), logZ.append(dtype(0.0))
            continue
        ia, ib = ps
        if p == 1:
            qs = ws * f[ia]
        else:
            qs = ws * f[ia] * f[ib] * _het(ia, ib)
        Zs = _seq_sum(qs, dtype)
        r = qs / Zs
        if p == 1:
            np.add.at(n, ia, r)                                     # (unbuffered: in the order of the pairs)
        else:
            np.add.at(n, np.stack([ia, ib], 1).ravel(), np.stack([r, r], 1).ravel())
        q.append(qs), Z.append(Zs), logZ.append(ms + _log(Zs, dtype))
    return q, Z, logZ, n


def evaluate(samples, ploidy, iters=ITERS, alpha=ALPHA, tol=TOL, dtype=np.float64):
    """One item.  samples: per sample (a, b, lw) or None; ploidy: per sample (or one for all).  Returns a dict: status,
    alleles, freq, count, C, trace [iters][2], delta, converged, objective [iters] (the penalised log-likelihood under
    f_{t-1}) and per sample -- None where it takes no part -- index, call, post, logZ, r, q, gap (best log q minus the
    second's, inf for one pair) and beyond (the same to the largest q that is not equal to the best, inf where there is
    none: what separates a group of exactly tied pairs from the rest).  dtype: the type of the arithmetic."""
    if not (1 <= int(iters) <= MAX_ITERS) or not (alpha > 0 and math.isfinite(alpha)):
        raise ValueError("parameters out of range")
    ploidy = [int(p) for p in np.broadcast_to(np.asarray(ploidy), (len(samples),))]
    ns = len(samples)
    status = refusal(samples, ploidy)
    if status != OK:
        return dict(status=status, alleles=np.zeros(0, np.int32), freq=np.zeros(0), count=np.zeros(0), C=0,
                    trace=np.zeros((iters, 2)), delta=0.0, converged=False, objective=np.zeros(iters), index=[None] * ns,
                    call=[None] * ns, post=[None] * ns, logZ=[None] * ns, r=[None] * ns, q=[None] * ns, gap=[None] * ns,
                    beyond=[None] * ns)
    lists = _lists(samples)
    alleles = sorted(set(x for s in lists if s is not None for x in s[0].tolist() + s[1].tolist()))
    rank = {c: j for j, c in enumerate(alleles)}
    A = len(alleles)
    C = sum(p for s, p in zip(lists, ploidy) if s is not None)
    w, m, pos = [], [], []
    for s in lists:
        if s is None:
            w.append(None), m.append(dtype(0.0)), pos.append(None)
            continue
        lw = s[2].astype(np.float64).astype(dtype)
        m.append(dtype(lw.max()))
        w.append(_weights(lw, m[-1]))
        pos.append((np.array([rank[x] for x in s[0].tolist()], np.int64), np.array([rank[x] for x in s[1].tolist()], np.int64)))
    alpha = dtype(alpha)
    f = np.full(A, dtype(1.0) / A, dtype)
    trace, objective = np.zeros((iters, 2), dtype), np.zeros(iters, dtype)
    for t in range(iters):
        _, _, logZ, n = _e_step(lists, ploidy, w, m, pos, f, dtype)
        new = (n + alpha / A) / (C + alpha)
        trace[t] = (_seq_sum(logZ, dtype), np.abs(new - f).max())
        objective[t] = trace[t, 0] + (alpha / A) * _seq_sum(np.log(f), dtype)
        f = new
    q, Z, logZ, n = _e_step(lists, ploidy, w, m, pos, f, dtype)
    out = dict(status=OK, alleles=np.array(alleles, np.int32), freq=f, count=n, C=C, trace=trace, delta=float(trace[-1, 1]),
               converged=bool(trace[-1, 1] < tol), objective=objective, index=[], call=[], post=[], logZ=[], r=[], q=[], gap=[],
               beyond=[])
    for s, qs, Zs, lz in zip(lists, q, Z, logZ):
        if s is None:
            for name in ("index", "call", "post", "logZ", "r", "q", "gap", "beyond"):
                out[name].append(None)
            continue
        best = _pick(qs, s[0])
        r = qs / Zs
        order = np.sort(qs)
        rest = order[order != order[-1]]
        with np.errstate(divide="ignore"):
            gap = float(np.log(order[-1]) - np.log(order[-2])) if len(qs) > 1 else math.inf
            beyond = float(np.log(order[-1]) - np.log(rest[-1])) if len(rest) else math.inf
        out["index"].append(best), out["call"].append((int(s[0][best]), int(s[1][best]))), out["post"].append(r[best])
        out["logZ"].append(lz), out["r"].append(r), out["q"].append(qs), out["gap"].append(gap), out["beyond"].append(beyond)
    return out
