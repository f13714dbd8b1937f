"""The second tier of sw_cont_kernel's bounded-gain exit and its one-test short-cut, on top of tests/sw_exit_model.py.

The kernel (csrc/sw_ladder.hip: steady_exit, SW_EXIT_BOUND = 2) asks the bounded-gain test with the bound
G2(row) = match * min(L - 1 - row, 5 + Wtail[lane of row]) in its 7- and 10-row production instantiations -- sw_exit_model's
rule "tier2" -- and, once some read of the wave has a candidate, asks that test alone: a failed test no longer falls through
to the two-boundary test.  `replay` is sw_exit_model.replay with that short-cut; `ladder_passes` runs both passes of one
ladder's reads through either of the two, so that they can be compared wave by wave (tests/test_sw_tier2_model.py: same
columns, same arg-max words).

Run as a program it compares the two on a bench-shaped batch and prints the trunk columns by rule:

    python -m tests.sw_tier2_model [--samples 3] [--readlen 150] [--seed 1]
"""
import argparse
import sys

from . import sw_exit_model as xm


def kernel_rule(R, generic):
    """The rule sw_cont_kernel runs since the second tier: both tiers in the 7- and 10-row production instantiations (where
    the 6-mer premise does not hold the table says "no bound" and sw_exit_model's tier 2 is its tier 1), the old rule elsewhere."""
    return "tier2" if not generic and R in (7, 10) else "old"


def replay(st, idx, best, rule):
    """sw_exit_model.replay, except that once some read of the wave has a candidate a failed bounded-gain test ends the
    question for this template end: the two-boundary test is not asked and ok_run is left alone."""
    idx = list(idx)
    best = list(best)
    if st.tier2 and not any(st.W[i] >= st.thr for i in idx):
        return 0, best, "filter"
    if not any(st.still_open(i, 1, best[k]) for k, i in enumerate(idx)):
        return 0, best, "closed"
    M = st.M2 if rule == "tier2" else st.M1
    cols = st.alen
    ok_run = 0
    u = 1
    while True:
        cols += st.period
        need = [st.need(i, u, best[k]) for k, i in enumerate(idx)]
        dropped = not any(st.score[i, u] >= need[k] for k, i in enumerate(idx))
        if not dropped:
            for k, i in enumerate(idx):
                cand = (int(st.score[i, u]) << 9 | (511 - u)) << 3
                if st.tag[i, u] != xm.TAG_NONE and cand > (best[k] | 7):
                    best[k] = cand | int(st.tag[i, u])
        u += 1
        if not any(st.still_open(i, u, best[k]) for k, i in enumerate(idx)):
            return cols, best, "strand"
        if u > st.mu:
            return cols, best, "end"
        if not dropped or rule == "none":
            ok_run = 0
            continue
        if rule in ("tier1", "tier2") and any(x >= 0 for x in best):
            if all(M[u - 1, i] < st.need(i, u, best[k]) for k, i in enumerate(idx)):
                return cols, best, "new"
            continue                                     # the short-cut
        thr = st.alen + (st.period if ok_run else 0)
        if any(st.lo[u - 1, i] < thr for i in idx):
            ok_run = 0
        elif ok_run:
            return cols, best, "steady"
        else:
            ok_run = 1


def ladder_passes(reads, ladder, scoring, R, rules, clip=False, replays=(replay,)):
    """Both passes of one ladder's reads (sw_exit_model.ladder_passes without the per-read periods) under each rule and each
    of `replays` -> {(rule, replay index): dict(cols, waves, best, quads)}; quads: per wave (strand, reads, columns, reason)."""
    n = len(reads)
    st = [xm.Strand(reads, ladder, s, scoring, R, clip) for s in range(2)]
    out = {}
    for rule in rules:
        for ri, rp in enumerate(replays):
            best = [-1] * n
            cols = waves = 0
            log = []
            for s in range(2):
                members = [i for i in range(n) if (st[s].W[i] >= st[s].thr or not st[s].premise) and (s == 0 or st[1].still_open(i, 1, best[i]))]
                for quad in xm.pack_quads(st[s].W, members):
                    c, nb, why = rp(st[s], quad, [best[i] for i in quad], rule)
                    for i, b in zip(quad, nb):
                        best[i] = b
                    cols += c
                    waves += 1
                    log.append((s, tuple(quad), c, why))
            out[rule, ri] = dict(cols=cols, waves=waves, best=best, quads=log)
    return out


def compare_replays(reads, ladder, scoring, R, rules=("tier1", "tier2"), clip=False):
    """-> {rule: trunk columns}; asserts that the short-cut changes no wave's columns and no read's arg-max word."""
    res = ladder_passes(reads, ladder, scoring, R, rules, clip, replays=(xm.replay, replay))
    cols = {}
    for rule in rules:
        a, b = res[rule, 0], res[rule, 1]
        assert a["best"] == b["best"], (ladder, rule)
        assert [(q[0], q[1], q[2]) for q in a["quads"]] == [(q[0], q[1], q[2]) for q in b["quads"]], (ladder, rule)
        cols[rule] = b["cols"]
    return cols


def model_columns(quads, ladder, scoring, R, rules, clip=False):
    """Trunk columns of a list of quads that each are a ladder and unit of their own (tests/sw_exit_gpu_cases.py), by rule."""
    tot = {r: 0 for r in rules}
    for q in quads:
        res = ladder_passes(q, ladder, scoring, R, rules, clip)
        for r in rules:
            tot[r] += res[r, 0]["cols"]
    return tot


def main(argv=None):
    import numpy as np
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--readlen", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    from tredparse_amd import synth
    loci = [l for l in synth.load_loci() if l["name"] not in ("FXTAS", "AR")]
    b = synth.build_batch(args.seed, loci, args.samples, synth.SynthParams(readlen=args.readlen))
    R = xm.rows_per_lane(args.readlen)
    read_lad = np.repeat(b.unit_ladder, np.diff(b.unit_read_off))
    tot = {"tier1": 0, "tier2": 0}
    for li, lad in enumerate(b.ladders):
        reads = [synth.decode(b.codes[i]) for i in np.nonzero(read_lad == li)[0]]
        cols = compare_replays(reads, lad, (1, 5, 7, 2), R)
        for r in tot:
            tot[r] += cols[r]
        print("{:8s} reads {:5d}  trunk columns tier1 {:7d} tier2 {:7d}  (the short-cut changes nothing)".format(
            loci[li]["name"], len(reads), cols["tier1"], cols["tier2"]), flush=True)
    print("readlen", args.readlen, "reads", b.n_reads, "trunk columns tier1", tot["tier1"], "tier2", tot["tier2"],
          "{:+.2%}".format(tot["tier2"] / max(1, tot["tier1"]) - 1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
