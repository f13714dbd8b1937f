#!/usr/bin/env python3
"""Record the reference's CIGARs as golden vectors: tests/golden/sw_cigar.npz, and tests/golden/alignments_t001_HD.txt,
the --alignments report of t001 / HD put together from the reference's texts of the (a) items.

BUILD-CONTAINER ONLY (CPU): every alignment is the reference's own -- src/ssw.c compiled into oracle/_ref/libssw.so,
driven through the reference's ssw_wrap.Aligner / PyAlignRes (tools/refshim.py), so the recorded `cigar_string`,
`alignment` and `str()` are its text.  The alignments run in child processes that report item by item: a fault of the
reference's CIGAR pass (oracle/ref_driver.c:15-23) ends one child, loses that one item, and a fresh child goes on
with the rest.  Nothing of the reference is stored, only these inputs and outputs.

    python tools/gen_golden_cigar.py                        tests/golden/sw_cigar.npz at 1/5/7/2 (and the report)
    python tools/gen_golden_cigar.py --scoring 2/2/3/1 ...   tests/golden/sw_cigar_scorings.npz: a draw of its own of the
                                                            classes b-e (reads of 36-250 bp) per scoring given

Scoring is 1/5/7/2 (bam_parser.py:95-98) unless --scoring says otherwise.  Items:
  a  the winning (read, template) pair of every `details` read of t001/HD and t002/DM1 (run_t001_t002.json)
  b  synthetic reads of 36/100/150/250/480 bp on ladders of period 3/4/5/6/12, both strands, 1 % substitutions and N
  c  the same reads against a template one or two units off: a single I or D of 3-24 bases, band > 1 from the start
  d  plain references with one 3-base deletion and one 3-base insertion >= 40 bases apart (refLen == readLen: the band
     starts at 1 and doubles twice), and the 6-base variant (three doublings)
  e  an indel close to an end of the alignment (a local alignment never STARTS or ENDS with a gap -- dropping the gap
     and what lies beyond it scores higher -- so the traceback's closing `e op + 1M` branch cannot be reached from
     ssw_align; the count of items whose first or last operation is a gap is printed: 0)
  f  one 480 x 511 item and one single-M item of 15 bases, and short exact matches around them
An item is kept only if the reference returned and its operations consume exactly the aligned query and reference
bases; no item of (a) may be excluded, at most 2 % of (b)-(f), and (c)-(f) keep at least 10 items each.
"""
import json
import math
import os
import random
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCORING = dict(match=1, mismatch=5, gap_open=7, gap_extend=2)
SCORINGS_FILE = os.path.join(ROOT, "tests", "golden", "sw_cigar_scorings.npz")


def parse_scoring(text):
    """'m/x/o/e' -> the Aligner's keyword arguments."""
    m, x, o, e = (int(v) for v in text.split("/"))
    return dict(match=m, mismatch=x, gap_open=o, gap_extend=e)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def template(ladder, t):
    """Template t of a ladder in db order (u=1 fwd, u=1 rc, u=2 fwd, ...); max_units 0: the plain reference."""
    prefix, repeat, suffix, mu = ladder
    if mu == 0:
        return prefix
    s = prefix + repeat * (t // 2 + 1) + suffix
    return rc(s) if t % 2 else s


# ---- the child: the reference, item by item -----------------------------------------------------------------------
def worker(scoring=SCORING):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import refshim
    ref = refshim.load_reference()
    res_cls = ref.ssw.PyAlignRes
    raw_op = res_cls.cigar_int_to_op
    res_cls.cigar_int_to_op = staticmethod(lambda v: raw_op(v).decode())     # c_char is bytes under Python 3
    for line in sys.stdin:
        ref_seq, read = json.loads(line)
        al = ref.ssw.Aligner(ref_seq=ref_seq, report_secondary=False, **scoring).align(read)
        out = {"fields": [al.score, al.ref_begin, al.ref_end, al.query_begin, al.query_end],
               "ops": [int(v) & 0xFFFFFFFF for v in al._cigar_string], "cigar_string": al.cigar_string,
               "alignment": list(al.alignment), "str": str(al)}
        sys.stdout.write(json.dumps(out) + "\n")
        sys.stdout.flush()


def run_reference(pairs, chunk=200, scoring=SCORING):
    """[result dict or None (the reference faulted)] for every (ref_seq, read)."""
    out = [None] * len(pairs)
    k = 0
    tag = "{match}/{mismatch}/{gap_open}/{gap_extend}".format(**scoring)
    while k < len(pairs):
        part = pairs[k:k + chunk]
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tag], input="".join(json.dumps(x) + "\n" for x in part),
                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, universal_newlines=True)
        lines = [l for l in p.stdout.split("\n") if l.endswith("}")]
        for i, l in enumerate(lines):
            out[k + i] = json.loads(l)
        k += len(lines) + (0 if len(lines) == len(part) else 1)       # the item the child died on is skipped
    return out


# ---- the items ------------------------------------------------------------------------------------------------------
def mutate(rng, s, sub=0.01, n=0.005):
    o = []
    for c in s:
        r = rng.random()
        o.append(rng.choice([b for b in "ACGT" if b != c]) if r < sub else "N" if r < sub + n else c)
    return "".join(o)


def randseq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def build(rng):
    from tredparse_amd import synth
    ladders, items = [], []          # items: (class, ladder, template, read, meta)

    def ladder_id(l):
        l = tuple(l)
        if l not in ladders:
            ladders.append(l)
        return ladders.index(l)

    # a: real reads -- every template of the locus' ladder is aligned, the winner kept (bam_parser.py:123-174)
    loci = {x["name"]: x for x in synth.load_loci()}
    with open(os.path.join(ROOT, "tests", "golden", "run_t001_t002.json")) as fp:
        run = json.load(fp)["samples"]
    real = []
    for sample, name in (("t001", "HD"), ("t002", "DM1")):
        x = loci[name]
        lad = ladder_id((x["prefix"], x["repeat"], x["suffix"], int(math.ceil(150. / len(x["repeat"])))))
        for d in run[sample][name + ".details"]:
            real.append((lad, d, sample, name))
    # b, c: synthetic ladders
    motifs = {3: "CAG", 4: "CCTG", 5: "ATTCT", 6: "GGCCTG", 12: "CCCCGCCCCGCG"}
    for readlen in (36, 100, 150, 250, 480):
        for period, motif in sorted(motifs.items()):
            mu = -(-readlen // period)
            flank = min(30, (511 - mu * period) // 2)
            lad = ladder_id((randseq(rng, flank), motif, randseq(rng, flank), mu))
            for strand in (0, 1):
                for rep in range(2):
                    u = mu if rep == 0 else rng.randint(max(1, mu // 4), mu)      # rep 0: a read of the full length
                    t = 2 * (u - 1) + strand
                    src = template(ladders[lad], t)
                    L = min(readlen, len(src))
                    at = rng.choice([0, len(src) - L, rng.randint(0, len(src) - L)])
                    read = mutate(rng, src[at:at + L])
                    items.append(("b", lad, t, read))
                    for off in ([-1, 1, 2] if rep == 0 else [-2, 1]):                 # c: a unit or two off
                        u2 = u + off
                        if 1 <= u2 <= mu and 3 <= abs(off) * period <= 24 and at == 0 and L == len(src):
                            items.append(("c", lad, 2 * (u2 - 1) + strand, read))
    # c needs reads that span the whole tract: short templates read end to end
    for period, motif in sorted(motifs.items()):
        for k in range(8):
            mu = -(-150 // period)
            lad = ladder_id((randseq(rng, 20), motif, randseq(rng, 20), mu))
            u = rng.randint(3, min(mu - 2, 100 // period))
            strand = k % 2
            read = mutate(rng, template(ladders[lad], 2 * (u - 1) + strand), n=0.0)
            for off in (-2, -1, 1, 2):
                if 1 <= u + off <= mu and abs(off) * period <= 24:
                    items.append(("c", lad, 2 * (u + off - 1) + strand, read))
    # d: compensating indels on plain references
    for k in range(36):
        g = 3 if k < 24 else 6
        n = rng.choice([150, 200, 250])
        ref = randseq(rng, n + 20)
        p1 = rng.randint(45, n - 100)
        p2 = p1 + rng.randint(40, n - 45 - p1)
        body = ref[10:10 + n]
        if k % 2:
            read = body[:p1] + body[p1 + g:p2] + randseq(rng, g) + body[p2:]
        else:
            read = body[:p1] + randseq(rng, g) + body[p1:p2] + body[p2 + g:]
        items.append(("d", ladder_id((ref, "A", "", 0)), 0, read))
    # e: an indel close to an end of the alignment
    for k in range(30):
        n = rng.choice([60, 100, 150])
        ref = randseq(rng, n + 30)
        body = ref[15:15 + n]
        g, d = rng.randint(1, 3), rng.randint(12, 16)
        p = d if k % 2 else n - d - g
        read = body[:p] + body[p + g:] if k % 4 < 2 else body[:p] + randseq(rng, g) + body[p:]
        items.append(("e", ladder_id((ref, "A", "", 0)), 0, read))
    # f: the extremes
    ref = randseq(rng, 511)
    items.append(("f", ladder_id((ref, "A", "", 0)), 0, mutate(rng, ref[20:500])))
    ref = randseq(rng, 40)
    items.append(("f", ladder_id((ref, "A", "", 0)), 0, ref[12:27]))
    for k in range(12):
        n = rng.randint(15, 40)
        ref = randseq(rng, n + rng.randint(0, 30))
        at = rng.randint(0, len(ref) - n)
        items.append(("f", ladder_id((ref, "A", "", 0)), 0, ref[at:at + n]))
    return ladders, real, items


def main():
    rng = random.Random(20261017)
    ladders, real, items = build(rng)
    # a: the winner among all templates of the ladder
    pairs, owner = [], []
    for k, (lad, d, _, _) in enumerate(real):
        for t in range(2 * ladders[lad][3]):
            pairs.append((template(ladders[lad], t), d["seq"]))
            owner.append((k, t))
    res = run_reference(pairs)
    assert all(r is not None for r in res), "the reference faulted on a real read"
    FLANK = 9
    chosen = {}
    for (k, t), r, (target, seq) in zip(owner, res, pairs):
        sc, rb, re_, qb, qe = r["fields"]
        min_len = min(len(seq), len(target)) // 2
        if not (sc >= max(min_len, 30) and qe - qb + 1 >= min_len):
            continue
        units, period = t // 2 + 1, len(ladders[real[k][0]][1])
        hang = min(len(target) - re_ - 1 + qb, rb + len(seq) - qe - 1, rb + len(target) - re_ - 1, qb + len(seq) - qe - 1)
        pre, suf = rb < FLANK, re_ > len(target) - FLANK - 1
        mu = ladders[real[k][0]][3]
        tag = "HANG" if hang >= FLANK else ("FULL" if suf else "PREF") if pre else "POST" if suf else \
            "REPT" if units >= mu - 1 and units * period <= len(seq) else None
        if tag is None:
            continue
        key = (sc, -units)
        if k not in chosen or key > chosen[k][0]:
            chosen[k] = (key, t, r, tag)
    done = []
    report = []
    for k, (lad, d, sample, name) in enumerate(real):
        key, t, r, tag = chosen[k]
        assert (tag, -key[1]) == (d["tag"], d["h"]), (d, tag, key)          # the winner is the pair the read was counted for
        done.append(("a", lad, t, d["seq"], r))
        if (sample, name) == ("t001", "HD"):
            # tred.py --alignments: a header, the reference's verbose block (bam_parser.py:145-147), a blank line
            report.append(">{} {} h={} {} {}\n".format(name, tag, d["h"], "-" if t % 2 else "+", d["id"]))
            report.append("\n".join(["{} {}".format(t // 2 + 1, template(ladders[lad], t)), r["str"].strip()] + r["alignment"]) + "\n\n")
    with open(os.path.join(ROOT, "tests", "golden", "alignments_t001_HD.txt"), "w") as fp:
        fp.write("".join(report))
    res = run_reference([(template(ladders[lad], t), read) for _, lad, t, read in items])
    done += [(c, lad, t, read, r) for (c, lad, t, read), r in zip(items, res)]

    kept, excluded = [], {}
    total = {}
    for c, lad, t, read, r in done:
        total[c] = total.get(c, 0) + 1
        ok = r is not None and len(r["ops"]) > 0
        if ok:
            q = sum(v >> 4 for v in r["ops"] if v & 15 in (0, 1))
            rr = sum(v >> 4 for v in r["ops"] if v & 15 in (0, 2))
            f = r["fields"]
            ok = q == f[4] - f[3] + 1 and rr == f[2] - f[1] + 1
        if ok:
            kept.append((c, lad, t, read, r))
        else:
            excluded[c] = excluded.get(c, 0) + 1
    n_kept = {c: sum(1 for k in kept if k[0] == c) for c in total}
    synth_total = sum(v for c, v in total.items() if c != "a")
    synth_excl = sum(v for c, v in excluded.items() if c != "a")
    assert excluded.get("a", 0) == 0, excluded
    assert synth_excl <= 0.02 * synth_total, (excluded, total)
    assert all(n_kept[c] >= 10 for c in "cdef"), n_kept
    gaps = sum(1 for k in kept if any(v & 15 for v in k[4]["ops"]))
    end_gap = sum(1 for k in kept if k[4]["ops"][0] & 15 or k[4]["ops"][-1] & 15)
    many = sum(1 for k in kept if len(k[4]["ops"]) > 3)
    meta = {"generator": "tools/gen_golden_cigar.py: the reference's ssw_wrap.Aligner (src/ssw.c compiled, via tools/refshim.py), "
                         "scoring 1/5/7/2", "scoring": SCORING, "ladders": [list(l) for l in ladders], "total": total,
            "kept": n_kept, "excluded": excluded, "with_gap": gaps, "more_than_3_ops": many, "first_or_last_op_is_gap": end_gap,
            "texts": [{"cigar_string": k[4]["cigar_string"], "alignment": k[4]["alignment"], "str": k[4]["str"]} for k in kept]}
    print(json.dumps({k: v for k, v in meta.items() if k not in ("ladders", "texts")}, indent=1))
    ops_off = np.zeros(len(kept) + 1, np.int64)
    ops_off[1:] = np.cumsum([len(k[4]["ops"]) for k in kept])
    np.savez_compressed(
        os.path.join(ROOT, "tests", "golden", "sw_cigar.npz"),
        cls=np.array([k[0] for k in kept]), ladder=np.array([k[1] for k in kept], np.int32),
        template=np.array([k[2] for k in kept], np.int32), reads=np.array([k[3] for k in kept]),
        fields=np.array([k[4]["fields"] for k in kept], np.int16), ops_off=ops_off,
        ops=np.array([v for k in kept for v in k[4]["ops"]], np.uint32), meta=np.array(json.dumps(meta)))


def build_small(rng):
    """About 60 items of the classes b-e with reads of 36-250 bp: (ladders, items) as build() gives them."""
    ladders, items = [], []

    def ladder_id(l):
        ladders.append(tuple(l))
        return len(ladders) - 1

    motifs = {3: "CAG", 4: "CCTG", 5: "ATTCT", 6: "GGCCTG", 12: "CCCCGCCCCGCG"}
    for readlen in (36, 100, 150, 250):                               # b: periodic ladders, both strands
        for period in rng.sample(sorted(motifs), 2):
            mu = -(-readlen // period)
            lad = ladder_id((randseq(rng, 30), motifs[period], randseq(rng, 30), mu))
            for strand in (0, 1):
                u = mu if strand == 0 else rng.randint(max(1, mu // 4), mu)
                src = template(ladders[lad], 2 * (u - 1) + strand)
                L = min(readlen, len(src))
                at = rng.choice([0, len(src) - L, rng.randint(0, len(src) - L)])
                items.append(("b", lad, 2 * (u - 1) + strand, mutate(rng, src[at:at + L])))
    for period, motif in sorted(motifs.items()):                      # c: a unit or two off, read end to end
        for k in range(2):
            mu = -(-150 // period)
            lad = ladder_id((randseq(rng, 20), motif, randseq(rng, 20), mu))
            u = rng.randint(3, min(mu - 2, 100 // period))
            strand = k % 2
            read = mutate(rng, template(ladders[lad], 2 * (u - 1) + strand), n=0.0)
            for off in rng.sample([-2, -1, 1, 2], 2):
                if 1 <= u + off <= mu and abs(off) * period <= 24:
                    items.append(("c", lad, 2 * (u + off - 1) + strand, read))
    for k in range(14):                                               # d: compensating indels on plain references
        g = rng.choice([1, 3, 3, 6])
        n = rng.choice([100, 150, 200, 250])
        ref = randseq(rng, n + 20)
        p1 = rng.randint(25, n // 2 - 10)
        p2 = p1 + rng.randint(30, n - 25 - p1)
        body = ref[10:10 + n]
        if k % 2:
            read = body[:p1] + body[p1 + g:p2] + randseq(rng, g) + body[p2:]
        else:
            read = body[:p1] + randseq(rng, g) + body[p1:p2] + body[p2 + g:]
        items.append(("d", ladder_id((ref, "A", "", 0)), 0, mutate(rng, read)))
    for k in range(14):                                               # e: an indel close to an end, or a long one
        n = rng.choice([36, 60, 100, 150])
        ref = randseq(rng, n + 30)
        body = ref[15:15 + n]
        g, d = (rng.randint(1, 3), rng.randint(8, 16)) if k < 8 else (rng.choice([12, 24]), n // 2 - 12)
        p = d if k % 2 else n - d - g
        read = body[:p] + body[p + g:] if k % 4 < 2 else body[:p] + randseq(rng, g) + body[p:]
        items.append(("e", ladder_id((ref, "A", "", 0)), 0, read))
    return ladders, items


def main_scorings(texts):
    """tests/golden/sw_cigar_scorings.npz: per scoring a draw of build_small, the reference's fields and operations."""
    ladders, rows, kept_n, excl_n, cigars = [], [], {}, {}, []
    for text in texts:
        scoring = parse_scoring(text)
        rng = random.Random("20261018 " + text)
        lads, items = build_small(rng)
        res = run_reference([(template(lads[lad], t), read) for _, lad, t, read in items], scoring=scoring)
        kept = 0
        for (c, lad, t, read), r in zip(items, res):
            ok = r is not None and len(r["ops"]) > 0
            if ok:
                q = sum(v >> 4 for v in r["ops"] if v & 15 in (0, 1))
                rr = sum(v >> 4 for v in r["ops"] if v & 15 in (0, 2))
                f = r["fields"]
                ok = q == f[4] - f[3] + 1 and rr == f[2] - f[1] + 1
            if not ok:
                continue
            kept += 1
            rows.append((c, len(ladders) + lad, t, read, r, [scoring[k] for k in ("match", "mismatch", "gap_open", "gap_extend")]))
            cigars.append(r["cigar_string"])
        ladders += lads
        kept_n[text], excl_n[text] = kept, len(items) - kept
        assert excl_n[text] <= 0.02 * len(items), (text, kept_n, excl_n)
    used = sorted({r[1] for r in rows})                               # ladders no kept item refers to are dropped
    renum = {l: i for i, l in enumerate(used)}
    meta = {"generator": "tools/gen_golden_cigar.py --scoring: the reference's ssw_wrap.Aligner (src/ssw.c compiled, via "
                         "tools/refshim.py), classes b-e, one draw per scoring", "scorings": list(texts),
            "ladders": [list(ladders[l]) for l in used], "kept": kept_n, "excluded": excl_n,
            "with_gap": {t: sum(1 for r in rows if "/".join(map(str, r[5])) == t and any(v & 15 for v in r[4]["ops"])) for t in texts},
            "more_than_3_ops": {t: sum(1 for r in rows if "/".join(map(str, r[5])) == t and len(r[4]["ops"]) > 3) for t in texts},
            "cigar_string": cigars}
    print(json.dumps({k: v for k, v in meta.items() if k not in ("ladders", "cigar_string")}, indent=1))
    ops_off = np.zeros(len(rows) + 1, np.int64)
    ops_off[1:] = np.cumsum([len(r[4]["ops"]) for r in rows])
    np.savez_compressed(
        SCORINGS_FILE, cls=np.array([r[0] for r in rows]), ladder=np.array([renum[r[1]] for r in rows], np.int32),
        template=np.array([r[2] for r in rows], np.int32), reads=np.array([r[3] for r in rows]),
        fields=np.array([r[4]["fields"] for r in rows], np.int16), scoring=np.array([r[5] for r in rows], np.int32),
        ops_off=ops_off, ops=np.array([v for r in rows for v in r[4]["ops"]], np.uint32), meta=np.array(json.dumps(meta)))


if __name__ == "__main__":
    if "--worker" in sys.argv:
        rest = sys.argv[sys.argv.index("--worker") + 1:]
        worker(parse_scoring(rest[0]) if rest else SCORING)
    elif "--scoring" in sys.argv:
        main_scorings(sys.argv[sys.argv.index("--scoring") + 1:])
    else:
        main()
