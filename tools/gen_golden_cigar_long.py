#!/usr/bin/env python3
"""Record the reference's CIGARs of long alignments as golden vectors: tests/golden/sw_cigar_long.npz (reads of up to
2 048 bp on templates of up to 4 095 columns, the range of tredlong_sw_cigar) and tests/golden/alignments_synlong600.json.

BUILD-CONTAINER ONLY (CPU), as tools/gen_golden_cigar.py is, whose helpers it imports: every alignment is the reference's
own -- src/ssw.c compiled into oracle/_ref/libssw.so, driven through the reference's ssw_wrap.Aligner (tools/refshim.py) in
child processes that report item by item.  Nothing of the reference is stored, only these inputs and outputs.

    python tools/gen_golden_cigar_long.py [OUTPUT DIRECTORY, default tests/golden]

Items (class, scoring):
  La  the winning (read, template) pair of every `details` read of synlong600 (run_long.json) at HD, DM1, ULD and SCA10,
      1/5/7/2; the sample is regenerated from its seed.  The winner is the pair gen_golden_cigar.main picks: every template
      of the ladder is aligned, the highest score among those that give a tag wins, then the fewest units, then db order;
      tag and units are asserted against the golden's.
  Lb  synthetic reads of 481, 512, 600, 1 000, 1 024, 1 025 and 2 048 bp on ladders of period 3/4/5/6/12, both strands,
      1 % substitutions and N, the whole template or a cut of the longest one; and reads of 300 bp on such a ladder
  Lc  the whole-template reads against a template one or two units off: a single I or D, band > 1 from the start
  Ld  compensating indels of 3, 6 and 20 bases on plain references of 600-1 200 bp (the band doubles 2, 3 and 5 times)
  Le  one gap of 70, 100, 130 and 200 bases at 2/2/3/1 and 8/16/16/1 in reads of 1 000-2 000 bp
  Lf  the extremes: 481 x 512, 2 048 x 2 048 at band 1, 2 048 bp on 4 095 columns with six 2-base indels, and at 8/16/16/1
      a(1024) + b(1024) against a + x(2047) + b: the 2 048 x 4 095 rectangle in one band
Lb-Ld alternate between 1/5/7/2 and 2/2/3/1.  An item is kept only if the reference returned and its operations consume
exactly the aligned bases; no item of La may be left out, at most 2 % of the others, and every class keeps at least 8.
"""
import hashlib
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_cigar import mutate, parse_scoring, randseq, template          # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
DEFAULT, CHEAP, DEAR = "1/5/7/2", "2/2/3/1", "8/16/16/1"
FLANK = 9
LOCI = ("HD", "DM1", "ULD", "SCA10")
REPORT_LOCI = ("HD", "SCA10")


# ---- the child: the reference, item by item, with its CPU seconds ---------------------------------------------------------
def worker(scoring):
    import refshim
    ref = refshim.load_reference()
    res_cls = ref.ssw.PyAlignRes
    raw_op = res_cls.cigar_int_to_op
    res_cls.cigar_int_to_op = staticmethod(lambda v: raw_op(v).decode())     # c_char is bytes under Python 3
    for line in sys.stdin:
        ref_seq, read = json.loads(line)
        t0 = time.process_time()
        al = ref.ssw.Aligner(ref_seq=ref_seq, report_secondary=False, **scoring).align(read)
        out = {"fields": [al.score, al.ref_begin, al.ref_end, al.query_begin, al.query_end],
               "ops": [int(v) & 0xFFFFFFFF for v in al._cigar_string], "cigar_string": al.cigar_string,
               "alignment": list(al.alignment), "str": str(al), "cpu_s": time.process_time() - t0}
        sys.stdout.write(json.dumps(out) + "\n")
        sys.stdout.flush()


def run_reference(pairs, tag, chunk=100):
    """[result dict or None (the reference faulted)] for every (ref_seq, read) at scoring `tag`."""
    out = [None] * len(pairs)
    k = 0
    while k < len(pairs):
        part = pairs[k:k + chunk]
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tag],
                           input="".join(json.dumps(x) + "\n" for x in part), stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL, universal_newlines=True)
        lines = [l for l in p.stdout.split("\n") if l.endswith("}")]
        for i, l in enumerate(lines):
            out[k + i] = json.loads(l)
        k += len(lines) + (0 if len(lines) == len(part) else 1)       # the item the child died on is skipped
    return out


# ---- the items --------------------------------------------------------------------------------------------------------------
def build(rng):
    ladders, items = [], []          # items: (class, ladder, template, read, scoring)

    def ladder_id(l):
        ladders.append(tuple(l))
        return len(ladders) - 1

    def plain(cls, ref, read, scoring):
        items.append((cls, ladder_id((ref, "A", "", 0)), 0, read, scoring))

    motifs = {3: "CAG", 4: "CCTG", 5: "ATTCT", 6: "GGCCTG", 12: "CCCCGCCCCGCG"}
    periods = sorted(motifs)
    flip = 0
    for n, T in enumerate((481, 512, 600, 1000, 1024, 1025, 2048)):                 # b, c
        for k in range(2):
            period = periods[(2 * n + k) % len(periods)]
            u = (T - 60) // period
            lad = ladder_id((randseq(rng, 30), motifs[period], randseq(rng, T - 30 - u * period), u + 3))
            strand = (n + k) % 2
            scoring = (DEFAULT, CHEAP)[flip % 2]
            flip += 1
            whole = mutate(rng, template(ladders[lad], 2 * (u - 1) + strand))
            assert len(whole) == T
            items.append(("Lb", lad, 2 * (u - 1) + strand, whole, scoring))
            for off in rng.sample([-2, -1, 1, 2], 2):
                items.append(("Lc", lad, 2 * (u + off - 1) + strand, whole, scoring))
            src = template(ladders[lad], 2 * (u + 3 - 1) + (1 - strand))               # a cut of the longest template
            at = rng.choice([0, len(src) - T, rng.randint(0, len(src) - T)])
            items.append(("Lb", lad, 2 * (u + 3 - 1) + (1 - strand), mutate(rng, src[at:at + T]), scoring))
            if T in (600, 1000, 2048) and k == 0:                                      # a short read on a long ladder
                at = rng.randint(0, len(src) - 300)
                items.append(("Lb", lad, 2 * (u + 3 - 1) + (1 - strand), mutate(rng, src[at:at + 300]), scoring))
    for k, (n, g) in enumerate((n, g) for n in (600, 800, 1000, 1200) for g in (3, 6, 20)):      # d
        ref = randseq(rng, n + 20)
        body = ref[10:10 + n]
        p1 = rng.randint(150, n // 2 - 60)
        p2 = rng.randint(n // 2 + 60, n - 150)
        if k % 2:
            read = body[:p1] + body[p1 + g:p2] + randseq(rng, g) + body[p2:]
        else:
            read = body[:p1] + randseq(rng, g) + body[p1:p2] + body[p2 + g:]
        plain("Ld", ref, read, (DEFAULT, CHEAP)[k % 2] if g < 20 else (DEFAULT, CHEAP)[(k // 3) % 2])
    for k, (g, scoring) in enumerate((g, s) for g in (70, 100, 130, 200) for s in (CHEAP, DEAR, DEAR if g < 130 else CHEAP)):   # e
        n = rng.choice([1000, 1400, 1800, 2000 - g])
        ref = randseq(rng, n + g + 20)
        p = rng.randint(n // 3, 2 * n // 3)
        if k % 2:                                                  # a deletion: the read skips g reference bases
            read = ref[10:10 + p] + ref[10 + p + g:10 + n + g]
        else:                                                      # an insertion of g bases
            read = ref[10:10 + p] + randseq(rng, g) + ref[10 + p:10 + n - g]
        plain("Le", ref, read if scoring == DEAR else mutate(rng, read, sub=0.003, n=0.001), scoring)
    # f: the extremes
    ref = randseq(rng, 512)
    plain("Lf", ref, mutate(rng, ref[20:501]), DEFAULT)                                # 481 x 512
    ref = randseq(rng, 2048)
    plain("Lf", ref, mutate(rng, ref), DEFAULT)                                        # 2 048 x 2 048, band 1
    ref = randseq(rng, 2100)
    plain("Lf", ref, ref[30:2078], CHEAP)                                              # 2048M
    ref = randseq(rng, 4095)
    read, at = "", 1000
    for k in range(6):                                                                # six 2-base indels
        seg = 340
        read += ref[at:at + seg]
        at += seg
        if k % 2:
            at += 2
        else:
            read += randseq(rng, 2)
    plain("Lf", ref, (read + ref[at:at + 2048])[:2048], CHEAP)
    a, b, x = randseq(rng, 1024), randseq(rng, 1024), randseq(rng, 2047)
    plain("Lf", a + x + b, a + b, DEAR)                                               # 2 048 x 4 095 in one band
    a, b = randseq(rng, 800), randseq(rng, 895)
    plain("Lf", a + b, a + randseq(rng, 353) + b, DEAR)                               # 800M353I895M
    lad = ladder_id((randseq(rng, 20), "CAG", randseq(rng, 20), 683))                  # 1 260 bp on (CAG)683
    src = template(ladders[lad], 2 * 682)
    items.append(("Lf", lad, 2 * 682, mutate(rng, src[400:1660]), DEFAULT))
    ref = randseq(rng, 4095)
    plain("Lf", ref, mutate(rng, ref[3600:4081]), DEFAULT)                             # 481 bp at the end of 4 095 columns
    ref = randseq(rng, 2050)
    plain("Lf", ref, ref[1:1000] + ref[1001:2050], CHEAP)                              # 2 048 bp with one base deleted
    return ladders, items


def consumes(r):
    if r is None or len(r["ops"]) == 0:
        return False
    q = sum(v >> 4 for v in r["ops"] if v & 15 in (0, 1))
    rr = sum(v >> 4 for v in r["ops"] if v & 15 in (0, 2))
    f = r["fields"]
    return q == f[4] - f[3] + 1 and rr == f[2] - f[1] + 1


def tag_of(r, seq, target, units, period, mu):
    """_parseReadSW's tag of one alignment (bam_parser.py:123-174), None without one."""
    sc, rb, re_, qb, qe = r["fields"]
    min_len = min(len(seq), len(target)) // 2
    if not (sc >= max(min_len, 30) and qe - qb + 1 >= min_len):
        return None
    hang = min(len(target) - re_ - 1 + qb, rb + len(seq) - qe - 1, rb + len(target) - re_ - 1, qb + len(seq) - qe - 1)
    pre, suf = rb < FLANK, re_ > len(target) - FLANK - 1
    return "HANG" if hang >= FLANK else ("FULL" if suf else "PREF") if pre else "POST" if suf else \
        "REPT" if units >= mu - 1 and units * period <= len(seq) else None


def real_items(ladders):
    """La: [(ladder, template, read, result, locus, detail)] in `details` order, and the report golden."""
    import math
    import tempfile
    from gen_golden import LONG_SAMPLES
    from tredparse_amd import synth, synth_bam, tred as tredmod
    from tredparse_amd.meta import TREDsRepo
    with open(os.path.join(GOLD, "run_long.json")) as fp:
        gold = json.load(fp)["samples"]["synlong600"]
    seed, names, kw, alt_rate = LONG_SAMPLES["synlong600"]
    loci = [l for l in synth.load_loci() if l["name"] in names]
    recs, _ = synth_bam.simulate_sample(seed, loci, synth.SynthParams(**kw), alt_rate=alt_rate)
    tmp = tempfile.mkdtemp()
    bam = os.path.join(tmp, "synlong600.bam")
    synth_bam.write_bam(bam, recs, sample="synlong600", level=1)
    repo = TREDsRepo(ref="hg38", sites=os.path.join(GOLD, "no_sites"))
    scan = tredmod.collect_sample(("synlong600", bam, repo, gold["loci"], 300, False, False, True, True, "INFO"), long_reads=True)
    by_name = {l["name"]: l for l in loci}
    out = []
    for k, name in enumerate(scan.names):
        if name not in LOCI:
            continue
        x = by_name[name]
        mu = int(math.ceil(float(scan.readlen) / len(x["repeat"])))                    # bam_parser.py: the ladder of the read length
        lad = len(ladders)
        ladders.append((x["prefix"], x["repeat"], x["suffix"], mu))
        a, b = scan.reads_of(k)
        pool = [(scan.name(i), scan.sequence(i)) for i in range(a, b)]                 # the locus' reads, BAM order
        details = gold["tredCalls"][name + ".details"]
        # every template of the ladder for every read that bears a `details` name, the winner as gen_golden_cigar.main
        # picks it: the highest score among the templates that give a tag, then the fewest units, then db order
        wanted = {d[0] for d in details}
        cand = [pi for pi, (nm, _) in enumerate(pool) if nm in wanted]
        pairs = [(template(ladders[lad], t), pool[pi][1]) for pi in cand for t in range(2 * mu)]
        res = run_reference(pairs, DEFAULT, chunk=400)
        assert all(r is not None for r in res), "the reference faulted on a real read"
        winner = {}
        for n, pi in enumerate(cand):
            for t in range(2 * mu):
                r, (target, seq) = res[n * 2 * mu + t], pairs[n * 2 * mu + t]
                tag = tag_of(r, seq, target, t // 2 + 1, len(x["repeat"]), mu)
                if tag is None:
                    continue
                key = (r["fields"][0], -(t // 2 + 1))
                if pi not in winner or key > winner[pi][0]:
                    winner[pi] = (key, t, r, tag)
        at = 0
        for rid, tag, h in details:                    # `details` is in BAM order: the next read of that name and result
            pi = next(pi for pi in cand if pi >= at and pool[pi][0] == rid and pi in winner and
                      (winner[pi][3], -winner[pi][0][1]) == (tag, int(h)))
            at = pi + 1
            _, t, r, _ = winner[pi]
            out.append((lad, t, pool[pi][1], r, name, {"id": rid, "tag": tag, "h": int(h)}))
    return out


def main(out_dir=GOLD):
    rng = random.Random(20261019)
    ladders, items = build(rng)
    done = []
    t_ref = 0.0
    real = real_items(ladders)
    for lad, t, seq, r, name, d in real:
        done.append(("La", lad, t, seq, DEFAULT, r))
    for tag in (DEFAULT, CHEAP, DEAR):
        sub = [it for it in items if it[4] == tag]
        res = run_reference([(template(ladders[lad], t), read) for _, lad, t, read, _ in sub], tag)
        done += [(c, lad, t, read, s, r) for (c, lad, t, read, s), r in zip(sub, res)]
    order = {c: i for i, c in enumerate(("La", "Lb", "Lc", "Ld", "Le", "Lf"))}
    done.sort(key=lambda k: order[k[0]])
    kept, total, excluded = [], {}, {}
    for it in done:
        total[it[0]] = total.get(it[0], 0) + 1
        if consumes(it[5]):
            kept.append(it)
        else:
            excluded[it[0]] = excluded.get(it[0], 0) + 1
    n_kept = {c: sum(1 for k in kept if k[0] == c) for c in total}
    others = sum(v for c, v in total.items() if c != "La")
    assert excluded.get("La", 0) == 0, excluded
    assert sum(v for c, v in excluded.items() if c != "La") <= 0.02 * others, (excluded, total)
    assert all(n_kept.get(c, 0) >= 8 for c in order), n_kept
    assert len(kept) >= 60
    used = sorted({k[1] for k in kept})
    renum = {l: i for i, l in enumerate(used)}
    cpu = [k[5]["cpu_s"] for k in kept]
    largest = max(range(len(kept)), key=lambda i: (kept[i][5]["fields"][2] - kept[i][5]["fields"][1] + 1) *
                  (kept[i][5]["fields"][4] - kept[i][5]["fields"][3] + 1))
    # the three texts of 8 items: the shortest with a gap of every class but La, and the shortest two of La
    text_of = []
    for c in order:
        ks = sorted((i for i, k in enumerate(kept) if k[0] == c and any(v & 15 for v in k[5]["ops"])),
                    key=lambda i: len(kept[i][3])) or sorted((i for i, k in enumerate(kept) if k[0] == c), key=lambda i: len(kept[i][3]))
        text_of += ks[:2 if c in ("La", "Lb") else 1]
    text_of = sorted(text_of)[:8]
    assert len(text_of) == 8
    meta = {"generator": "tools/gen_golden_cigar_long.py: the reference's ssw_wrap.Aligner (src/ssw.c compiled, via tools/refshim.py)",
            "ladders": [list(ladders[l]) for l in used], "total": total, "kept": n_kept, "excluded": excluded,
            "with_gap": sum(1 for k in kept if any(v & 15 for v in k[5]["ops"])),
            "more_than_3_ops": sum(1 for k in kept if len(k[5]["ops"]) > 3),
            "reference_cpu_seconds": round(sum(cpu), 3),
            "reference_cpu_seconds_by_scoring": {t: round(sum(c for c, k in zip(cpu, kept) if k[4] == t), 3) for t in (DEFAULT, CHEAP, DEAR)},
            "largest_item": largest, "largest_item_cpu_seconds": round(cpu[largest], 3),
            "texts": {str(i): {"cigar_string": kept[i][5]["cigar_string"], "alignment": kept[i][5]["alignment"], "str": kept[i][5]["str"]}
                      for i in text_of}}
    print(json.dumps({k: v for k, v in meta.items() if k not in ("ladders", "texts")}, indent=1))
    ops_off = np.zeros(len(kept) + 1, np.int64)
    ops_off[1:] = np.cumsum([len(k[5]["ops"]) for k in kept])
    path = os.path.join(out_dir, "sw_cigar_long.npz")
    np.savez_compressed(
        path, cls=np.array([k[0] for k in kept]), ladder=np.array([renum[k[1]] for k in kept], np.int32),
        template=np.array([k[2] for k in kept], np.int32), reads=np.array([k[3] for k in kept]),
        fields=np.array([k[5]["fields"] for k in kept], np.int16),
        scoring=np.array([[parse_scoring(k[4])[f] for f in ("match", "mismatch", "gap_open", "gap_extend")] for k in kept], np.int32),
        ops_off=ops_off, ops=np.array([v for k in kept for v in k[5]["ops"]], np.uint32), meta=np.array(json.dumps(meta)))
    assert os.path.getsize(path) < 150 * 1024, os.path.getsize(path)
    print(os.path.getsize(path), "bytes")
    # the --alignments report of synlong600: per `details` read of two loci what the report says, the block as a digest
    report = {}
    for lad, t, seq, r, name, d in real:
        if name not in REPORT_LOCI:
            continue
        target = template(ladders[lad], t)
        block = "\n".join(["{} {}".format(t // 2 + 1, target), r["str"].strip()] + r["alignment"]) + "\n"      # gen_golden_cigar.main
        report.setdefault(name, []).append({"id": d["id"], "tag": d["tag"], "h": d["h"], "strand": "-" if t % 2 else "+",
                                            "fields": r["fields"], "cigar_string": r["cigar_string"],
                                            "block_sha256": hashlib.sha256(block.encode()).hexdigest()})
    with open(os.path.join(out_dir, "alignments_synlong600.json"), "w") as fp:
        json.dump({"generator": "tools/gen_golden_cigar_long.py: per `details` read of synlong600 (run_long.json) the reference's "
                                "alignment with the template it was counted for; block_sha256: the verbose block of the "
                                "--alignments report (units and template, str(), the three alignment lines)",
                   "loci": report}, fp, indent=0)


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker(parse_scoring(sys.argv[sys.argv.index("--worker") + 1]))
    else:
        main(*sys.argv[1:2])
