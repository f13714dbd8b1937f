"""Plain-Python restatement of tredpileup_pileup (include/tredpileup.h) and of the consensus rules Engine.consensus
reads from its table: the CPU yardstick of tredparse_amd/csrc/pileup.hip and tredparse_amd/consensus.py.

    add_item        one alignment (template length, strand, read, fields, operations) into a table of the FORWARD template
    status_of       the refusals an item can be given on its own
    pileup          a whole call: groups, the shape a group takes from its first accepted item, the table and the statuses
    consensus_of    per-column consensus, depth, interruptions and insertions of one table
    from_lines      the INDEPENDENT derivation: the same table from the three text lines of an alignment (reference letters,
                    match marks, read letters), its `Reference begin`, strand and target -- it never sees a CIGAR
"""
import numpy as np

from .cigar_model import template

OK, TOO_LONG, BAD_ITEM = 0, 4, 5
CH = 8
LETTERS = "ACGTN-"
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
MAX_READ, MAX_TEMPLATE = 2048, 4095


def channel(letter):
    return CODE.get(letter.upper(), 4)


def table(L):
    return [[0] * CH for _ in range(L + 1)]


def add_item(counts, L, strand, read, fields, ops):
    """The item into counts ([L + 1][8]): strand 1 is a reverse-complement template, whose column c is forward column
    L - 1 - c, whose letters are complemented and whose insertion before c sits before L - c."""
    r, q = int(fields[1]), int(fields[3])
    for v in ops:
        n, op = int(v) >> 4, int(v) & 15
        if op == 1:
            slot = L - r if strand else r
            counts[slot][6] += 1
            counts[slot][7] += n
            q += n
            continue
        for k in range(n):
            c, ch = r + k, 5
            if op == 0:
                ch = channel(read[q + k])
                if strand and ch < 4:
                    ch = 3 - ch
            counts[L - 1 - c if strand else c][ch] += 1
        r += n
        if op == 0:
            q += n


def template_len(ladder, t):
    prefix, repeat, suffix, mu = ladder
    return len(prefix) + len(repeat) * (t // 2 + 1) + len(suffix) if mu > 0 else len(prefix)


def status_of(ladders, n_groups, cap, read_len, lad, tpl, fields, ops, n_ops, group):
    """ops: the item's row of `cap` entries (or fewer: missing entries are 0), n_ops its count."""
    if not 0 <= group < n_groups or not 0 <= lad < len(ladders):
        return BAD_ITEM
    mu = ladders[lad][3]
    if not 0 <= tpl < (2 * mu if mu > 0 else 1):
        return BAD_ITEM
    T = template_len(ladders[lad], tpl)
    if read_len > MAX_READ or T > MAX_TEMPLATE:
        return TOO_LONG
    _, rb, re_, qb, qe = (int(v) for v in fields[:5])
    if rb < 0 or re_ < rb or re_ >= T or qb < 0 or qe < qb or qe >= read_len:
        return BAD_ITEM
    if n_ops < 1 or n_ops > cap:
        return BAD_ITEM
    row = [int(v) for v in ops[:n_ops]] + [0] * (n_ops - len(ops))
    if any(v & 15 > 2 or v >> 4 == 0 for v in row):
        return BAD_ITEM
    if sum(v >> 4 for v in row if v & 15 != 1) != re_ - rb + 1 or sum(v >> 4 for v in row if v & 15 != 2) != qe - qb + 1:
        return BAD_ITEM
    return OK


def pileup(ladders, reads, item_ladder, item_template, fields, ops, n_ops, item_group, n_groups, stride, cap, read_len=None):
    """(counts int32 [n_groups][stride][8], status int32 [n]) of a call.  ops: one list per item."""
    n = len(reads)
    counts = np.zeros((n_groups, stride, CH), np.int32)
    status = np.zeros(n, np.int32)
    shape, tables = {}, {}
    for k in range(n):
        L = len(reads[k]) if read_len is None else int(read_len[k])
        lad, tpl, g = int(item_ladder[k]), int(item_template[k]), int(item_group[k])
        status[k] = status_of(ladders, n_groups, cap, L, lad, tpl, fields[k], ops[k], int(n_ops[k]), g)
        if status[k] != OK:
            continue
        if g not in shape:
            shape[g] = (lad, tpl // 2)
            tables[g] = table(template_len(ladders[lad], tpl))
        if shape[g] != (lad, tpl // 2):
            status[k] = BAD_ITEM
            continue
        strand = tpl % 2 if ladders[lad][3] > 0 else 0
        add_item(tables[g], template_len(ladders[lad], tpl), strand, reads[k], fields[k], ops[k][:int(n_ops[k])])
    for g, t in tables.items():
        counts[g, :len(t)] = t
    return counts, status


def revcomp(s):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(c, "N") for c in reversed(s))


def from_lines(counts, L, strand, ref_begin, r_line, q_line):
    """The same table from the text of an alignment: reference letter over read letter is a base, letter over blank a
    deletion, blank over letter an insertion (a run of them is one event).  The lines are those of the item's own strand."""
    assert len(r_line) == len(q_line)
    c, run = int(ref_begin), 0
    for a, b in zip(r_line, q_line):
        if a == " ":
            assert b != " "
            slot = L - c if strand else c
            counts[slot][6] += 0 if run else 1
            counts[slot][7] += 1
            run += 1
            continue
        run = 0
        ch = 5
        if b != " ":
            ch = channel(b)
            if strand and ch < 4:
                ch = 3 - ch
        counts[L - 1 - c if strand else c][ch] += 1
        c += 1


def consensus_of(counts, T, prefix_len, period, a):
    """counts [len(T) + 1][8] of the forward template T = prefix + repeat * a + suffix -> dict(consensus, depth,
    interruptions, insertions) by the rules of Engine.consensus."""
    cons, depth, inter, ins = [], [], [], []
    for c, ref in enumerate(T):
        row = [int(v) for v in counts[c][:6]]
        d = sum(row)
        depth.append(d)
        if d == 0:
            cons.append(ref.lower())
            continue
        top = max(row)
        tied = [ch for ch in range(6) if row[ch] == top]
        ch = channel(ref) if channel(ref) in tied else tied[0]
        cons.append(LETTERS[ch])
        if prefix_len <= c < prefix_len + a * period and d >= 2 and ch != channel(ref) and 2 * row[ch] > d:
            inter.append({"unit": (c - prefix_len) // period + 1, "offset": (c - prefix_len) % period, "ref": ref,
                          "alt": LETTERS[ch], "support": row[ch], "depth": d})
    for c in range(len(T) + 1):
        if counts[c][6] > 0:
            ins.append({"before": c, "reads": int(counts[c][6]), "bases": int(counts[c][7])})
    return {"consensus": "".join(cons), "depth": depth, "interruptions": inter, "insertions": ins}


def parse_blocks(text):
    """The blocks of an --alignments report: dicts with locus, tag, h, strand (0 / 1), read id, target, ref_begin, the
    five fields, cigar_string and the three alignment lines."""
    out = []
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        if not lines[i].startswith(">"):
            i += 1
            continue
        locus, tag, h, strand, rid = lines[i][1:].split(" ", 4)
        units, target = lines[i + 1].split(" ")
        assert lines[i + 2] == "OPTIMAL MATCH"
        vals = {}
        j = i + 3
        while not lines[j].startswith("Cigar_string"):
            key, v = lines[j].rsplit(None, 1)
            vals[key] = int(v)
            j += 1
        out.append(dict(locus=locus, tag=tag, h=int(h[2:]), strand=int(strand == "-"), id=rid, target=target,
                        units=int(units), cigar_string=lines[j].split()[1], lines=lines[j + 1:j + 4],
                        fields=[vals["Score"], vals["Reference begin"], vals["Reference end"], vals["Query begin"],
                                vals["Query end"]]))
        i = j + 4
    return out


def cigar_ops(cigar_string):
    """The M / I / D operations of a CIGAR text (soft clips left out) as length << 4 | op."""
    import re
    return [int(n) << 4 | "MID".index(op) for n, op in re.findall(r"(\d+)([MIDS])", cigar_string) if op != "S"]
