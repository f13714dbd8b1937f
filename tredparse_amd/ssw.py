"""`ssw.Aligner` with the reference's signature (src/ssw_wrap.py:110-143, 177-227) on top of the GPU kernel: one
alignment = one read against a plain reference registered as a max_units = 0 ladder.

For tests, spot checks and code that still thinks one (reference, read) pair at a time -- the product path batches
whole template ladders (bam_parser / engine) and never comes through here.  All Aligners of a process share ONE
private GPU context (created on first use, never the engine's: registering a one-template ladder replaces a
context's ladder table), the reference is re-registered only when it differs from the one registered last, and
`align_many` takes any number of reads per call.

The reference computes two things on every call that are opt-in here, one kernel launch each per `align_many` and only
for the queries that pass the min_score / min_len filter: `report_cigar=True` fills the CIGAR (include/tredcigar.h) and
`report_secondary=True` fills `score2` / `ref_end2` (include/tredsecond.h) -- the best score that ends at least
len(query) // 2 columns (15 for queries of up to 30 letters) away from the optimal end, as ssw_align's struct has it; the
reference's own wrapper leaves `score2 = None` whatever the flag says (ssw_wrap.py:304).  On a tandem repeat
`score - score2` says how firmly the read is placed.
"""
import numpy as np

from . import _lib

_shared = {"ctx": None, "registered": None}


def _context():
    if _shared["ctx"] is None:
        _shared["ctx"] = _lib.Context(0)
    return _shared["ctx"]


def set_long_reads(enabled):
    """Switch the long-read path (Context.set_long_reads) of the shared private context: on, Aligners without a context of
    their own take references of up to 4 095 letters and queries of up to 2 048 bp, report_cigar and report_secondary
    included."""
    ctx = _context()
    if not enabled and ctx.long_reads:
        ctx.set_ladders([("N", "A", "", 0)])       # (a registered long reference would refuse the switch)
        _shared["registered"] = None
    ctx.set_long_reads(enabled)


class PyAlignRes(object):
    """The reference's result object (ssw_wrap.py:259-383): the five fields, score2 / ref_end2 (`second`; None without
    report_secondary), and -- from the operations `ops` (length << 4 | op, M=0 I=1 D=2; empty without report_cigar) -- its
    cigar_string / cigar, iter_cigar, alignment and str() texts."""

    def __init__(self, rec, query_seq, ref_seq, ops=(), second=None):
        self.score, self.ref_begin, self.ref_end, self.query_begin, self.query_end = (int(x) for x in rec[:5])
        self.score2, self.ref_end2 = (None, None) if second is None else (int(second[0]), int(second[1]))
        self.ref_seq, self.query_seq = ref_seq, query_seq
        self._cigar_string = [int(v) for v in ops]

    def __str__(self):                                                    # ssw_wrap.py:284-300
        msg = "OPTIMAL MATCH\n"
        msg += "Score            {}\n".format(self.score)
        msg += "Reference begin  {}\n".format(self.ref_begin)
        msg += "Reference end    {}\n".format(self.ref_end)
        msg += "Query begin      {}\n".format(self.query_begin)
        msg += "Query end        {}\n".format(self.query_end)
        if self.cigar_string:
            msg += "Cigar_string     {}\n".format(self.cigar_string)
        if self.score2:
            msg += "SUB-OPTIMAL MATCH\n"
            msg += "Score 2           {}\n".format(self.score2)
            msg += "Ref_end2          {}\n".format(self.ref_end2)
        return msg

    @property
    def iter_cigar(self):                                                 # cigar_int_to_len / _to_op, ssw.c:878-904
        for val in self._cigar_string:
            yield (val >> 4, "MIDNSHP=X"[val & 15] if val & 15 < 9 else "M")

    @property
    def cigar_string(self):                                               # ssw_wrap.py:320-345
        if len(self._cigar_string) == 0:
            return ""
        out = "{}S".format(self.query_begin) if self.query_begin > 0 else ""
        out += "".join("{}{}".format(n, op) for n, op in self.iter_cigar)
        end_len = len(self.query_seq) - self.query_end - 1
        if end_len != 0:
            out += "{}S".format(end_len)
        return out
    cigar = cigar_string

    @property
    def alignment(self):                                                  # ssw_wrap.py:348-383
        r, q = self.ref_begin if self.ref_begin > 0 else 0, self.query_begin if self.query_begin > 0 else 0
        r_line = m_line = q_line = ""
        for n, op in self.iter_cigar:
            if op == "M":
                rs, qs = self.ref_seq[r:r + n], self.query_seq[q:q + n]
                r_line += rs
                q_line += qs
                m_line += "".join("|" if a == b else "*" for a, b in zip(rs, qs))
                r, q = r + n, q + n
            elif op == "I":
                r_line += " " * n
                m_line += " " * n
                q_line += self.query_seq[q:q + n]
                q += n
            elif op == "D":
                r_line += self.ref_seq[r:r + n]
                m_line += " " * n
                q_line += " " * n
                r += n
        return (r_line, m_line, q_line)


class Aligner(object):
    def __init__(self, ref_seq="", match=2, mismatch=2, gap_open=3, gap_extend=1, report_secondary=False,
                 report_cigar=False, ctx=None):
        self.ref_seq = ref_seq
        self.match, self.mismatch, self.gap_open, self.gap_extend = match, mismatch, gap_open, gap_extend
        self.report_cigar = bool(report_cigar)   # the reference computes the CIGAR on every call; here it is opt-in
        self.report_secondary = bool(report_secondary)   # score2 / ref_end2: opt-in as well
        self._own = ctx            # a caller-supplied context is used as is (and its ladders replaced)

    def _ready(self):
        ctx = self._own or _context()
        key = (id(ctx), self.ref_seq)
        if self._own is not None or _shared["registered"] != key:
            ctx.set_ladders([(self.ref_seq, "A", "", 0)])
            if self._own is None:
                _shared["registered"] = key
        return ctx

    def align_many(self, queries, min_score=0, min_len=0):
        """[PyAlignRes or None] for every query, one kernel launch."""
        queries = list(queries)
        n = len(queries)
        if n == 0:
            return []
        ctx = self._ready()
        packed, woff, rlen = _lib.pack_reads(queries)
        tag, h, sc = np.zeros(n, np.uint8), np.zeros(n, np.int16), np.zeros(n, np.int16)
        dump = np.zeros((n, 1, 6), np.int16)
        p = _lib.SwParams(self.match, self.mismatch, self.gap_open, self.gap_extend, 9, 0, 0, 0)
        ctx.sw_classify(_lib.MEM_HOST, packed, woff, rlen, n, np.array([0, n], np.int32), np.zeros(1, np.int32), 1, p,
                        tag, h, sc, dump, 1)
        recs = dump[:, 0]
        keep = [int(rec[0]) >= min_score and int(rec[4]) - int(rec[3]) + 1 >= min_len for rec in recs]    # ssw_wrap.py:214-220
        ops = [()] * n
        if self.report_cigar and any(keep):
            ops = self._cigars(ctx, queries, recs, [k for k in range(n) if keep[k]], p, ops)
        second = [None] * n
        if self.report_secondary and any(keep):
            second = self._seconds(ctx, queries, recs, [k for k in range(n) if keep[k]], p, second)
        return [PyAlignRes(rec, q, self.ref_seq, o, s2) if k else None
                for q, rec, k, o, s2 in zip(queries, recs, keep, ops, second)]

    def _seconds(self, ctx, queries, recs, kept, p, second):
        """ONE sw_secondary call for the queries that passed the filter, maskLen as Aligner.align sets it (ssw_wrap.py:198-201)."""
        sub = [queries[k] for k in kept]
        m = len(sub)
        packed, woff, rlen = _lib.pack_reads(sub)
        zero = np.zeros(m, np.int32)
        mask = np.array([len(q) // 2 if len(q) > 30 else 15 for q in sub], np.int32)
        out, status = np.zeros((m, 4), np.int32), np.zeros(m, np.int32)
        ctx.sw_secondary(packed, woff, rlen, m, zero, zero, mask, p, out, status, ladders=[(self.ref_seq, "A", "", 0)])
        second = list(second)
        for i, k in enumerate(kept):
            if status[i] != _lib.SECOND_OK or (int(out[i, 0]), int(out[i, 1])) != (int(recs[k][0]), int(recs[k][2])):
                raise _lib.TredGpuError("sw_secondary: status {} for query {}, score1 / ref_end1 {} / {} against the SW "
                                        "kernel's {} / {}".format(int(status[i]), k, out[i, 0], out[i, 1], recs[k][0], recs[k][2]))
            second[k] = out[i, 2:]
        return second

    def _cigars(self, ctx, queries, recs, kept, p, ops):
        """ONE sw_cigar call for the queries that passed the filter; a CIGAR longer than the room gets a second call."""
        sub = [queries[k] for k in kept]
        m = len(sub)
        packed, woff, rlen = _lib.pack_reads(sub)
        fields = np.ascontiguousarray(recs[kept, :5], np.int16)
        zero = np.zeros(m, np.int32)
        cap = 32
        while True:
            out, n_ops, status = np.zeros((m, cap), np.uint32), np.zeros(m, np.int32), np.zeros(m, np.int32)
            ctx.sw_cigar(_lib.MEM_HOST, packed, woff, rlen, m, zero, zero, fields, p, cap, out, n_ops, status,
                         ladders=[(self.ref_seq, "A", "", 0)])
            if not (status == _lib.CIGAR_OVERFLOW).any():
                break
            cap = int(n_ops.max())
        ops = list(ops)
        for i, k in enumerate(kept):
            if status[i] != _lib.CIGAR_OK:
                raise _lib.TredGpuError("sw_cigar: status {} for query {} (the reference runs off its buffers there)".format(
                    int(status[i]), k))
            ops[k] = out[i, :n_ops[i]]
        return ops

    def align(self, query_seq, min_score=0, min_len=0):
        return self.align_many([query_seq], min_score, min_len)[0]
