"""What Engine.consensus reports of one allele: the pileup table of the reads that span it (Context.pileup,
include/tredpileup.h) -- with partial=True also of the reads anchored in one flank (Context.pileup_anchored) -- read
column by column.  Plain numpy, no GPU: the table is the kernel's, the rules are here."""
import numpy as np

LETTERS = "ACGTN-"           # the table's channels 0-5; 6: insertions before the column, 7: their summed length
_CODE = np.full(256, 4, np.int64)
for _k, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _k


class AlleleConsensus(object):
    """The evidence for allele h (repeat units) of a locus, on T = prefix + repeat * h + suffix:

      h, reads        the allele and the number of reads laid on it (FULL reads tagged with h)
      counts          int32 [len(T) + 1][8], the pileup table (slot len(T): insertions behind the last column)
      depth           per column, channels 0-5 summed
      consensus       one character per column: T[c] in lower case where depth is 0, otherwise the channel 0-5 with the
                      largest count as ACGTN- (on a tie T[c]'s channel if it is among the tied, else the lowest)
      interruptions   the tract columns with depth >= 2 whose consensus is not T[c] and holds more than half the depth:
                      {"unit" (1-based), "offset" (in the unit), "ref", "alt", "support", "depth"}
      insertions      {"before": column, "reads", "bases"} for every slot with an insertion
      partial         the PREF / POST reads laid on the allele from the side of their flank (Engine.consensus(partial=True);
                      0 otherwise).  Their columns are in counts with those of the FULL reads
      ambiguous, beyond   the PREF / POST reads of the unit laid nowhere: short enough to fit any allele asked for, and
                      longer than the longest.  Non-zero only on the unit's longest allele
    """
    __slots__ = ("h", "reads", "counts", "depth", "consensus", "interruptions", "insertions", "partial", "ambiguous", "beyond")

    def __init__(self, h, reads, counts, template, prefix_len, period, partial=0, ambiguous=0, beyond=0):
        T = len(template)
        self.h, self.reads = int(h), int(reads)
        self.partial, self.ambiguous, self.beyond = int(partial), int(ambiguous), int(beyond)
        self.counts = np.ascontiguousarray(counts[:T + 1], np.int32)
        six = self.counts[:T, :6].astype(np.int64)
        self.depth = six.sum(axis=1)
        ref = _CODE[np.frombuffer(template.encode("latin-1"), np.uint8)]
        top = six.max(axis=1) if T else np.zeros(0, np.int64)
        ch = six.argmax(axis=1) if T else np.zeros(0, np.int64)           # the lowest channel among the tied ...
        ref_tied = six[np.arange(T), ref] == top
        ch = np.where(ref_tied, ref, ch)                                  # ... unless the template's letter is one of them
        covered = self.depth > 0
        self.consensus = "".join(LETTERS[k] if ok else t.lower() for k, ok, t in zip(ch.tolist(), covered.tolist(), template))
        col = np.arange(T)
        hit = ((col >= prefix_len) & (col < prefix_len + self.h * period) & (self.depth >= 2) & (ch != ref) &
               (2 * six[col, ch] > self.depth))
        self.interruptions = [{"unit": (c - prefix_len) // period + 1, "offset": (c - prefix_len) % period, "ref": template[c],
                               "alt": LETTERS[ch[c]], "support": int(six[c, ch[c]]), "depth": int(self.depth[c])}
                              for c in np.nonzero(hit)[0].tolist()]
        self.insertions = [{"before": c, "reads": int(self.counts[c, 6]), "bases": int(self.counts[c, 7])}
                           for c in np.nonzero(self.counts[:, 6] > 0)[0].tolist()]

    def to_dict(self, partial=False):
        """What tred.py --consensus writes of the allele; partial: and what --consensus-partial adds."""
        d = {"h": self.h, "reads": self.reads, "consensus": self.consensus, "depth": [int(v) for v in self.depth],
             "interruptions": self.interruptions, "insertions": self.insertions}
        if partial:
            d.update(partial=self.partial, ambiguous=self.ambiguous, beyond=self.beyond)
        return d
