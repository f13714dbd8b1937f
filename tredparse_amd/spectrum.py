"""What Engine.spectrum reports of one locus: the repeat-unit words its reads show (Context.unit_spectrum,
include/tredpileup.h), per class of reads.  Position-free, so the in-repeat reads count, which no consensus can place.
Plain numpy, no GPU: the tables are the kernel's, the reading of them is here."""
import numpy as np

from ._lib import SPECTRUM_BINS, SPECTRUM_MAX_PERIOD, SPECTRUM_STRIDE

LETTERS = "ACGT"


def word_code(word):
    """The bin of a word of A C G T (sum letter_i * 4^(p - 1 - i)); None for any other letter."""
    code = 0
    for ch in word.upper():
        if ch not in LETTERS:
            return None
        code = code * 4 + LETTERS.index(ch)
    return code


def code_word(code, period):
    return "".join(LETTERS[(code >> (2 * (period - 1 - i))) & 3] for i in range(period))


class ClassSpectrum(object):
    """One class of reads (`full:a`, `partial`, `rept`) of a locus:

      reads              the reads of the class (accepted items)
      units              their clean units without an N: p read letters on the columns of one tract unit, all inside one
                         M operation
      with_n             clean units whose word holds an N (in no bin)
      touched            the units the reads' alignments reach, clean or not
      purity             units that are the motif / units; None at 0 units
      words              {word: count} of the non-zero bins, by falling count, then by word
      interrupted_reads  reads with a clean unit that is not the motif
    """
    __slots__ = ("reads", "units", "with_n", "touched", "purity", "words", "interrupted_reads")

    def __init__(self, motif, row, items):
        """row: int32 [SPECTRUM_STRIDE] of the group; items: int32 [m][3], out_item of its accepted items."""
        row = np.asarray(row, np.int64)
        assert row.shape == (SPECTRUM_STRIDE,)
        period = len(motif)
        clean, self.with_n, self.touched, self.reads = (int(v) for v in row[SPECTRUM_BINS:])
        self.units = clean - self.with_n
        code = word_code(motif)
        self.purity = None if self.units == 0 else (int(row[code]) if code is not None else 0) / self.units
        hit = np.nonzero(row[:SPECTRUM_BINS])[0]
        pairs = sorted(((int(row[c]), code_word(int(c), period)) for c in hit), key=lambda x: (-x[0], x[1]))
        self.words = {w: n for n, w in pairs}
        items = np.asarray(items, np.int64).reshape(-1, 3)
        self.interrupted_reads = int((items[:, 0] > items[:, 1]).sum())

    def to_dict(self):
        return {k: getattr(self, k) for k in sorted(self.__slots__)}


class RepeatSpectrum(object):
    """The spectrum of a locus: motif, period and classes {name: ClassSpectrum} -- `full:a` per allele asked for (reads
    tagged FULL with h == a), `partial` (all PREF and POST reads), `rept` (all REPT reads).  A period above
    SPECTRUM_MAX_PERIOD has no table: unsupported is True and there are no classes."""
    __slots__ = ("motif", "period", "classes", "unsupported")

    def __init__(self, motif, tables=None):
        """tables: {class name: (row, items)} as ClassSpectrum takes them; None for a period without a table."""
        self.motif, self.period = motif, len(motif)
        self.unsupported = self.period > SPECTRUM_MAX_PERIOD
        assert self.unsupported == (tables is None)
        self.classes = {} if tables is None else {name: ClassSpectrum(motif, row, items) for name, (row, items) in tables.items()}

    def to_dict(self):
        """What tred.py --spectrum writes of the locus."""
        if self.unsupported:
            return {"motif": self.motif, "period": self.period, "unsupported": True}
        return {"motif": self.motif, "period": self.period,
                "classes": {name: self.classes[name].to_dict() for name in sorted(self.classes)}}
