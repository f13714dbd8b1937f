"""ctypes binding of libtredgpu.so (include/tredgpu.h).

The library is the product path: there is no Python/CPU fallback.  Loading needs the in-tree
``tredparse_amd/libtredgpu.so`` (built by ``__graft_entry__.build()`` / ``make -C tredparse_amd/csrc``);
creating a context needs a HIP device and fails loudly otherwise.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TREDGPU_LIB") or os.path.join(HERE, "libtredgpu.so")   # override: kernel experiments

MEM_HOST, MEM_DEVICE = 0, 1
TAG_NONE, TAG_FULL, TAG_PREF, TAG_POST, TAG_REPT, TAG_HANG, TAG_INVALID = 0, 1, 2, 3, 4, 5, 255
MAX_READ_LEN, MAX_TEMPLATE_LEN = 480, 511                      # include/tredgpu.h
MAX_LONG_READ_LEN, MAX_LONG_TEMPLATE_LEN = 2048, 4095          # the long-read path (include/tredlong.h)
TAG_NAMES = {TAG_FULL: "FULL", TAG_PREF: "PREF", TAG_POST: "POST", TAG_REPT: "REPT", TAG_HANG: "HANG"}
SPAN = 1000


class TredGpuError(RuntimeError):
    pass


class SwParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32),
                ("gap_extend", C.c_int32), ("flank", C.c_int32), ("clip", C.c_int32),
                ("max_read_len", C.c_int32), ("reserved", C.c_int32)]


class UnitParams(C.Structure):
    _fields_ = [("period", C.c_int32), ("readlen", C.c_int32), ("ploidy", C.c_int32),
                ("maxinsert", C.c_int32), ("fullsearch", C.c_int32), ("ref_len", C.c_int32),
                ("minpe", C.c_int32), ("cutoff_risk", C.c_int32), ("is_expansion", C.c_int32),
                ("is_recessive", C.c_int32), ("pe_off", C.c_int32), ("n_global", C.c_int32),
                ("tl_off", C.c_int32), ("n_target", C.c_int32), ("half_depth", C.c_double)]


class Call(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_pairs", C.c_int32), ("h1", C.c_int32), ("h2", C.c_int32),
                ("ci", C.c_int32 * 4), ("run_pe", C.c_int32), ("pad", C.c_int32),
                ("lik", C.c_double), ("pp", C.c_double)]


class TrioParams(C.Structure):
    _fields_ = [("mu", C.c_double), ("rho", C.c_double), ("beta", C.c_double)]


class CohortParams(C.Structure):
    _fields_ = [("iters", C.c_int32), ("alpha", C.c_double)]


UNIT_DTYPE = np.dtype([("period", "<i4"), ("readlen", "<i4"), ("ploidy", "<i4"), ("maxinsert", "<i4"),
                       ("fullsearch", "<i4"), ("ref_len", "<i4"), ("minpe", "<i4"), ("cutoff_risk", "<i4"),
                       ("is_expansion", "<i4"), ("is_recessive", "<i4"), ("pe_off", "<i4"),
                       ("n_global", "<i4"), ("tl_off", "<i4"), ("n_target", "<i4"), ("half_depth", "<f8")])
CALL_DTYPE = np.dtype([("status", "<i4"), ("n_pairs", "<i4"), ("h1", "<i4"), ("h2", "<i4"),
                       ("ci", "<i4", (4,)), ("run_pe", "<i4"), ("pad", "<i4"), ("lik", "<f8"), ("pp", "<f8")])
assert UNIT_DTYPE.itemsize == C.sizeof(UnitParams) == 64
assert CALL_DTYPE.itemsize == C.sizeof(Call) == 56

# the long-read path's symbols (include/tredlong.h)
LONG_EXPORTS = ("tredlong_sw_classify", "tredlong_last_error", "tredlong_sw_cigar", "tredlong_cigar_timing",
                "tredlong_cigar_reset_timing", "tredlong_release")
LONG_CIGAR_SLOTS = 256          # wavefronts of a tredlong_sw_cigar launch at the most (csrc/cigar_long_plan.h)

# the CIGAR kernel's symbols (include/tredcigar.h)
CIGAR_EXPORTS = ("tredcigar_sw_cigar", "tredcigar_get_timing", "tredcigar_reset_timing", "tredcigar_release",
                 "tredcigar_last_error")
CIGAR_OK, CIGAR_NO_PATH, CIGAR_OFF_EDGE, CIGAR_OVERFLOW, CIGAR_TOO_LONG, CIGAR_BAD_ITEM = 0, 1, 2, 3, 4, 5

# the second-best alignment's symbols (include/tredsecond.h)
SECOND_EXPORTS = ("tredsecond_sw_second", "tredsecond_get_timing", "tredsecond_reset_timing", "tredsecond_release",
                  "tredsecond_last_error")
SECOND_OK, SECOND_TOO_LONG, SECOND_BAD_ITEM = 0, 4, 5

# the pileup's symbols (include/tredpileup.h)
PILEUP_EXPORTS = ("tredpileup_pileup", "tredpileup_pileup_anchored", "tredpileup_unit_spectrum", "tredpileup_get_timing",
                  "tredpileup_reset_timing", "tredpileup_release", "tredpileup_last_error")
PILEUP_OK, PILEUP_TOO_LONG, PILEUP_BAD_ITEM = 0, 4, 5
PILEUP_ANCHOR_WHOLE, PILEUP_ANCHOR_BEGIN, PILEUP_ANCHOR_END = 0, 1, 2   # item_anchor of pileup_anchored: FULL, PREF, POST
PILEUP_CHANNELS = 8             # A C G T N, deleted, insertions before the column, their summed length
PILEUP_PERIOD = 6               # out_status of unit_spectrum: a period above SPECTRUM_MAX_PERIOD has no table
SPECTRUM_MAX_PERIOD = 6
SPECTRUM_BINS = 4096            # 4^6 words, code = sum letter_i * 4^(p - 1 - i), A 0 C 1 G 2 T 3
SPECTRUM_STRIDE = 4100          # the bins, then clean units, with_n, touched units, accepted items

# the trio evaluation's symbols (include/tredtrio.h)
TRIO_EXPORTS = ("tredtrio_evaluate", "tredtrio_get_timing", "tredtrio_reset_timing", "tredtrio_release", "tredtrio_last_error")
TRIO_OK, TRIO_EMPTY_CHILD, TRIO_DEGENERATE, TRIO_TOO_LONG, TRIO_BAD_ITEM = 0, 1, 2, 4, 5
TRIO_STATUS_NAMES = {TRIO_OK: "OK", TRIO_EMPTY_CHILD: "EMPTY_CHILD", TRIO_DEGENERATE: "DEGENERATE", TRIO_TOO_LONG: "TOO_LONG",
                     TRIO_BAD_ITEM: "BAD_ITEM"}
TRIO_MAX_ALLELE = 1024          # TREDGPU_TRIO_MAX_ALLELE: the largest allele of any pair list, in repeat units
TRIO_PAIR_CHUNK = 1024          # TREDGPU_TRIO_PAIR_CHUNK: pairs of a parent's list staged in LDS at a time
TRIO_GAMETE_TILE = 64           # TREDGPU_TRIO_GAMETE_TILE: distinct child alleles of one gamete workgroup
TRIO_MU, TRIO_RHO, TRIO_BETA = 0.01, 0.9, 0.5      # the defaults of the transmission model: a choice, not a measurement

# the cohort frequencies' symbols (include/tredcohort.h)
COHORT_EXPORTS = ("tredcohort_evaluate", "tredcohort_get_timing", "tredcohort_reset_timing", "tredcohort_release",
                  "tredcohort_last_error")
COHORT_OK, COHORT_EMPTY, COHORT_TOO_LONG, COHORT_BAD_ITEM = 0, 1, 4, 5
COHORT_STATUS_NAMES = {COHORT_OK: "OK", COHORT_EMPTY: "EMPTY", COHORT_TOO_LONG: "TOO_LONG", COHORT_BAD_ITEM: "BAD_ITEM"}
COHORT_MAX_ALLELE = 1024        # TREDGPU_COHORT_MAX_ALLELE: the largest allele of any pair list, in repeat units
COHORT_MAX_ITERS = 4096         # TREDGPU_COHORT_MAX_ITERS
COHORT_CHUNK = 1024             # TREDGPU_COHORT_CHUNK: incidence entries of an allele one wavefront sums in the M-step
COHORT_LONG_LIST = 1024         # TREDGPU_COHORT_LONG_LIST: a sample of more pairs has a workgroup to itself, any other a wavefront
COHORT_ITERS, COHORT_ALPHA, COHORT_TOL = 64, 1.0, 1e-6     # EM iterations, pseudo-chromosomes, what `converged` reports: a choice

# the tandem-repeat scan's symbols (include/tredscan.h)
SCAN_EXPORTS = ("tredscan_scan", "tredscan_get_timing", "tredscan_reset_timing", "tredscan_release", "tredscan_last_error")
SCAN_MAX_PERIOD = 6             # TREDSCAN_MAX_PERIOD
SCAN_TILE = 4096                # TREDSCAN_TILE: the letters one wavefront owns
SCAN_MAX_LETTERS = 1 << 30      # TREDSCAN_MAX_LETTERS: the letters of all segments of one call
SCAN_MIN_COPIES = (10, 6, 5, 4, 4, 4)      # whole copies a run of period 1 .. 6 needs to be reported: a choice, not a measurement

# the interrupted-tract scan's symbols (include/tredtract.h)
TRACT_EXPORTS = ("tredtract_scan", "tredtract_get_timing", "tredtract_reset_timing", "tredtract_release", "tredtract_last_error")
TRACT_MAX_GAP = 64              # TREDTRACT_MAX_GAP: the most letters between two linked seeds
TRACT_SEED_COPIES = (5, 3, 3, 3, 3, 3)     # whole copies a perfect run of period 1 .. 6 needs to take part: a choice, not a measurement
TRACT_MAX_GAP_DEFAULT = (1, 2, 3, 4, 5, 6)  # letters between two seeds that are joined (one unit): a choice, not a measurement

# every symbol include/tredgpu.h declares (tests check the .so exports them all)
EXPORTS = ("tredgpu_create", "tredgpu_destroy", "tredgpu_last_error", "tredgpu_sync", "tredgpu_get_stream",
           "tredgpu_version", "tredgpu_set_ladders", "tredgpu_set_model", "tredgpu_pack_reads",
           "tredgpu_sw_classify", "tredgpu_tally", "tredgpu_likelihood_grid", "tredgpu_likelihood_grid_joint",
           "tredgpu_genotype_batch", "tredgpu_genotype_batch_joint", "tredgpu_genotype_selected",
           "tredgpu_pe_kde", "tredgpu_reset_timing", "tredgpu_get_timing", "tredgpu_get_sw_counters",
           "tredgpu_inflater_create", "tredgpu_inflater_destroy", "tredgpu_inflater_last_error",
           "tredgpu_inflater_reserve", "tredgpu_inflate_blocks", "tredgpu_inflate_blocks_crc", "tredgpu_inflater_timing",
           "tredgpu_inflate_walk", "tredgpu_inflater_fetch", "tredgpu_inflater_walk_ms", "tredgpu_inflater_host_out",
           "tredgpu_inflater_fetch_dense", "tredgpu_inflater_pinned_bytes", "tredgpu_inflater_walk_serial_regions")

KERNEL_SW, KERNEL_TALLY, KERNEL_GRID = 0, 1, 2
KERNEL_GRID_PREPARE, KERNEL_GRID_PAIRS, KERNEL_GRID_REDUCE, KERNEL_GRID_KDE = 3, 4, 5, 6
KERNEL_CIGAR = 16               # include/tredcigar.h; tredgpu_get_timing's own series ends at 6
KERNEL_CIGAR_LONG = 17          # tredlong_cigar_timing (include/tredlong.h): a selector of the binding's only
KERNEL_SECOND = 18              # tredsecond_get_timing (include/tredsecond.h): calls of sw_secondary and their device time
KERNEL_PILEUP = 19              # tredpileup_get_timing (include/tredpileup.h): calls of pileup and their device time
KERNEL_TRIO = 20                # tredtrio_get_timing (include/tredtrio.h): calls of trio and their device time
KERNEL_COHORT = 21              # tredcohort_get_timing (include/tredcohort.h): calls of cohort and their device time
KERNEL_SCAN = 22                # tredscan_get_timing (include/tredscan.h): calls of scan and their device time
KERNEL_TRACT = 23               # tredtract_get_timing (include/tredtract.h): calls of scan_tracts and their device time


# the timed opt-in units: (prefix, get-timing, reset-timing, KERNEL_* selector, last_error), in the order reset_timing has
# always gone through them.  Context.close releases them (PREFIX_release) in this order too, tredlong first where it used
# to be last: a release returns nothing and touches its own unit's state alone (tredlong_release also frees what
# tredlong_sw_classify holds)
SIDE_UNITS = (("tredlong", "tredlong_cigar_timing", "tredlong_cigar_reset_timing", KERNEL_CIGAR_LONG, "tredlong_last_error"),
              ("tredcigar", "tredcigar_get_timing", "tredcigar_reset_timing", KERNEL_CIGAR, "tredcigar_last_error"),
              ("tredsecond", "tredsecond_get_timing", "tredsecond_reset_timing", KERNEL_SECOND, "tredsecond_last_error"),
              ("tredpileup", "tredpileup_get_timing", "tredpileup_reset_timing", KERNEL_PILEUP, "tredpileup_last_error"),
              ("tredtrio", "tredtrio_get_timing", "tredtrio_reset_timing", KERNEL_TRIO, "tredtrio_last_error"),
              ("tredcohort", "tredcohort_get_timing", "tredcohort_reset_timing", KERNEL_COHORT, "tredcohort_last_error"),
              ("tredscan", "tredscan_get_timing", "tredscan_reset_timing", KERNEL_SCAN, "tredscan_last_error"),
              ("tredtract", "tredtract_get_timing", "tredtract_reset_timing", KERNEL_TRACT, "tredtract_last_error"))

_lib = None


def load():
    """dlopen the in-tree library and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TredGpuError("{} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)".format(LIB_PATH))
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.tredgpu_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.tredgpu_destroy.argtypes = [vp]
    lib.tredgpu_destroy.restype = None
    lib.tredgpu_last_error.argtypes = [vp]
    lib.tredgpu_last_error.restype = C.c_char_p
    lib.tredgpu_sync.argtypes = [vp]
    lib.tredlong_sw_classify.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                             C.POINTER(C.c_char_p), vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, C.c_int32]
    lib.tredlong_sw_cigar.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                      vp, vp, vp, vp, i64, vp, vp, vp, C.POINTER(SwParams), i32, vp, vp, vp]
    lib.tredcigar_sw_cigar.argtypes = [vp, C.c_int, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                       vp, vp, vp, vp, i64, vp, vp, vp, C.POINTER(SwParams), i32, vp, vp, vp]
    lib.tredsecond_sw_second.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                         vp, vp, vp, vp, i64, vp, vp, vp, C.POINTER(SwParams), vp, vp]
    lib.tredpileup_pileup.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                      vp, vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp]
    lib.tredpileup_pileup_anchored.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                               vp, vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]
    lib.tredpileup_unit_spectrum.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                             vp, vp, vp, vp, i64, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]
    lib.tredtrio_evaluate.argtypes = [vp, C.POINTER(TrioParams), i64] + [vp] * 19
    lib.tredcohort_evaluate.argtypes = [vp, C.POINTER(CohortParams), i64] + [vp] * 16
    lib.tredscan_scan.argtypes = [vp, vp, vp, i32, vp, i64, vp, vp, vp, vp, C.POINTER(i64)]
    lib.tredtract_scan.argtypes = [vp, vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]
    for prefix, get_timing, reset_timing, _, last_error in SIDE_UNITS:
        getattr(lib, get_timing).argtypes = [vp, C.POINTER(i64), C.POINTER(C.c_double)]
        getattr(lib, reset_timing).argtypes = [vp]
        getattr(lib, prefix + "_release").argtypes = [vp]
        getattr(lib, prefix + "_release").restype = None
        getattr(lib, last_error).argtypes = []
        getattr(lib, last_error).restype = C.c_char_p
    lib.tredgpu_get_stream.argtypes = [vp]
    lib.tredgpu_get_stream.restype = vp
    lib.tredgpu_version.restype = C.c_char_p
    lib.tredgpu_set_ladders.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                        C.POINTER(C.c_char_p), vp]
    lib.tredgpu_set_model.argtypes = [vp, vp, vp, C.c_double, C.c_double]
    lib.tredgpu_pack_reads.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.tredgpu_pack_reads.restype = i64
    lib.tredgpu_sw_classify.argtypes = [vp, C.c_int, vp, vp, vp, i64, vp, vp, i32, C.POINTER(SwParams),
                                        vp, vp, vp, vp, i32]
    lib.tredgpu_tally.argtypes = [vp, C.c_int, vp, vp, i64, vp, i32, vp, i32, vp, vp, vp]
    lib.tredgpu_likelihood_grid.argtypes = [vp, C.c_int, vp, i32, i32, vp, vp, vp, vp, i64, vp, i64, vp,
                                            vp, vp, vp, i32]
    lib.tredgpu_likelihood_grid_joint.argtypes = [vp, C.c_int, vp, i32, i32, vp, vp, vp, vp, i64, vp, i64, vp,
                                                  vp, i32, vp, vp, vp, vp]
    lib.tredgpu_genotype_batch.argtypes = [vp, C.c_int, vp, vp, vp, i64, vp, vp, vp, i32,
                                           C.POINTER(SwParams), vp, vp, i64, vp, i64, vp, vp, vp, i32,
                                           vp, vp, vp, vp]
    lib.tredgpu_genotype_batch_joint.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, i32, C.POINTER(SwParams), vp, vp, i64, vp, i64,
                                                 vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.tredgpu_genotype_selected.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(SwParams), vp, i64, vp, i64,
                                              vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.tredgpu_pe_kde.argtypes = [vp, C.c_int, vp, i32, vp, i64, vp, vp]
    lib.tredgpu_reset_timing.argtypes = [vp]
    lib.tredgpu_get_timing.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(C.c_double)]
    lib.tredgpu_get_sw_counters.argtypes = [vp, vp]
    lib.tredgpu_inflater_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.tredgpu_inflater_destroy.argtypes = [vp]
    lib.tredgpu_inflater_destroy.restype = None
    lib.tredgpu_inflater_last_error.argtypes = [vp]
    lib.tredgpu_inflater_last_error.restype = C.c_char_p
    lib.tredgpu_inflater_reserve.argtypes = [vp, i64, i64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.tredgpu_inflate_blocks.argtypes = [vp, i32, vp]
    lib.tredgpu_inflate_blocks_crc.argtypes = [vp, i32, vp, vp]
    lib.tredgpu_inflater_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.tredgpu_inflate_walk.argtypes = [vp, i32, vp, vp, C.POINTER(WalkArgs)]
    lib.tredgpu_inflater_fetch.argtypes = [vp, i32, vp]
    lib.tredgpu_inflater_walk_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.tredgpu_inflater_host_out.argtypes = [vp, C.c_int]
    lib.tredgpu_inflater_pinned_bytes.argtypes = [vp]
    lib.tredgpu_inflater_pinned_bytes.restype = i64
    lib.tredgpu_inflater_walk_serial_regions.argtypes = [vp]
    lib.tredgpu_inflater_walk_serial_regions.restype = i64
    lib.tredgpu_inflater_fetch_dense.argtypes = [vp, i32, vp, C.POINTER(vp), vp]
    _lib = lib
    return lib


def _ptr(a):
    """Raw pointer of a numpy array, a torch tensor, an int address or None."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        if not a.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return a.data_ptr()
    raise TypeError("unsupported buffer type {}".format(type(a)))


def _ladder_args(ladders):
    """A list of (prefix, repeat, suffix, max_units) as the (n_ladders, prefix, repeat, suffix, max_units) arguments of
    tredgpu_set_ladders, tredlong_sw_classify and tredcigar_sw_cigar.  The ctypes arrays own what they point to: the
    caller holds the tuple until the call has returned."""
    n = len(ladders)
    arr = lambda k: (C.c_char_p * max(n, 1))(*[l[k].encode() for l in ladders])
    mu = np.ctypeslib.as_ctypes(np.asarray([l[3] for l in ladders] or [0], np.int32))
    return n, arr(0), arr(1), arr(2), mu


def pack_reads(seqs):
    """2-bit + N-mask packing (tredgpu_pack_reads).  seqs: list of str/bytes.
    Returns (packed uint32[], word_off int64[n+1], read_len int32[n])."""
    lib = load()
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    n = len(bs)
    off = np.zeros(n + 1, np.int64)
    if n:
        off[1:] = np.cumsum([len(b) for b in bs])
    blob = b"".join(bs)
    buf = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
    woff = np.zeros(n + 1, np.int64)
    rlen = np.zeros(max(n, 1), np.int32)
    total = lib.tredgpu_pack_reads(buf.ctypes.data, off.ctypes.data, n, None, woff.ctypes.data, rlen.ctypes.data)
    if total < 0:
        raise TredGpuError("tredgpu_pack_reads failed ({})".format(total))
    packed = np.zeros(max(int(total), 1), np.uint32)
    lib.tredgpu_pack_reads(buf.ctypes.data, off.ctypes.data, n, packed.ctypes.data, woff.ctypes.data, rlen.ctypes.data)
    return packed, woff, rlen[:n]


def pack_codes(codes, lengths=None):
    """Vectorised packer for a 2-D uint8 array of base codes (0..3, 4 = N), all reads the same
    length (rows) -- same record layout as tredgpu_pack_reads; used by the synthetic generator."""
    codes = np.ascontiguousarray(codes, np.uint8)
    n, L = codes.shape
    nb, nm = (L + 15) // 16, (L + 31) // 32
    isn = codes >= 4
    c = np.where(isn, 0, codes).astype(np.uint8)
    bits = np.zeros((n, nb * 32), np.uint8)          # bit 2k = low bit of base k, bit 2k+1 = high bit
    bits[:, 0:2 * L:2] = c & 1
    bits[:, 1:2 * L:2] = c >> 1
    words = np.packbits(bits, axis=1, bitorder="little").view("<u4")
    mbits = np.zeros((n, nm * 32), np.uint8)
    mbits[:, :L] = isn
    masks = np.packbits(mbits, axis=1, bitorder="little").view("<u4")
    packed = np.ascontiguousarray(np.concatenate([words, masks], axis=1).reshape(-1))
    woff = (np.arange(n + 1, dtype=np.int64) * (nb + nm))
    rlen = np.full(n, L, np.int32)
    return packed, woff, rlen


def version():
    """The library's version string incl. the hash of the kernel sources it was built from (csrc/Makefile)."""
    return load().tredgpu_version().decode()


class Context:
    """One GPU + one HIP stream (tredgpu_ctx)."""

    def __init__(self, device_id=0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.tredgpu_create(device_id, C.byref(h))
        if rc != 0:
            raise TredGpuError("tredgpu_create({}) failed: {}".format(
                device_id, self.lib.tredgpu_last_error(None).decode()))
        self.h = h
        self.n_ladders = 0
        self.ladders = None
        self.long_reads = False
        self._is_long = None   # the long-read path's mask over self.ladders (None while the path is off) -- see set_ladders

    def close(self):
        if getattr(self, "h", None):
            for unit in SIDE_UNITS:
                getattr(self.lib, unit[0] + "_release")(self.h)
            self.lib.tredgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise TredGpuError("{} failed ({}): {}".format(what, rc, self.lib.tredgpu_last_error(self.h).decode()))

    def sync(self):
        self._chk(self.lib.tredgpu_sync(self.h), "tredgpu_sync")

    @property
    def stream(self):
        return self.lib.tredgpu_get_stream(self.h)

    def set_ladders(self, ladders):
        """ladders: list of (prefix, repeat, suffix, max_units).  With the long-read path on (set_long_reads), a ladder
        whose longest template exceeds MAX_TEMPLATE_LEN (up to MAX_LONG_TEMPLATE_LEN) is registered with the library as a
        one-letter stand-in, and every read of it goes to the long kernel."""
        ladders = list(ladders)
        native, is_long = ladders, None
        if self.long_reads:
            for i, l in enumerate(ladders):
                T = self._template_len(l)
                if T > MAX_LONG_TEMPLATE_LEN:
                    raise TredGpuError("tredgpu_set_ladders failed: ladder {}: longest template {} exceeds "
                                       "TREDGPU_MAX_LONG_TEMPLATE_LEN={}".format(i, T, MAX_LONG_TEMPLATE_LEN))
            is_long = np.array([self._template_len(l) > MAX_TEMPLATE_LEN for l in ladders], bool)
            # the library's table: a plain one-letter reference stands in for a long ladder (none of its reads reaches it)
            native = [("N", "A", "", 0) if lg else l for l, lg in zip(ladders, is_long)]
        table = _ladder_args(native)
        self._chk(self.lib.tredgpu_set_ladders(self.h, *table), "tredgpu_set_ladders")
        self.n_ladders = len(native)
        self.ladders, self._is_long = ladders, is_long

    # ---- the long-read path (include/tredlong.h) -------------------------------------------------------------
    def set_long_reads(self, enabled):
        """Switch the long-read path on or off (off by default).  On: set_ladders accepts ladders up to
        MAX_LONG_TEMPLATE_LEN columns, and sw_classify, genotype_batch and genotype_batch_joint (host memory) accept reads
        up to MAX_LONG_READ_LEN bp.  A read longer than MAX_READ_LEN or on a ladder longer than MAX_TEMPLATE_LEN goes to
        tredlong_sw_classify; every other read goes to the library's calls exactly as with the path off.  sw_cigar routes
        its items the same way, to tredlong_sw_cigar.  Refused
        while a registered ladder is longer than MAX_TEMPLATE_LEN and the path is switched off."""
        enabled = bool(enabled)
        if not enabled and self._is_long is not None and self._is_long.any():
            raise TredGpuError("a registered ladder is longer than {} columns: register shorter ladders before switching "
                               "the long-read path off".format(MAX_TEMPLATE_LEN))
        was, self.long_reads = self.long_reads, enabled
        if enabled and not was and self.ladders is not None:
            self.set_ladders(self.ladders)
        if not enabled:
            self._is_long = None

    @staticmethod
    def _template_len(l):
        prefix, repeat, suffix, mu = l
        return len(prefix) + len(suffix) + len(repeat) * int(mu) if int(mu) > 0 else len(prefix)

    def _routed_call(self, mem, read_len, n_reads, unit_read_off, unit_ladder, n_units):
        """Reads of a call that take the long path (None: none, the call is the library's own)."""
        if self._is_long is None or n_reads == 0:
            return None
        if mem != MEM_HOST:
            if self._is_long.any():
                raise TredGpuError("the long-read path takes host-memory calls (MEM_HOST) only")
            return None
        rl = np.asarray(read_len)[:n_reads]
        uro = np.asarray(unit_read_off)[:n_units + 1].astype(np.int64)
        lad = np.repeat(np.asarray(unit_ladder)[:n_units], np.diff(uro))
        longest = int(rl.max())
        if longest > MAX_LONG_READ_LEN:
            raise TredGpuError("tredgpu_sw_classify failed: read of {} bp exceeds TREDGPU_MAX_LONG_READ_LEN={}".format(
                longest, MAX_LONG_READ_LEN))
        if lad.size and (lad.min() < 0 or lad.max() >= len(self._is_long)):
            return None                                   # (the library refuses the call with its own message)
        routed = (rl > MAX_READ_LEN) | (self._is_long[lad] if lad.size else False)
        return np.nonzero(routed)[0] if routed.any() else None

    def _classify_routed(self, routed, packed, read_off, read_len, unit_read_off, unit_ladder, n_units, params, out_tag,
                         out_h, out_score, out_dump=None, dump_templates=0, n_reads=None):
        """sw_classify with the routed reads hidden from the library's kernels (length 0) and aligned by the long
        kernel into the same output arrays."""
        rl = np.ascontiguousarray(np.asarray(read_len)[:n_reads], np.int32)
        masked = rl.copy()
        masked[routed] = 0
        p = SwParams(params.match, params.mismatch, params.gap_open, params.gap_extend, params.flank, params.clip,
                     min(int(params.max_read_len), MAX_READ_LEN), params.reserved)
        # (a call whose reads are all routed asks nothing of the library's kernels: their packed-value scoring bound,
        # check_sw_range, would refuse scorings the long kernel takes, such as gap_extend 16)
        if len(routed) < n_reads:
            self._chk(self.lib.tredgpu_sw_classify(self.h, MEM_HOST, _ptr(packed), _ptr(read_off), _ptr(masked), n_reads,
                                                   _ptr(unit_read_off), _ptr(unit_ladder), n_units, C.byref(p), _ptr(out_tag),
                                                   _ptr(out_h), _ptr(out_score), _ptr(out_dump), dump_templates),
                      "tredgpu_sw_classify")
        woff = np.asarray(read_off)
        pk = np.asarray(packed)
        sub_off = np.zeros(len(routed) + 1, np.int64)
        sub_off[1:] = np.cumsum(woff[routed + 1] - woff[routed])
        sub = np.ascontiguousarray(np.concatenate([pk[woff[r]:woff[r + 1]] for r in routed]), np.uint32)
        uro = np.asarray(unit_read_off)[:n_units + 1].astype(np.int64)
        lad = np.ascontiguousarray(np.repeat(np.asarray(unit_ladder)[:n_units], np.diff(uro))[routed], np.int32)
        table = _ladder_args(self.ladders)
        m = len(routed)
        tag, h, sc = np.zeros(m, np.uint8), np.zeros(m, np.int16), np.zeros(m, np.int16)
        dump = np.zeros((m, dump_templates, 6), np.int16) if out_dump is not None else None
        sub_len = np.ascontiguousarray(rl[routed])      # (held here: _ptr keeps no reference)
        rc = self.lib.tredlong_sw_classify(self.h, *table, _ptr(sub), _ptr(sub_off), _ptr(sub_len), m, _ptr(lad), C.byref(p),
                                           _ptr(tag), _ptr(h), _ptr(sc), _ptr(dump), dump_templates if dump is not None else 0)
        self._chk_side(rc, "tredlong_sw_classify failed ({})".format(rc), self.lib.tredlong_last_error)
        np.asarray(out_tag)[routed] = tag
        np.asarray(out_h)[routed] = h
        np.asarray(out_score)[routed] = sc
        if out_dump is not None:
            np.asarray(out_dump).reshape(-1, dump_templates, 6)[routed] = dump

    def set_model(self, step_pdf, stutter_w, gc=.68, score=1.0):
        step = np.ascontiguousarray(step_pdf, np.float64)
        w = np.ascontiguousarray(stutter_w, np.float64)
        assert step.shape == (6, 37) and w.shape == (5,)
        self._chk(self.lib.tredgpu_set_model(self.h, step.ctypes.data, w.ctypes.data, gc, score),
                  "tredgpu_set_model")

    def sw_classify(self, mem, packed, read_off, read_len, n_reads, unit_read_off, unit_ladder, n_units,
                    params, out_tag, out_h, out_score, out_dump=None, dump_templates=0):
        routed = self._routed_call(mem, read_len, n_reads, unit_read_off, unit_ladder, n_units)
        if routed is not None:
            return self._classify_routed(routed, packed, read_off, read_len, unit_read_off, unit_ladder, n_units, params,
                                         out_tag, out_h, out_score, out_dump, dump_templates, n_reads=n_reads)
        self._chk(self.lib.tredgpu_sw_classify(self.h, mem, _ptr(packed), _ptr(read_off), _ptr(read_len),
                                               n_reads, _ptr(unit_read_off), _ptr(unit_ladder), n_units,
                                               C.byref(params), _ptr(out_tag), _ptr(out_h), _ptr(out_score),
                                               _ptr(out_dump), dump_templates), "tredgpu_sw_classify")

    def tally(self, mem, tag, h, n_reads, unit_read_off, n_units, read_pair_id, hist_stride, full_cnt,
              pref_cnt, rept_cnt):
        self._chk(self.lib.tredgpu_tally(self.h, mem, _ptr(tag), _ptr(h), n_reads, _ptr(unit_read_off),
                                         n_units, _ptr(read_pair_id), hist_stride, _ptr(full_cnt),
                                         _ptr(pref_cnt), _ptr(rept_cnt)), "tredgpu_tally")

    def likelihood_grid(self, mem, units, n_units, hist_stride, full_cnt, pref_cnt, rept_cnt, global_lens,
                        n_global_total, target_lens, n_target_total, calls, grid_off=None, grid_dump=None,
                        marg=None, marg_stride=0):
        self._chk(self.lib.tredgpu_likelihood_grid(self.h, mem, _ptr(units), n_units, hist_stride,
                                                   _ptr(full_cnt), _ptr(pref_cnt), _ptr(rept_cnt),
                                                   _ptr(global_lens), n_global_total, _ptr(target_lens),
                                                   n_target_total, _ptr(calls), _ptr(grid_off),
                                                   _ptr(grid_dump), _ptr(marg), marg_stride),
                  "tredgpu_likelihood_grid")

    def likelihood_grid_joint(self, mem, units, n_units, hist_stride, full_cnt, pref_cnt, rept_cnt, global_lens,
                              n_global_total, target_lens, n_target_total, calls, marg, marg_stride, joint_off, joint,
                              joint_n, joint_total):
        self._chk(self.lib.tredgpu_likelihood_grid_joint(self.h, mem, _ptr(units), n_units, hist_stride,
                                                         _ptr(full_cnt), _ptr(pref_cnt), _ptr(rept_cnt),
                                                         _ptr(global_lens), n_global_total, _ptr(target_lens),
                                                         n_target_total, _ptr(calls), _ptr(marg), marg_stride,
                                                         _ptr(joint_off), _ptr(joint), _ptr(joint_n), _ptr(joint_total)),
                  "tredgpu_likelihood_grid_joint")

    def genotype_batch(self, mem, packed, read_off, read_len, n_reads, unit_read_off, unit_ladder, units,
                       n_units, params, read_pair_id, global_lens, n_global_total, target_lens,
                       n_target_total, out_tag, out_h, out_score, hist_stride, full_cnt, pref_cnt, rept_cnt,
                       calls):
        routed = self._routed_call(mem, read_len, n_reads, unit_read_off, unit_ladder, n_units)
        if routed is not None:
            return self._genotype_routed(routed, True, self.likelihood_grid, (), packed, read_off, read_len, n_reads,
                                         unit_read_off, unit_ladder, units, n_units, params, read_pair_id, global_lens,
                                         n_global_total, target_lens, n_target_total, out_tag, out_h, out_score, hist_stride,
                                         full_cnt, pref_cnt, rept_cnt, calls)
        self._chk(self.lib.tredgpu_genotype_batch(self.h, mem, _ptr(packed), _ptr(read_off), _ptr(read_len),
                                                  n_reads, _ptr(unit_read_off), _ptr(unit_ladder), _ptr(units),
                                                  n_units, C.byref(params), _ptr(read_pair_id),
                                                  _ptr(global_lens), n_global_total, _ptr(target_lens),
                                                  n_target_total, _ptr(out_tag), _ptr(out_h), _ptr(out_score),
                                                  hist_stride, _ptr(full_cnt), _ptr(pref_cnt), _ptr(rept_cnt),
                                                  _ptr(calls)), "tredgpu_genotype_batch")

    def genotype_batch_joint(self, packed, read_off, read_len, n_reads, unit_read_off, unit_ladder, units, n_units, params,
                             read_pair_id, global_lens, n_global_total, target_lens, n_target_total, out_tag, out_h, out_score,
                             hist_stride, rept_cnt, calls, marg, marg_stride, joint_off, joint, joint_n, joint_total):
        """tredgpu_genotype_batch_joint: SW + tagging -> histograms -> grid with marginals and sparse joint, host arrays,
        one wait."""
        routed = self._routed_call(MEM_HOST, read_len, n_reads, unit_read_off, unit_ladder, n_units)
        if routed is not None:
            return self._genotype_routed(routed, False, self.likelihood_grid_joint,
                                         (marg, marg_stride, joint_off, joint, joint_n, joint_total), packed, read_off, read_len,
                                         n_reads, unit_read_off, unit_ladder, units, n_units, params, read_pair_id, global_lens,
                                         n_global_total, target_lens, n_target_total, out_tag, out_h, out_score, hist_stride,
                                         None, None, rept_cnt, calls)
        self._chk(self.lib.tredgpu_genotype_batch_joint(self.h, _ptr(packed), _ptr(read_off), _ptr(read_len), n_reads,
                                                        _ptr(unit_read_off), _ptr(unit_ladder), _ptr(units), n_units,
                                                        C.byref(params), _ptr(read_pair_id), _ptr(global_lens), n_global_total,
                                                        _ptr(target_lens), n_target_total, _ptr(out_tag), _ptr(out_h),
                                                        _ptr(out_score), hist_stride, _ptr(rept_cnt), _ptr(calls), _ptr(marg),
                                                        marg_stride, _ptr(joint_off), _ptr(joint), _ptr(joint_n),
                                                        _ptr(joint_total)), "tredgpu_genotype_batch_joint")

    def _genotype_routed(self, routed, every_ladder, grid, grid_tail, packed, read_off, read_len, n_reads, unit_read_off,
                         unit_ladder, units, n_units, params, read_pair_id, global_lens, n_global_total, target_lens,
                         n_target_total, out_tag, out_h, out_score, hist_stride, full_cnt, pref_cnt, rept_cnt, calls):
        """genotype_batch / genotype_batch_joint with routed reads: SW (the long path included) -> tally -> grid as host-memory
        calls, the composition the library makes of them.  grid: likelihood_grid or likelihood_grid_joint, grid_tail its
        arguments after `calls`; full_cnt / pref_cnt None: histograms of the call's own.  The library only knows the
        stand-ins of long ladders, so hist_stride is checked here against the ladders in full: every_ladder, against every
        registered one (tredgpu_genotype_batch checks c->max_ladder_units), else against the batch's own (the fused call
        checks it per unit)."""
        ids = range(len(self.ladders)) if every_ladder else np.asarray(unit_ladder)[:n_units]
        for i in sorted(set(int(k) for k in ids)):
            mu = int(self.ladders[i][3])
            if hist_stride <= mu:
                raise TredGpuError("hist_stride {} must exceed the max_units {} of ladder {}".format(hist_stride, mu, i))
        self._classify_routed(routed, packed, read_off, read_len, unit_read_off, unit_ladder, n_units, params, out_tag,
                              out_h, out_score, n_reads=n_reads)
        if full_cnt is None:
            full_cnt, pref_cnt = np.zeros(n_units * hist_stride, np.int32), np.zeros(n_units * hist_stride, np.int32)
        self.tally(MEM_HOST, out_tag, out_h, n_reads, unit_read_off, n_units, read_pair_id, hist_stride, full_cnt, pref_cnt,
                   rept_cnt)
        return grid(MEM_HOST, units, n_units, hist_stride, full_cnt, pref_cnt, rept_cnt, global_lens, n_global_total,
                    target_lens, n_target_total, calls, *grid_tail)

    def genotype_selected(self, segs, unit_read_off, unit_word_off, unit_seq4_off, unit_name_off, unit_ladder, units, n_units, params,
                          global_lens, n_global_total, target_lens, n_target_total, out_tag, out_h, out_score, hist_stride, rept_cnt,
                          calls, marg, marg_stride, joint_off, joint, joint_n, joint_total, read_len, seq4_off, seq4, name_off, names):
        """tredgpu_genotype_selected: genotype_batch_joint over reads the inflaters' selections left on the device.
        segs: [(Inflater, int32 array of its tasks in batch order)]."""
        arr = (SelectedUnits * max(len(segs), 1))()
        keep = []
        for k, (inf, task) in enumerate(segs):
            task = np.ascontiguousarray(task, np.int32)
            keep.append(task)
            arr[k] = SelectedUnits(inf._h, len(task), 0, task.ctypes.data if len(task) else None)
        self._chk(self.lib.tredgpu_genotype_selected(self.h, arr, len(segs), _ptr(unit_read_off), _ptr(unit_word_off), _ptr(unit_seq4_off),
                                                     _ptr(unit_name_off), _ptr(unit_ladder), _ptr(units), n_units, C.byref(params),
                                                     _ptr(global_lens), n_global_total, _ptr(target_lens), n_target_total, _ptr(out_tag),
                                                     _ptr(out_h), _ptr(out_score), hist_stride, _ptr(rept_cnt), _ptr(calls), _ptr(marg),
                                                     marg_stride, _ptr(joint_off), _ptr(joint), _ptr(joint_n), _ptr(joint_total),
                                                     _ptr(read_len), _ptr(seq4_off), _ptr(seq4), _ptr(name_off), _ptr(names)),
                  "tredgpu_genotype_selected")

    def sw_cigar(self, mem, packed, read_off, read_len, n_items, item_ladder, item_template, fields, params, cap, out_ops,
                 out_n_ops, out_status, ladders=None):
        """tredcigar_sw_cigar (include/tredcigar.h): the reference's CIGAR of n_items alignments.  Item k is read k
        (packed / read_off / read_len as pack_reads writes them) against template item_template[k] (db order) of ladder
        item_ladder[k], placed by fields[k] = {score, ref_begin, ref_end, read_begin, read_end} (int16 [n][5]: a row of
        sw_classify's dump).  out_ops: uint32 [n][cap] (length << 4 | op, M=0 I=1 D=2), out_n_ops / out_status: int32 [n]
        (CIGAR_*).  ladders: the table the indices refer to (default: the one registered with set_ladders).
        With the long-read path on (set_long_reads), an item whose read is longer than MAX_READ_LEN or whose ladder's
        longest template is beyond MAX_TEMPLATE_LEN goes to tredlong_sw_cigar (include/tredlong.h; host memory only), all
        of them in one call, and the rest to tredcigar_sw_cigar in one call, exactly as with the path off."""
        ladders = list(self.ladders if ladders is None else ladders)
        if self.long_reads and n_items > 0:
            long_lad = np.array([self._template_len(l) > MAX_TEMPLATE_LEN for l in ladders], bool)
            if mem != MEM_HOST:
                if long_lad.any():
                    raise TredGpuError("the long-read path takes host-memory calls (MEM_HOST) only")
                if int(self._device_max(read_len, n_items)) > MAX_READ_LEN:
                    raise TredGpuError("the long-read path takes host-memory calls (MEM_HOST) only: a read of the call is "
                                       "longer than {} bp".format(MAX_READ_LEN))
            else:
                rl = np.asarray(read_len)[:n_items]
                lad = np.asarray(item_ladder)[:n_items]
                known = (lad >= 0) & (lad < len(ladders))
                routed = rl > MAX_READ_LEN
                routed[known] |= long_lad[lad[known]]
                if routed.any():
                    return self._cigar_routed(np.nonzero(routed)[0], ladders, packed, read_off, rl, n_items, lad, item_template,
                                              fields, params, cap, out_ops, out_n_ops, out_status)
        self._cigar_call(False, mem, ladders, packed, read_off, read_len, n_items, item_ladder, item_template, fields, params,
                         cap, out_ops, out_n_ops, out_status)

    def _cigar_call(self, long_call, mem, ladders, packed, read_off, read_len, n_items, item_ladder, item_template, fields,
                    params, cap, out_ops, out_n_ops, out_status):
        """One call of tredlong_sw_cigar (long_call; host memory only, so it has no mem argument) or tredcigar_sw_cigar."""
        unit = "tredlong" if long_call else "tredcigar"
        self._items_call(unit + "_sw_cigar", unit + "_last_error", ladders, packed, read_off, read_len, n_items, item_ladder,
                         item_template, _ptr(fields), C.byref(params), cap, _ptr(out_ops), _ptr(out_n_ops), _ptr(out_status),
                         mem=None if long_call else mem)

    def _items_call(self, entry, last_error, ladders, packed, read_off, read_len, n_items, item_ladder, item_template, *tail,
                    mem=None):
        """One call of a side unit's item-list entry (include/tredcigar.h, tredlong.h, tredsecond.h, tredpileup.h): the
        context, mem where the entry takes one (tredcigar_sw_cigar), the ladder table (ladders; None: the one registered
        with set_ladders), the items -- packed, read_off, read_len, n_items, item_ladder, item_template --, then tail, the
        entry's own arguments as the library takes them.  A refusal raises with the unit's own last_error."""
        table = _ladder_args(list(self.ladders if ladders is None else ladders))
        rc = getattr(self.lib, entry)(self.h, *(() if mem is None else (mem,)), *table, _ptr(packed), _ptr(read_off),
                                      _ptr(read_len), n_items, _ptr(item_ladder), _ptr(item_template), *tail)
        self._chk_side(rc, "{} failed ({})".format(entry, rc), getattr(self.lib, last_error))

    @staticmethod
    def _chk_side(rc, what, last_error):
        """Raises a side unit's error with the text of its own last_error (tredlong_* / tredcigar_*), not the context's."""
        if rc != 0:
            raise TredGpuError("{}: {}".format(what, last_error().decode()))

    @staticmethod
    def _device_max(read_len, n):
        """The largest of the first n read lengths of a device-memory call (a torch tensor or a raw address)."""
        if hasattr(read_len, "data_ptr"):
            return read_len[:n].max().item()
        return 0                      # (a raw address: the library's own refusal of the item, TOO_LONG, stands)

    def _cigar_routed(self, routed, ladders, packed, read_off, rl, n, lad, item_template, fields, params, cap, out_ops,
                      out_n_ops, out_status):
        """sw_cigar with the routed items through tredlong_sw_cigar and the others through tredcigar_sw_cigar, one call
        each, merged into the caller's arrays in the caller's order (the pattern of _classify_routed)."""
        woff = np.asarray(read_off).astype(np.int64)
        pk = np.asarray(packed)
        tpl = np.asarray(item_template)[:n]
        fl = np.asarray(fields).reshape(-1, 5)[:n]
        ops = np.asarray(out_ops).reshape(-1, cap) if cap > 0 else np.zeros((n, 0), np.uint32)
        mask = np.zeros(n, bool)
        mask[routed] = True
        for sel, long_call in ((np.nonzero(~mask)[0], False), (routed, True)):
            m = len(sel)
            if m == 0:
                continue
            words = np.where((rl[sel] >= 0) & (rl[sel] <= MAX_LONG_READ_LEN), ((rl[sel] + 15) >> 4) + ((rl[sel] + 31) >> 5), 0)
            sub_off = np.zeros(m + 1, np.int64)                     # (read_off[k] is where read k begins, in any order)
            sub_off[1:] = np.cumsum(words)
            sub = np.ascontiguousarray(np.concatenate([pk[woff[r]:woff[r] + w] for r, w in zip(sel, words)] +
                                                      [np.zeros(1, pk.dtype)]), np.uint32)
            args = [np.ascontiguousarray(rl[sel], np.int32), np.ascontiguousarray(lad[sel], np.int32),
                    np.ascontiguousarray(tpl[sel], np.int32), np.ascontiguousarray(fl[sel], np.int16)]
            o, no, st = np.zeros((m, cap), np.uint32), np.zeros(m, np.int32), np.zeros(m, np.int32)
            self._cigar_call(long_call, MEM_HOST, ladders, sub, sub_off, args[0], m, args[1], args[2], args[3], params, cap, o, no,
                             st)
            ops[sel] = o
            np.asarray(out_n_ops)[sel] = no
            np.asarray(out_status)[sel] = st

    def sw_secondary(self, packed, read_off, read_len, n_items, item_ladder, item_template, mask_len, params, out, out_status,
                     ladders=None):
        """tredsecond_sw_second (include/tredsecond.h): what ssw_align reports as score1 / ref_end1 / score2 / ref_end2 for
        n_items pairs, host memory.  Item k is read k (packed / read_off / read_len as pack_reads writes them) against
        template item_template[k] (db order) of ladder item_ladder[k] with maskLen mask_len[k] (int32 [n]).  out: int32
        [n][4], out_status: int32 [n] (SECOND_*).  ladders: the table the indices refer to (default: the one registered
        with set_ladders).  One unit takes short and long items alike, whether or not the long-read path is on."""
        self._items_call("tredsecond_sw_second", "tredsecond_last_error", ladders, packed, read_off, read_len, n_items,
                         item_ladder, item_template, _ptr(mask_len), C.byref(params), _ptr(out), _ptr(out_status))

    def pileup(self, packed, read_off, read_len, n_items, item_ladder, item_template, fields, ops, cap, n_ops, item_group,
               n_groups, stride, out_counts, out_status, ladders=None):
        """tredpileup_pileup (include/tredpileup.h): the items of sw_cigar -- packed / read_off / read_len, item_ladder,
        item_template, fields as given to it, ops (uint32 [n][cap]) and n_ops as it returned them -- counted per group
        (item_group int32 [n], 0 .. n_groups - 1) and per column of the group's forward template, host memory.  out_counts:
        int32 [n_groups][stride][PILEUP_CHANNELS] (A C G T N under an M operation, deleted, insertions before the column
        and their summed length), stride at least the longest template + 1; out_status: int32 [n] (PILEUP_*).  ladders: the
        table the indices refer to (default: the one registered with set_ladders).  One unit takes short and long items
        alike, whether or not the long-read path is on."""
        self._items_call("tredpileup_pileup", "tredpileup_last_error", ladders, packed, read_off, read_len, n_items, item_ladder,
                         item_template, _ptr(fields), _ptr(ops), cap, _ptr(n_ops), _ptr(item_group), n_groups, stride,
                         _ptr(out_counts), _ptr(out_status))

    def pileup_anchored(self, packed, read_off, read_len, n_items, item_ladder, item_template, fields, ops, cap, n_ops,
                        item_group, item_anchor, n_groups, group_ladder, group_units, stride, out_counts, out_status,
                        ladders=None):
        """tredpileup_pileup_anchored (include/tredpileup.h): pileup with the shape of every group given -- group_ladder,
        group_units (int32 [n_groups]): the allele a >= 1 of the group, which may lie beyond the ladder -- and an anchor per
        item (item_anchor int32 [n], PILEUP_ANCHOR_*): an item of h < a units keeps the flank it is anchored in and the
        tract next to it, moved to where they lie on the group's template.  stride: at least the longest GROUP template
        + 1.  Everything else as pileup takes it."""
        self._items_call("tredpileup_pileup_anchored", "tredpileup_last_error", ladders, packed, read_off, read_len, n_items,
                         item_ladder, item_template, _ptr(fields), _ptr(ops), cap, _ptr(n_ops), _ptr(item_group),
                         _ptr(item_anchor), n_groups, _ptr(group_ladder), _ptr(group_units), stride, _ptr(out_counts),
                         _ptr(out_status))

    def unit_spectrum(self, packed, read_off, read_len, n_items, item_ladder, item_template, fields, ops, cap, n_ops,
                      item_group, n_groups, group_ladder, out_spectrum, out_item, out_status, ladders=None):
        """tredpileup_unit_spectrum (include/tredpileup.h): the items of pileup, counted per group by the repeat-unit
        words they show whole inside one M operation.  group_ladder: int32 [n_groups]; out_spectrum: int32
        [n_groups][SPECTRUM_STRIDE] (bins 0 .. 4^p - 1, then at SPECTRUM_BINS clean units, with_n, touched units, accepted
        items); out_item: int32 [n][3] (N-free clean units, those equal to the repeat, touched units); out_status: int32
        [n] (PILEUP_*, PILEUP_PERIOD for a period above SPECTRUM_MAX_PERIOD).  Everything else as pileup takes it."""
        self._items_call("tredpileup_unit_spectrum", "tredpileup_last_error", ladders, packed, read_off, read_len, n_items,
                         item_ladder, item_template, _ptr(fields), _ptr(ops), cap, _ptr(n_ops), _ptr(item_group), n_groups,
                         _ptr(group_ladder), _ptr(out_spectrum), _ptr(out_item), _ptr(out_status))

    def trio(self, n_items, child, father, mother, ploidy, father_informative, mother_informative, out_status, out_call,
             out_values, out_J, mu=TRIO_MU, rho=TRIO_RHO, beta=TRIO_BETA):
        """tredtrio_evaluate (include/tredtrio.h): n_items (trio, locus) items, host memory.  child, father, mother: the
        members' pair lists as CSR tuples (off int64 [n + 1], a int32, b int32, lw float64), alleles in repeat units;
        ploidy: int32 [n], the child's; father_informative / mother_informative: int32 [n], 0 for a parent that says
        nothing.  out_status: int32 [n] (TRIO_*); out_call: int32 [n][3] (index in the child's list, a, b); out_values:
        float64 [n][4] (Jmax, S, denovo, paternal); out_J: float64, parallel to the child's lists.  Parameters out of
        range raise (-2), as every refusal of the call as a whole does."""
        lists = [_ptr(x) for member in (child, father, mother) for x in member]
        rc = self.lib.tredtrio_evaluate(self.h, C.byref(TrioParams(mu, rho, beta)), n_items, *lists, _ptr(ploidy),
                                        _ptr(father_informative), _ptr(mother_informative), _ptr(out_status), _ptr(out_call),
                                        _ptr(out_values), _ptr(out_J))
        self._chk_side(rc, "tredtrio_evaluate failed ({})".format(rc), self.lib.tredtrio_last_error)

    def cohort(self, n_items, item_off, samples, ploidy, allele_off, out_status, out_n_alleles, out_alleles, out_freq, out_count,
               out_trace, out_sample_call, out_sample_values, out_r, iters=COHORT_ITERS, alpha=COHORT_ALPHA):
        """tredcohort_evaluate (include/tredcohort.h): n_items items -- one locus with its samples each --, host memory.
        item_off: int64 [n + 1], the samples of an item; samples: their pair lists as one CSR tuple (off int64
        [n_samples + 1], a int32, b int32, lw float64), alleles in repeat units; ploidy: int32 [n_samples]; allele_off: int64
        [n + 1], the room of an item in out_alleles (int32), out_freq and out_count (float64).  out_status, out_n_alleles:
        int32 [n]; out_trace: float64 [n][iters][2]; out_sample_call: int32 [n_samples][3] (index in the sample's list, a,
        b); out_sample_values: float64 [n_samples][2] (logZ, post); out_r: float64, parallel to the pairs.  Parameters out
        of range raise (-2), as every refusal of the call as a whole does."""
        rc = self.lib.tredcohort_evaluate(self.h, C.byref(CohortParams(int(iters), float(alpha))), n_items, _ptr(item_off),
                                          *(_ptr(x) for x in samples), _ptr(ploidy), _ptr(allele_off), _ptr(out_status),
                                          _ptr(out_n_alleles), _ptr(out_alleles), _ptr(out_freq), _ptr(out_count), _ptr(out_trace),
                                          _ptr(out_sample_call), _ptr(out_sample_values), _ptr(out_r))
        self._chk_side(rc, "tredcohort_evaluate failed ({})".format(rc), self.lib.tredcohort_last_error)

    def scan(self, letters, seg_off, min_copies=SCAN_MIN_COPIES, cap=1 << 16):
        """tredscan_scan (include/tredscan.h): the tandem repeats of the segments seg_off (int64 [n_seg + 1]) of letters
        (bytes or a uint8 array), host memory.  min_copies: the whole copies a run of period 1 .. 6 needs, 0 for a period
        that is off.  Returns (seg int32, start int64, length int32, period int32, total): the first min(total, cap)
        records in ascending (seg, start, period) order; total is what there is, also above cap."""
        buf = np.frombuffer(letters, np.uint8) if not isinstance(letters, np.ndarray) else letters
        off = np.ascontiguousarray(seg_off, np.int64)
        mc = np.ascontiguousarray(min_copies, np.int32)
        if buf.dtype != np.uint8 or off.ndim != 1 or len(off) < 1 or mc.shape != (SCAN_MAX_PERIOD,):
            raise ValueError("scan: letters are bytes, seg_off has n_seg + 1 entries, min_copies has {}".format(SCAN_MAX_PERIOD))
        if len(buf) < off[-1]:
            raise ValueError("scan: seg_off ends at {} but there are {} letters".format(int(off[-1]), len(buf)))
        cap = int(cap)
        room = max(cap, 0)
        seg, start = np.empty(room, np.int32), np.empty(room, np.int64)
        length, period = np.empty(room, np.int32), np.empty(room, np.int32)
        total = C.c_int64(0)
        rc = self.lib.tredscan_scan(self.h, _ptr(buf) if len(buf) else None, _ptr(off), len(off) - 1, _ptr(mc), cap, _ptr(seg),
                                    _ptr(start), _ptr(length), _ptr(period), C.byref(total))
        self._chk_side(rc, "tredscan_scan failed ({})".format(rc), self.lib.tredscan_last_error)
        n = min(total.value, room)
        return seg[:n], start[:n], length[:n], period[:n], total.value

    def scan_tracts(self, letters, seg_off, min_copies=SCAN_MIN_COPIES, seed_copies=TRACT_SEED_COPIES, max_gap=TRACT_MAX_GAP_DEFAULT,
                    cap=1 << 16):
        """tredtract_scan (include/tredtract.h): the interrupted tandem repeats of the segments seg_off (int64 [n_seg + 1])
        of letters (bytes or a uint8 array), host memory.  Perfect runs of seed_copies whole copies and more (the seeds) of
        one motif in one phase are joined across at most max_gap letters; a tract of min_copies whole copies is a record
        (per period 1 .. 6; a min_copies of 0 switches the period off).  The defaults are a choice, not a measurement.
        Returns (seg int32, start int64, length int32, period int32, seeds int32, mismatch int32, total): the first
        min(total, cap) records in ascending (seg, start, period) order; total is what there is, also above cap."""
        buf = np.frombuffer(letters, np.uint8) if not isinstance(letters, np.ndarray) else letters
        off = np.ascontiguousarray(seg_off, np.int64)
        mc, sc, mg = (np.ascontiguousarray(x, np.int32) for x in (min_copies, seed_copies, max_gap))
        if buf.dtype != np.uint8 or off.ndim != 1 or len(off) < 1 or any(x.shape != (SCAN_MAX_PERIOD,) for x in (mc, sc, mg)):
            raise ValueError("scan_tracts: letters are bytes, seg_off has n_seg + 1 entries, min_copies, seed_copies and max_gap "
                             "have {} each".format(SCAN_MAX_PERIOD))
        if len(buf) < off[-1]:
            raise ValueError("scan_tracts: seg_off ends at {} but there are {} letters".format(int(off[-1]), len(buf)))
        cap = int(cap)
        room = max(cap, 0)
        start = np.empty(room, np.int64)
        seg, length, period, seeds, mismatch = (np.empty(room, np.int32) for _ in range(5))
        total = C.c_int64(0)
        rc = self.lib.tredtract_scan(self.h, _ptr(buf) if len(buf) else None, _ptr(off), len(off) - 1, _ptr(mc), _ptr(sc), _ptr(mg),
                                     cap, _ptr(seg), _ptr(start), _ptr(length), _ptr(period), _ptr(seeds), _ptr(mismatch),
                                     C.byref(total))
        self._chk_side(rc, "tredtract_scan failed ({})".format(rc), self.lib.tredtract_last_error)
        n = min(total.value, room)
        return seg[:n], start[:n], length[:n], period[:n], seeds[:n], mismatch[:n], total.value

    def reset_timing(self):
        self._chk(self.lib.tredgpu_reset_timing(self.h), "tredgpu_reset_timing")
        for _, _, reset_timing, _, last_error in SIDE_UNITS:
            self._chk_side(getattr(self.lib, reset_timing)(self.h), reset_timing + " failed", getattr(self.lib, last_error))

    def get_timing(self, which):
        """(launches, total device ms) of kernel `which` since reset_timing (HIP events)."""
        n, ms = C.c_int64(0), C.c_double(0)
        for _, get_timing, _, kernel, last_error in SIDE_UNITS:
            if which == kernel:
                self._chk_side(getattr(self.lib, get_timing)(self.h, C.byref(n), C.byref(ms)), get_timing + " failed",
                               getattr(self.lib, last_error))
                return n.value, ms.value
        self._chk(self.lib.tredgpu_get_timing(self.h, which, C.byref(n), C.byref(ms)), "tredgpu_get_timing")
        return n.value, ms.value

    def get_sw_counters(self):
        """dict of the SW kernel's work counters since reset_timing (tredgpu_get_sw_counters)."""
        out = np.zeros(8, np.uint64)
        self._chk(self.lib.tredgpu_get_sw_counters(self.h, out.ctypes.data), "tredgpu_get_sw_counters")
        keys = ("trunk_cols", "continuation_cols", "templates_combined", "templates_dropped", "emitted_from_trunk", "waves", "read_cols")
        return {k: int(v) for k, v in zip(keys, out)}

    def pe_kde(self, mem, units, n_units, global_lens, n_global_total, pdf_out, status_out):
        self._chk(self.lib.tredgpu_pe_kde(self.h, mem, _ptr(units), n_units, _ptr(global_lens),
                                          n_global_total, _ptr(pdf_out), _ptr(status_out)), "tredgpu_pe_kde")


def default_sw_params(clip=False, max_read_len=0):
    """bam_parser.py:95-98 scoring (1/5/7/2), FLANKMATCH 9 (bam_parser.py:30)."""
    return SwParams(1, 5, 7, 2, 9, int(bool(clip)), int(max_read_len), 0)


class WalkArgs(C.Structure):
    """tredgpu_walk_args (include/tredgpu.h)."""
    _fields_ = [("blk_coffset", C.c_void_p), ("blk_clen", C.c_void_p), ("blk_crc", C.c_void_p),
                ("tasks", C.c_void_p), ("n_tasks", C.c_int32), ("chunks", C.c_void_p), ("n_chunks", C.c_int32),
                ("results", C.c_void_p), ("global_pool", C.c_void_p), ("cap_global", C.c_int64),
                ("target_pool", C.c_void_p), ("cap_target", C.c_int64), ("n_global", C.c_int64), ("n_target", C.c_int64),
                ("alt_tasks", C.c_void_p), ("n_alt_tasks", C.c_int32), ("alt_chunks", C.c_void_p), ("n_alt_chunks", C.c_int32),
                ("alt_results", C.c_void_p), ("need", C.c_void_p), ("select", C.c_void_p), ("selected", C.c_void_p)]


class SelectedUnits(C.Structure):
    """tredgpu_selected_units (include/tredgpu.h section 5)."""
    _fields_ = [("inf", C.c_void_p), ("n_units", C.c_int32), ("pad", C.c_int32), ("task", C.c_void_p)]


# layouts of tredgpu_walk_task / _chunk / _result (the same as bamio.WALK_*_DTYPE: tredbam.h's structs)
WALK_TASK_DTYPE = np.dtype([(k, "<i4") for k in ("tid", "start", "end", "tstart", "tend", "span", "chunk_first", "n_chunks",
                                                 "block_first", "block_end", "win_lo", "win_hi")])
WALK_CHUNK_DTYPE = np.dtype([("begin_block", "<i4"), ("begin_upos", "<i4"), ("end_voffset", "<u8")])
WALK_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_global", "<i4"), ("n_target", "<i4"), ("n_window", "<i4"),
                              ("global_first", "<i8"), ("target_first", "<i8"), ("win_vbeg", "<u8"), ("win_vend", "<u8")])
ALT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("vbeg", "<u8", (6,))])
# tredgpu_select_task / tredgpu_select_result (section 5: the read selection on the device)
SELECT_TASK_DTYPE = np.dtype([("pos_lo", "<i4"), ("pos_hi", "<i4"), ("alt_first", "<i4"), ("n_alt", "<i4")])
SELECT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_reads", "<i4"), ("n_words", "<i4"), ("seq4_bytes", "<i4"), ("name_bytes", "<i4"),
                                ("max_len", "<i4"), ("depth_sum", "<i8")])
assert SELECT_TASK_DTYPE.itemsize == 16 and SELECT_RESULT_DTYPE.itemsize == 32
SELECT_CAP = 4096


MIN_PAIR_BYTES = 2 * (36 + 2 + 4 + 18)    # two BAM records of a pair at their smallest: fixed fields, name, one CIGAR op, 36 bases


def walk_pool_pairs(tasks, out_off):
    """Upper bound of the pair lengths one walk call can produce -- the room its pools are given, shared by all tasks:
    every pair needs two records among the call's inflated bytes (out_off: the call's block offsets; a record of a read
    of >= 36 bases cannot be smaller than MIN_PAIR_BYTES / 2), and a byte belongs to the regions of at most two loci
    (FXS / FXTAS and SBMA / AR share their coordinates; loci further apart than +-10 kb share nothing).  30x samples
    sit near a tenth of this bound; a locus list with three or more loci on one spot could exceed it -- those regions
    then come back with status 6 and the host walks them."""
    if len(tasks) == 0:
        return 0
    return 2 * int(np.asarray(out_off, np.int64)[-1]) // MIN_PAIR_BYTES + 64 * len(tasks)


class Inflater:
    """Batch DEFLATE decoder on the GPU (include/tredgpu.h section 4): one HIP stream with pinned staging; one per host
    thread.  ``reserve`` hands out numpy views of the staging buffers -- compressed payloads and their offsets are
    written into them, the inflated bytes are read from ``out`` in place after ``run``."""

    def __init__(self, device=0, host_out=True):
        """host_out=False: no pinned host copy of the whole output (run / fetch are then not available: run_walk and
        fetch_dense are) -- 45 MB less page-locked memory per 30x sample of a call."""
        self._lib = load()
        self._h = C.c_void_p()
        rc = self._lib.tredgpu_inflater_create(device, C.byref(self._h))
        if rc != 0:
            raise TredGpuError("tredgpu_inflater_create: %s (rc=%d)" % (self._lib.tredgpu_inflater_last_error(None).decode(), rc))
        self.comp_addr = self.out_addr = 0
        self.host_out = bool(host_out)
        if not host_out:
            self._check(self._lib.tredgpu_inflater_host_out(self._h, 0), "tredgpu_inflater_host_out")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.tredgpu_inflater_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: the module globals may be gone
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise TredGpuError("%s: %s (rc=%d)" % (what, self._lib.tredgpu_inflater_last_error(self._h).decode(), rc))
        return rc

    def reserve(self, comp_bytes, out_bytes, n_blocks):
        """(comp, out, comp_off, out_off): uint8 views of comp_bytes / out_bytes bytes, int64 views of n_blocks + 1."""
        ptr = [C.c_void_p() for _ in range(4)]
        self._check(self._lib.tredgpu_inflater_reserve(self._h, comp_bytes, out_bytes, n_blocks, *[C.byref(p) for p in ptr]),
                    "tredgpu_inflater_reserve")
        self.comp_addr, self.out_addr = ptr[0].value, ptr[1].value or 0

        def view(p, ctype, n):
            if not p.value:
                return None                   # (host_out=False: there is no host copy of the output)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(max(n, 1),))[:n]
        return (view(ptr[0], C.c_uint8, comp_bytes), view(ptr[1], C.c_uint8, out_bytes),
                view(ptr[2], C.c_int64, n_blocks + 1), view(ptr[3], C.c_int64, n_blocks + 1))

    def run(self, n_blocks, crc=False):
        """Decodes the n_blocks blocks laid out in the reserved buffers; returns the int32 status per block -- with
        ``crc=True`` (status, uint32 CRC-32 of every block's inflated bytes, computed on the device)."""
        status = np.zeros(max(n_blocks, 1), np.int32)
        if not crc:
            self._check(self._lib.tredgpu_inflate_blocks(self._h, n_blocks, status.ctypes.data), "tredgpu_inflate_blocks")
            return status[:n_blocks]
        sums = np.zeros(max(n_blocks, 1), np.uint32)
        self._check(self._lib.tredgpu_inflate_blocks_crc(self._h, n_blocks, status.ctypes.data, sums.ctypes.data), "tredgpu_inflate_blocks_crc")
        return status[:n_blocks], sums[:n_blocks]

    def run_walk(self, n_blocks, blk_coffset, blk_clen, blk_crc, tasks, chunks, pairs_per_task=2048, alt_tasks=None, alt_chunks=None,
                 pool_pairs=None, select=None):
        """tredgpu_inflate_walk: decodes the blocks laid out in the reserved buffers and walks the pair-length regions
        (tasks WALK_TASK_DTYPE, chunks WALK_CHUNK_DTYPE) over them on the device.  No block is copied back (fetch does
        that).  Returns (status, crc, results WALK_RESULT_DTYPE, global pool, target pool) -- with alt_tasks / alt_chunks
        (the alternative loci's walks) also (results ALT_RESULT_DTYPE, uint8 flags of the blocks that hold their records).
        pool_pairs: room in the global pool for the whole call (walk_pool_pairs: a bound from the planned bytes, so that
        no coverage makes a region fall back to the host for want of room); without it pairs_per_task per task.
        select (SELECT_TASK_DTYPE, one per task): the read selection, depth sums and sizes where the records are (tredgpu.h
        section 5) -- the results (SELECT_RESULT_DTYPE) are appended to the returned tuple, the selected records stay on the
        device for Context.genotype_selected."""
        status, sums = np.zeros(max(n_blocks, 1), np.int32), np.zeros(max(n_blocks, 1), np.uint32)
        coff = np.ascontiguousarray(blk_coffset, np.int64)
        clen = np.ascontiguousarray(blk_clen, np.int32)
        xcrc = np.ascontiguousarray(blk_crc, np.uint32)
        tasks = np.ascontiguousarray(tasks, WALK_TASK_DTYPE)
        chunks = np.ascontiguousarray(chunks, WALK_CHUNK_DTYPE)
        if not (len(coff) == len(clen) == len(xcrc) == n_blocks):
            raise ValueError("one compressed offset / length / CRC per block")
        res = np.zeros(max(len(tasks), 1), WALK_RESULT_DTYPE)
        room = len(tasks) * int(pairs_per_task) if pool_pairs is None else int(pool_pairs)
        gp = np.zeros(room + 4096, np.int32)
        tp = np.zeros(max(room // 8, 16 * len(tasks)) + 1024, np.int32)
        n_alt = 0 if alt_tasks is None else len(alt_tasks)
        at = np.ascontiguousarray(alt_tasks if n_alt else np.zeros(1, WALK_TASK_DTYPE), WALK_TASK_DTYPE)
        ac = np.ascontiguousarray(alt_chunks if (n_alt and len(alt_chunks)) else np.zeros(1, WALK_CHUNK_DTYPE), WALK_CHUNK_DTYPE)
        ares = np.zeros(max(n_alt, 1), ALT_RESULT_DTYPE)
        need = np.zeros(max(n_blocks, 1), np.uint8)
        sel = selres = None
        if select is not None:
            sel = np.ascontiguousarray(select, SELECT_TASK_DTYPE)
            if len(sel) != len(tasks):
                raise ValueError("one select task per walk task")
            selres = np.zeros(max(len(tasks), 1), SELECT_RESULT_DTYPE)
        a = WalkArgs(coff.ctypes.data, clen.ctypes.data, xcrc.ctypes.data, tasks.ctypes.data, len(tasks), chunks.ctypes.data,
                     len(chunks), res.ctypes.data, gp.ctypes.data, len(gp), tp.ctypes.data, len(tp), 0, 0,
                     at.ctypes.data, n_alt, ac.ctypes.data, len(alt_chunks) if n_alt else 0, ares.ctypes.data, need.ctypes.data,
                     sel.ctypes.data if sel is not None and len(sel) else None, selres.ctypes.data if sel is not None and len(sel) else None)
        self._check(self._lib.tredgpu_inflate_walk(self._h, n_blocks, status.ctypes.data, sums.ctypes.data, C.byref(a)),
                    "tredgpu_inflate_walk")
        out = (status[:n_blocks], sums[:n_blocks], res[:len(tasks)], gp[:a.n_global], tp[:a.n_target])
        if alt_tasks is not None:
            out = out + (ares[:n_alt], need[:n_blocks])
        return out if select is None else out + (selres[:len(tasks)],)

    def fetch(self, need):
        """tredgpu_inflater_fetch: the blocks with need[k] != 0 of the last run_walk, to their places in ``out``."""
        need = np.ascontiguousarray(need, np.uint8)
        return self._check(self._lib.tredgpu_inflater_fetch(self._h, len(need), need.ctypes.data), "tredgpu_inflater_fetch")

    def fetch_dense(self, need):
        """tredgpu_inflater_fetch_dense: the blocks with need[k] != 0 of the last run_walk (and short gaps between them),
        one after the other in a pinned buffer of their own; returns (address, int64 offsets[n + 1]): block k lies at
        address + offsets[k] and is offsets[k + 1] - offsets[k] bytes long (0: not copied)."""
        need = np.ascontiguousarray(need, np.uint8)
        off = np.zeros(len(need) + 1, np.int64)
        host = C.c_void_p()
        self._check(self._lib.tredgpu_inflater_fetch_dense(self._h, len(need), need.ctypes.data, C.byref(host), off.ctypes.data),
                    "tredgpu_inflater_fetch_dense")
        return host.value or 0, off

    def pinned_bytes(self):
        """Page-locked host memory this inflater holds, in bytes."""
        return int(self._lib.tredgpu_inflater_pinned_bytes(self._h)) if self._h else 0

    def walk_serial_regions(self):
        """Regions of the last run_walk whose records the serial chain listed (the lane-parallel one handed them back)."""
        return int(self._lib.tredgpu_inflater_walk_serial_regions(self._h))

    def walk_ms(self):
        a = C.c_double()
        self._check(self._lib.tredgpu_inflater_walk_ms(self._h, C.byref(a)), "tredgpu_inflater_walk_ms")
        return a.value

    def timing(self):
        """(total_ms, kernel_ms) of the last call on the device."""
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.tredgpu_inflater_timing(self._h, C.byref(a), C.byref(b)), "tredgpu_inflater_timing")
        return a.value, b.value
