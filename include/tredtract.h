/* tredtract.h -- interrupted tandem repeats of a letter sequence on the GPU (libtredgpu.so, gfx950), under a prefix of its
 * own as tredscan.h is.  tredscan_scan reports perfect repeats only: an interruption ends a run.  tredtract_scan joins the
 * perfect runs of one motif in one phase that a few substituted letters separate -- (CGG)9 AGG (CGG)9 AGG (CGG)10 is one
 * tract of 30 copies with 2 mismatches, not three runs ("Interrupted tracts"; the restatement in Python, by all
 * pairs and connected components, is tests/tract_model.py).
 *
 * Opt-in: nothing else in libtredgpu calls it (Context.scan_tracts, prepare.scan_repeats(interruptions=...), python -m
 * tredparse_amd.prepare scan --interruptions).
 */
#ifndef TREDTRACT_H
#define TREDTRACT_H

#include "tredscan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TREDTRACT_MAX_GAP 64                /* the most letters between two linked seeds */
#define TREDGPU_KERNEL_TRACT 23             /* the timing selector of the binding (tredscan.h has 22) */

/*
 * The tracts of n_seg segments of one byte buffer, on the context's stream.  HOST memory only: copies in, runs, copies
 * out, waits.  letters, seg_off, codes, segments, e_p, maximal runs, whole copies and "primitive" are tredscan.h's.
 *   min_copies[6]      per period p = 1 .. 6 at [p - 1]: the whole copies a tract needs to be reported, 2 at the least; 0
 *                      switches the period off
 *   seed_copies[6]     the whole copies a perfect run needs to take part
 *   max_gap[6]         the most letters between two seeds that are joined
 * SEED.  A seed of period p is a maximal period-p run [a, a + L) with L / p >= seed_copies[p - 1] and a primitive motif:
 * what tredscan_scan reports with seed_copies in the place of min_copies.  Every letter of a seed is A/C/G/T.  Its template
 * is the periodic function T(x) = code(s[a + ((x - a) mod p)]).
 * LINK.  Two seeds [a1, b1) and [a2, b2) of one segment and one period p, a1 < a2, are linked iff the gap g = a2 - b1 has
 * 1 <= g <= max_gap[p - 1] and they have the same template: code(s[a2 + j]) == code(s[a1 + ((a2 - a1 + j) mod p)]) for
 * j = 0 .. p - 1 -- the same motif in the same phase, so what separates them is substitutions only.  Codes are compared,
 * not bytes: cag and CAG are the same.
 * TRACT.  A tract is a connected component of the link relation (a seed without a link is a tract of one seed).  It spans
 * from its first seed's start to its last seed's end (start, L); seeds is the number of its seeds; mismatch is the number
 * of x in [start, start + L) with code(s[x]) != T(x) -- they lie in the gaps only, and an N in a gap is one.  It is a record
 * iff L / p >= min_copies[p - 1].  Tracts of different periods that overlap are all records.
 *   out_seg, out_len, out_period, out_seeds, out_mismatch   int32 [out_cap]
 *   out_start                                               int64 [out_cap]: 0-based within the segment
 *   out_n              the number of records found, also where it exceeds out_cap: the first out_cap records are written
 *                      then, and nothing beyond the first min(*out_n, out_cap) entries of an array is touched
 * The records are in ascending (segment, start, period) order, and a call repeated gives the same bytes: every seed, tract
 * and record has its place from a count and a prefix sum in a fixed order, none from the order in which wavefronts finish.
 *
 * ARGUMENTS.  min_copies follows tredscan_scan: 0 (off) or 2 and above, not every period off.  For each period that is on:
 *   2 <= seed_copies[p - 1] <= min_copies[p - 1]
 *   0 <= max_gap[p - 1] <= TREDTRACT_MAX_GAP
 *   seed_copies[p - 1] * p > max_gap[p - 1] + 2 p - 2
 * seed_copies and max_gap of a period that is off are not read.  The last rule: two maximal runs of one period share at
 * most p - 1 letters, so a period-p seed that starts between two linked seeds would be at most g + 2 p - 2 letters long;
 * under the rule there is none, a seed's only possible partner to the left is its predecessor among the seeds of its
 * period, and tracts are the maximal stretches of consecutive linked seeds of the per-period list.  With max_gap all 0 and
 * seed_copies == min_copies the records are tredscan_scan's, each with 1 seed and 0 mismatches.
 * The defaults of the binding (seed_copies 5,3,3,3,3,3, max_gap 1,2,3,4,5,6: one unit) are a choice, not a measurement.
 * Known limit: a lone unit behind an interruption is not absorbed (the last CAG of ...CAG CAA CAG CCG... is no seed).
 *
 * Returns 0, -2 bad arguments (tredscan_scan's, with seed_copies, max_gap and the two new out arrays among the arrays that
 * may not be NULL, and a violation of the rules above: nothing is written then, *out_n included), -10 HIP error, a workspace
 * that cannot be allocated included; tredtract_last_error() has the text (per thread).  At most TREDSCAN_MAX_LETTERS letters
 * per call.  The workspace is 169 bytes per tile of 4096 letters and 17 bytes per seed; seeds are counted in 31 bits, which
 * 2^30 letters cannot exceed (starts of one period are p + 1 apart at the least), and a count that did would be refused
 * with -2.  tredtract_release frees what the calls on a context hold: call it before tredgpu_destroy; calling it again, or
 * before any call, does nothing.
 */
int tredtract_scan(tredgpu_ctx* ctx, const uint8_t* letters, const int64_t* seg_off, int32_t n_seg, const int32_t* min_copies,
                   const int32_t* seed_copies, const int32_t* max_gap, int64_t out_cap, int32_t* out_seg, int64_t* out_start,
                   int32_t* out_len, int32_t* out_period, int32_t* out_seeds, int32_t* out_mismatch, int64_t* out_n);
/* calls of tredtract_scan on this context since tredtract_reset_timing and the summed device time of their kernels (HIP
   events, one pair around the launches of a call) */
int tredtract_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms);
int tredtract_reset_timing(tredgpu_ctx* ctx);
void tredtract_release(tredgpu_ctx* ctx);
const char* tredtract_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
