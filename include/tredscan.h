/* tredscan.h -- perfect tandem repeats of a letter sequence on the GPU (libtredgpu.so, gfx950), under a prefix of its own
 * as tredlong.h, tredcigar.h, tredsecond.h, tredpileup.h, tredtrio.h and tredcohort.h are (tredgpu.h is the ABI of the
 * kernels the profiles under profiles/ were taken from).
 *
 * Every other entry of the library works on the reads of the 32 loci of the table.  tredscan_scan answers the question
 * in front of that table: where in a sequence are the repeats?  One streaming pass over the letters, integer-exact
 * ("Tandem-repeat scan"; the numpy restatement is tests/scan_model.py).
 *
 * Opt-in: nothing else in libtredgpu calls it (Context.scan, prepare.scan_repeats, python -m tredparse_amd.prepare scan).
 */
#ifndef TREDSCAN_H
#define TREDSCAN_H

#include "tredgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TREDSCAN_MAX_PERIOD 6
#define TREDSCAN_TILE 4096                  /* letters one wavefront owns: 64 lanes of 64 letters (csrc/scan.hip) */
#define TREDSCAN_MAX_LETTERS 1073741824LL   /* 2^30 letters of all segments of one call: out_len is an int32, and the
                                               largest human chromosome (2^28 letters) is one call four times over */
#define TREDGPU_KERNEL_SCAN 22              /* the timing selector of the binding (tredcohort.h has 21) */

/*
 * The repeats of n_seg segments of one byte buffer, on the context's stream.  HOST memory only: copies in, runs, copies
 * out, waits.
 *   letters            the bytes of all segments; Aa -> 0, Cc -> 1, Gg -> 2, Tt -> 3, any other byte -> 4 (N)
 *   seg_off[n_seg + 1] segment k is letters[seg_off[k] .. seg_off[k + 1]); the offsets are not negative and do not
 *                      descend (a segment may be empty; bytes below seg_off[0] belong to no segment).  Nothing crosses a
 *                      segment's end
 *   min_copies[6]      per period p = 1 .. 6 at [p - 1]: the whole copies a run needs to be reported, 2 at the least; 0
 *                      switches the period off
 * With s the codes of a segment of n letters and e_p[i] = 1 iff i + p < n, s[i] <= 3 and s[i] == s[i + p]: a maximal run of
 * ones [i0, i1) of e_p is the maximal substring [i0, i1 + p) of period p, of length L = i1 - i0 + p, L / p whole copies and
 * the motif s[i0 .. i0 + p) (in genomic phase, not canonicalised).  It is a record iff L / p >= min_copies[p - 1] and the
 * motif is primitive (has no period d with d | p, d < p: such a run lies inside the period-d run, which is reported).
 * Overlapping runs of different periods are all records.
 *   out_seg, out_len, out_period   int32 [out_cap]: the segment, L (the partial last copy included), p
 *   out_start                      int64 [out_cap]: i0, 0-based within the segment
 *   out_n              the number of records found, also where it exceeds out_cap: the first out_cap records are written
 *                      then, and nothing beyond the first min(*out_n, out_cap) entries of an array is touched
 * The records are in ascending (segment, start, period) order, and a call repeated gives the same bytes: every record has
 * its place from a count and a prefix sum, none from the order in which wavefronts finish.  A run is one record however
 * long it is and whatever tiles it crosses.
 * Returns 0, -2 bad arguments (a NULL argument, n_seg < 0, offsets that are negative or descend, more than
 * TREDSCAN_MAX_LETTERS letters, a min_copies of 1 or below 0, every period off, out_cap < 0: nothing is written then, *out_n
 * included), -10 HIP error; tredscan_last_error() has the text (per thread).  letters may be NULL where there is no letter,
 * the four out arrays where out_cap is 0.  tredscan_release frees what the calls on a context hold (staging buffers, timing
 * events): call it before tredgpu_destroy; calling it again, or before any call, does nothing.
 */
int tredscan_scan(tredgpu_ctx* ctx, const uint8_t* letters, const int64_t* seg_off, int32_t n_seg, const int32_t* min_copies,
                  int64_t out_cap, int32_t* out_seg, int64_t* out_start, int32_t* out_len, int32_t* out_period, int64_t* out_n);
/* calls of tredscan_scan on this context since tredscan_reset_timing and the summed device time of their kernels (HIP
   events, one pair around the launches of a call) */
int tredscan_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms);
int tredscan_reset_timing(tredgpu_ctx* ctx);
void tredscan_release(tredgpu_ctx* ctx);
const char* tredscan_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
