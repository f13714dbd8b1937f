/* tredsecond.h -- the second-best alignment of ssw_align, on the GPU (libtredgpu.so, gfx950), under a prefix of its own
 * as tredlong.h and tredcigar.h are (tredgpu.h is the ABI of the kernels the profiles under profiles/ were taken from).
 *
 * The reference's s_align carries score2 / ref_end2 (src/ssw.h:30-49): the best score that ends at least maskLen columns
 * away from the optimal end, and the column where it ends.  On a tandem repeat score1 - score2 is the only measure ssw
 * offers of how firmly a read is placed.  tredsecond_sw_second restates what src/ssw.c computes, quirks included:
 *   1. padding rows take part.  The byte pass pads the read to a multiple of 16 rows and the word pass to a multiple of
 *      8; a padding row scores 0 against every letter (:108) and maxColumn[c] is the maximum over real and padding rows,
 *      E and F running through them (:215, :448), so a value of the read's last rows is carried diagonally into later
 *      columns.  score1 / ref_end1 do not notice (a padding cell never exceeds a real cell of an earlier column);
 *   2. the byte pass counts when score1 + mismatch < 255, otherwise the word pass is run afresh (:283, :317, :806-810);
 *   3. the mask: the columns 0 .. max(ref_end1 - maskLen, 0) - 1 and those from e = min(ref_end1 + maskLen, refLen) in
 *      the word pass, from e + 1 in the byte pass (:334 against :537); a column replaces the running best only when
 *      strictly greater; nothing found is 0 / 0, and maskLen < 15 is 0 / -1 (:828-834);
 *   4. maskLen is the caller's (Aligner.align passes len(query) / 2 beyond 30 letters and 15 otherwise, ssw_wrap.py:198-201).
 * Every cell is the full recurrence.  With gap_open == gap_extend the reference's word pass can leave its lazy-F loop
 * early (:468-479) and a column maximum of its own then falls short of the recurrence's; the kernel does not copy that.
 *
 * Opt-in: nothing else in libtredgpu calls it (Aligner(report_secondary=True), tredparse_amd/ssw.py).
 */
#ifndef TREDSECOND_H
#define TREDSECOND_H

#include "tredgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TREDGPU_SECOND_OK 0
#define TREDGPU_SECOND_TOO_LONG 4  /* read beyond TREDGPU_MAX_LONG_READ_LEN or template beyond TREDGPU_MAX_LONG_TEMPLATE_LEN
                                      (tredlong.h); the values are those of TREDGPU_CIGAR_TOO_LONG / _BAD_ITEM */
#define TREDGPU_SECOND_BAD_ITEM 5  /* ladder or template index out of range, or a negative read length */

#define TREDGPU_KERNEL_SECOND 18   /* the timing selector of the binding (tredcigar.h has 16, the long CIGAR 17) */

/*
 * score1 / ref_end1 / score2 / ref_end2 of n_items (read, template) pairs on the context's stream.  HOST memory only:
 * copies in, runs, copies out, waits.
 *   n_ladders, prefix, repeat, suffix, max_units   the template ladders, as tredcigar_sw_cigar takes them (uploaded
 *                      again only when they differ from the previous call's; the context's own table is not used)
 *   packed, read_off[n_items+1], read_len[n_items]  the items' reads, as tredgpu_pack_reads writes them
 *   item_ladder[n_items], item_template[n_items]    the template: ladder index, template index in db order (u=1 fwd,
 *                      u=1 rc, u=2 fwd, ...; 0 for a plain reference)
 *   mask_len[n_items]  maskLen of ssw_align
 *   params             scoring (match, mismatch, gap_open, gap_extend; the other members are not used)
 *   out                int32 [n_items][4] = {score1, ref_end1, score2, ref_end2}; ref_end1 is -1 where score1 is 0, as
 *                      ssw_align leaves it; all four are 0 for an item that is not TREDGPU_SECOND_OK
 *   out_status[n_items] (TREDGPU_SECOND_*)
 * The call needs nothing from tredgpu_sw_classify: score1 / ref_end1 are its own (and equal that call's dump).
 * One wavefront per item, reads of up to TREDGPU_MAX_LONG_READ_LEN bp and templates of up to
 * TREDGPU_MAX_LONG_TEMPLATE_LEN columns in one unit (csrc/sw_second.hip).
 * Returns 0, -2 bad arguments or a refused scoring, -10 HIP error; tredsecond_last_error() has the text (per thread).
 * tredsecond_release frees what the calls on a context hold (ladder table, staging buffers, timing events): call it
 * before tredgpu_destroy; calling it again, or before any call, does nothing.
 */
int tredsecond_sw_second(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                         const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                         const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                         const int32_t* mask_len, const tredgpu_sw_params* params, int32_t* out, int32_t* out_status);
/* calls of tredsecond_sw_second on this context since tredsecond_reset_timing and the summed device time of their
   kernels (HIP events, one pair around the launches of a call) */
int tredsecond_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms);
int tredsecond_reset_timing(tredgpu_ctx* ctx);
void tredsecond_release(tredgpu_ctx* ctx);
const char* tredsecond_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
