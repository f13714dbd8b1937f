/* tredcigar.h -- the CIGAR of an alignment, on the GPU (libtredgpu.so, gfx950), under a prefix of its own as
 * tredlong.h is (tredgpu.h is the ABI of the kernels the profiles under profiles/ were taken from).
 *
 * The reference computes a CIGAR on every Aligner.align call: src/ssw_wrap.py:203-211 passes flag 1, ssw_align then
 * runs banded_sw (src/ssw.c:852-867 -> :549-736) over the rectangle ref[ref_begin..ref_end] x read[read_begin..read_end]
 * and ssw_wrap.py:284-383 formats the result.  tredcigar_sw_cigar restates banded_sw exactly, quirks included, so the
 * operations are the reference's and not merely valid ones:
 *   - the band starts at |refLen - readLen| + 1 and doubles while the banded maximum is below `score` (:572-633);
 *   - the cells above a row's last band column read H = 0 and E = 0 (h_b[edge] / e_b[edge], :596-597) -- which also
 *     wipes the real cell above the last column of the rectangle while the band still starts at column 0;
 *   - f restarts at 0 in every row; E and F are stored unfloored, only e1 / f1 are floored (:608-620);
 *   - direction codes 1-5: the diagonal wins a tie (:627), F wins over E unless e1 > f1 (:628), a gap extends unless
 *     opening is strictly better (:612, :617);
 *   - the traceback starts at the last cell, runs until i == 0 whatever H is, and closes with e+1 M or with `e op`
 *     followed by 1M (:636-715); the list is then reversed (:717-726).
 * Where the reference runs off its buffers the item gets a status instead, never an out-of-range access.
 *
 * Opt-in: nothing else in libtredgpu calls it (Aligner(report_cigar=True), tredparse_amd/ssw.py).
 */
#ifndef TREDCIGAR_H
#define TREDCIGAR_H

#include "tredgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TREDGPU_CIGAR_OK 0
#define TREDGPU_CIGAR_NO_PATH 1   /* the band covers the whole rectangle and the maximum is still below score: the
                                     fields do not belong to the pair (the reference keeps doubling, ref_driver.c:15-23) */
#define TREDGPU_CIGAR_OFF_EDGE 2  /* the traceback stepped to a cell the band of its row does not hold (j < 0 included) */
#define TREDGPU_CIGAR_OVERFLOW 3  /* more than `cap` operations; out_n_ops holds the true count, the item's ops are zero */
#define TREDGPU_CIGAR_TOO_LONG 4  /* read beyond TREDGPU_MAX_READ_LEN or template beyond TREDGPU_MAX_TEMPLATE_LEN */
#define TREDGPU_CIGAR_BAD_ITEM 5  /* ladder / template index or fields outside the pair (begin < 0, end < begin, end >= length) */

#define TREDGPU_KERNEL_CIGAR 16   /* the timing selector of tredcigar_get_timing.  Not the next value of tredgpu.h's
                                     series: tredgpu_get_timing knows 0-6 only and keeps refusing anything else */

/*
 * The CIGAR of n_items alignments on the context's stream.
 *   n_ladders, prefix, repeat, suffix, max_units   the template ladders (tredgpu_set_ladders' arguments, HOST memory
 *                      always; the context's own table is not used or changed; uploaded again only when they differ
 *                      from the previous call's)
 *   packed, read_off[n_items+1], read_len[n_items]  the items' reads, as tredgpu_pack_reads writes them
 *   item_ladder[n_items], item_template[n_items]    the template: ladder index, template index in db order (u=1 fwd,
 *                      u=1 rc, u=2 fwd, ...; 0 for a plain reference)
 *   fields             int16 [n_items][5] = {score, ref_begin, ref_end, read_begin, read_end}: the first five values of a
 *                      row of tredgpu_sw_classify's out_dump
 *   params             scoring (match, mismatch, gap_open, gap_extend; the other members are not used)
 *   out_ops            uint32 [n_items][cap]: length << 4 | op, M=0 I=1 D=2 (to_cigar_int, ssw.h:132-156), oldest first;
 *                      entries behind the item's n_ops are zero
 *   out_n_ops[n_items], out_status[n_items] (TREDGPU_CIGAR_*)
 * mem: TREDGPU_MEM_HOST (copies in, runs, copies out, waits) or TREDGPU_MEM_DEVICE (the item arrays and outputs are device
 * pointers; the call only enqueues).  Returns 0, -2 bad arguments, -10 HIP error; tredcigar_last_error() has the text
 * (per thread).  tredcigar_release frees what the calls on a context hold (workspace, ladder table, timing events): call it
 * before tredgpu_destroy.
 */
int tredcigar_sw_cigar(tredgpu_ctx* ctx, int mem, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                       const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                       const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                       const int16_t* fields, const tredgpu_sw_params* params, int32_t cap, uint32_t* out_ops,
                       int32_t* out_n_ops, int32_t* out_status);
/* launches of the CIGAR kernels on this context since tredcigar_reset_timing and their summed device time (HIP events) */
int tredcigar_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms);
int tredcigar_reset_timing(tredgpu_ctx* ctx);
void tredcigar_release(tredgpu_ctx* ctx);
const char* tredcigar_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
