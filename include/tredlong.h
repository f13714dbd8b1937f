/* tredlong.h -- the long-read path of libtredgpu.so (gfx950), under a prefix of its own (tredgpu.h is the ABI of the
 * other kernels): exact template-ladder Smith-Waterman + tagging for reads of up to TREDGPU_MAX_LONG_READ_LEN bp against ladders of up to TREDGPU_MAX_LONG_TEMPLATE_LEN columns, where
 * tredgpu_sw_classify stops at TREDGPU_MAX_READ_LEN / TREDGPU_MAX_TEMPLATE_LEN.
 *
 * Same results as tredgpu_sw_classify for every read both accept: per template the five s_align fields of ssw_align
 * (tie rules of sw_ladder.hip: begin = largest start column, then largest start row; end = first column reaching
 * the max, then smallest row) and per read the tag / h / score of _parseReadSW.  Its DP values are 64-bit, so the
 * scoring range is only the parameter range of tredgpu_sw_params (no packed-value bound).
 *
 * The path is opt-in: nothing else in libtredgpu calls it.  The Python binding (tredparse_amd/_lib.py,
 * Context.set_long_reads) routes a read here when it is longer than TREDGPU_MAX_READ_LEN or its ladder is longer than
 * TREDGPU_MAX_TEMPLATE_LEN, and every other read of the call to tredgpu_sw_classify as before.
 *
 * tredlong_sw_cigar is the CIGAR of such alignments: tredcigar_sw_cigar (tredcigar.h) stops at TREDGPU_MAX_READ_LEN /
 * TREDGPU_MAX_TEMPLATE_LEN and keeps answering TREDGPU_CIGAR_TOO_LONG beyond them; Context.sw_cigar sends those items here.
 */
#ifndef TREDLONG_H
#define TREDLONG_H

#include "tredgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TREDGPU_MAX_LONG_READ_LEN 2048      /* 12-bit fields */
#define TREDGPU_MAX_LONG_TEMPLATE_LEN 4095

/*
 * Classify n_reads reads (HOST memory, tredgpu_pack_reads layout) on the context's stream; read r is aligned against
 * ladder read_ladder[r] of the n_ladders given here (tredgpu_set_ladders' arguments and layout; the context's own
 * table is not used or changed).  out_dump (optional): [n_reads][dump_templates][6] int16 as in tredgpu_sw_classify.
 * read_off[0] must not be negative (-2, "read_off must be monotone"), and read r has exactly the words of its length.
 * Waits for the results.  The context keeps the packed ladder table (uploaded again only when a call names another one)
 * and the staging buffers between calls, grow-only; tredlong_release frees them.  Cost beyond the kernel: the copies
 * from and to the caller's pageable arrays -- meant for the minority of reads the short kernels cannot hold; a sample
 * whose reads are all longer than TREDGPU_MAX_READ_LEN sends all of them here.  Returns 0, -2 bad arguments, -5 a read
 * beyond TREDGPU_MAX_LONG_READ_LEN, -10 HIP error; the message is in tredlong_last_error() (per thread).
 */
int tredlong_sw_classify(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                             const char* const* suffix, const int32_t* max_units, const uint32_t* packed,
                             const int64_t* read_off, const int32_t* read_len, int64_t n_reads, const int32_t* read_ladder,
                             const tredgpu_sw_params* params, uint8_t* out_tag, int16_t* out_h, int16_t* out_score,
                             int16_t* out_dump, int32_t dump_templates);
const char* tredlong_last_error(void);

/*
 * The CIGAR of n_items alignments on the context's stream: tredcigar_sw_cigar's contract (tredcigar.h) -- the reference's
 * banded_sw restated exactly, quirks included; the same arguments, operations, TREDGPU_CIGAR_* statuses and the same
 * out_ops / out_n_ops / zero-fill rules -- for reads of up to TREDGPU_MAX_LONG_READ_LEN bp on templates of up to
 * TREDGPU_MAX_LONG_TEMPLATE_LEN columns; an item beyond those is TREDGPU_CIGAR_TOO_LONG, a ladder beyond them refuses the
 * call (-2).  HOST memory only, like the rest of the long path: copies in, runs, copies out, waits.
 *
 * One wavefront per item with its lanes across a row's band (csrc/sw_cigar_long.hip); at most 256 wavefronts per launch
 * take the items in turn, item k on wavefront k % min(n_items, 256).
 * Workspace: a wavefront owns one byte per cell of the call's largest rectangle (ref_end - ref_begin + 1) x (read_end -
 * read_begin + 1) -- 8.4 MB for 2 048 x 4 095 -- and the launch has fewer wavefronts where 256 of them would exceed 1 GiB.
 * The context keeps it between calls, grow-only, with the ladder table and the staging buffers; tredlong_release frees
 * all of it and what tredlong_sw_classify holds (call it before tredgpu_destroy; calling it again, or before any call,
 * does nothing).
 * Cost: a pass over a band of b columns and r rows is r * ceil(b / 64) steps of one wavefront; the band starts at
 * |refLen - readLen| + 1 and doubles as the reference's does, and the traceback is one lane's walk over at most refLen +
 * readLen cells.  Meant for the minority of reads the short kernels cannot hold.
 * Returns 0, -2 bad arguments, -10 HIP error; the message is in tredlong_last_error() (per thread).
 */
int tredlong_sw_cigar(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                      const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                      const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                      const int16_t* fields, const tredgpu_sw_params* params, int32_t cap, uint32_t* out_ops,
                      int32_t* out_n_ops, int32_t* out_status);
/* launches of tredlong_sw_cigar's kernel on this context since tredlong_cigar_reset_timing and their summed device time */
int tredlong_cigar_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms);
int tredlong_cigar_reset_timing(tredgpu_ctx* ctx);
void tredlong_release(tredgpu_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif
