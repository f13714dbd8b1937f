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
 * Waits for the results.  Cost beyond the kernel: every call allocates and frees its device buffers and copies from
 * the caller's pageable arrays (a few hundred microseconds per call) -- meant for the minority of reads the short
 * kernels cannot hold; a sample whose reads are all longer than TREDGPU_MAX_READ_LEN sends all of them here.  Returns 0, -2 bad arguments, -5 a read beyond TREDGPU_MAX_LONG_READ_LEN, -10 HIP error;
 * the message is in tredlong_last_error() (per thread).
 */
int tredlong_sw_classify(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                             const char* const* suffix, const int32_t* max_units, const uint32_t* packed,
                             const int64_t* read_off, const int32_t* read_len, int64_t n_reads, const int32_t* read_ladder,
                             const tredgpu_sw_params* params, uint8_t* out_tag, int16_t* out_h, int16_t* out_score,
                             int16_t* out_dump, int32_t dump_templates);
const char* tredlong_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
