/* tredpileup.h -- per-allele evidence from per-read alignments, on the GPU (libtredgpu.so, gfx950), under a prefix of
 * its own as tredlong.h, tredcigar.h and tredsecond.h are (tredgpu.h is the ABI of the kernels the profiles under
 * profiles/ were taken from).
 *
 * tredcigar_sw_cigar says how ONE read lies on the template it was counted for.  tredpileup_pileup adds the reads of a
 * group -- the reads counted for one allele of one locus -- up, column by column of that allele's FORWARD template: which
 * letter each read shows there, whether it skips the column, and what it inserts before it.  That table is what a
 * consensus of the tract, and so an interruption of it (CAA in HTT, AGG in FMR1), is read from.
 *
 * tredpileup_pileup_anchored does the same for an allele LONGER than its reads, which no read spans: a read that begins in
 * one flank and ends inside the tract is laid on the allele's template from the side of that flank.
 *
 * Opt-in: nothing else in libtredgpu calls them (Engine.consensus, tred.py --consensus / --consensus-partial).
 */
#ifndef TREDPILEUP_H
#define TREDPILEUP_H

#include "tredgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TREDGPU_PILEUP_OK 0
#define TREDGPU_PILEUP_TOO_LONG 4  /* read beyond TREDGPU_MAX_LONG_READ_LEN or template beyond TREDGPU_MAX_LONG_TEMPLATE_LEN
                                      (tredlong.h); the values are those of TREDGPU_CIGAR_TOO_LONG / _BAD_ITEM */
#define TREDGPU_PILEUP_BAD_ITEM 5  /* ladder, template or group index out of range; fields outside the pair; n_ops < 1 or
                                      > cap; an operation other than M / I / D or of length 0; M + D lengths that are not
                                      ref_end - ref_begin + 1 or M + I lengths that are not read_end - read_begin + 1; a
                                      (ladder, units) other than that of the group's first accepted item */

#define TREDGPU_PILEUP_ANCHOR_WHOLE 0  /* item_anchor of tredpileup_pileup_anchored: the item spans the group's allele */
#define TREDGPU_PILEUP_ANCHOR_BEGIN 1  /* it lies at the begin of its OWN template (a read tagged PREF) */
#define TREDGPU_PILEUP_ANCHOR_END 2    /* ... at the end of its own template (POST) */

#define TREDGPU_PILEUP_CHANNELS 8
#define TREDGPU_PILEUP_MAX_STRIDE 65536
#define TREDGPU_KERNEL_PILEUP 19   /* the timing selector of the binding (tredsecond.h has 18) */

/*
 * The pileup of n_items alignments in n_groups groups on the context's stream.  HOST memory only: copies in, runs, copies
 * out, waits.
 *   n_ladders, prefix, repeat, suffix, max_units, packed, read_off, read_len, item_ladder, item_template, fields
 *                      the items, exactly as tredcigar_sw_cigar takes them (item_template in db order: u=1 fwd, u=1 rc,
 *                      u=2 fwd, ...; 0 for a plain reference); the scoring is not needed
 *   ops                uint32 [n_items][cap] and n_ops[n_items]: that call's out_ops / out_n_ops (length << 4 | op, M=0 I=1
 *                      D=2, oldest first)
 *   item_group[n_items], n_groups   the group of every item.  All items of a group name the same ladder and the same
 *                      units (item_template / 2), strands mixed freely; the group takes its shape from its first accepted
 *                      item, in the caller's order
 *   stride             columns of a group's table: at least the largest template length of the ladders (as far as an item
 *                      can be accepted: TREDGPU_MAX_LONG_TEMPLATE_LEN at the most) + 1, at most TREDGPU_PILEUP_MAX_STRIDE
 *   out_counts         int32 [n_groups][stride][8], written whole (a group without an accepted item is all zeros).  Column
 *                      c is column c of the FORWARD template of the group's (ladder, units), whichever strand an item lies
 *                      on.  Channels 0-3: reads showing A, C, G, T at the column under an M operation; 4: N; 5: reads
 *                      whose D operation covers the column; 6: insertions that sit immediately before the column (events);
 *                      7: their summed length.  Slot L (the template's length) takes an insertion behind the last column.
 *                      An item on a reverse-complement template of length L (odd item_template, max_units > 0) counts
 *                      its column c at L - 1 - c, its letter complemented (N stays N), and an insertion before c before
 *                      L - c.  Soft-clipped read ends count nowhere.
 *   out_status[n_items] (TREDGPU_PILEUP_*).  An item is validated completely before it counts anything, a refused item
 *                      counts nothing, and no index derived from an item is used before it is checked.
 * Every cell of out_counts is owned by one workgroup, which adds in LDS and stores once: the result is exact and does not
 * depend on the order of the items (csrc/pileup.hip).
 * Returns 0, -2 bad arguments (stride too small included: nothing is written then), -10 HIP error;
 * tredpileup_last_error() has the text (per thread).  tredpileup_release frees what the calls on a context hold (ladder
 * table, staging buffers, timing events): call it before tredgpu_destroy; calling it again, or before any call, does
 * nothing.
 */
int tredpileup_pileup(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                      const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                      const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                      const int16_t* fields, const uint32_t* ops, int32_t cap, const int32_t* n_ops, const int32_t* item_group,
                      int32_t n_groups, int32_t stride, int32_t* out_counts, int32_t* out_status);
/*
 * The same pileup with the shape of every group GIVEN and an anchor per item, for alleles longer than the reads.  The
 * arguments of tredpileup_pileup, and
 *   item_anchor[n_items]   TREDGPU_PILEUP_ANCHOR_*
 *   group_ladder[n_groups], group_units[n_groups]   the group's ladder and its allele a >= 1, which MAY exceed the
 *                      ladder's max_units: the group's template is prefix + repeat * a + suffix, of T_a columns
 *   stride             at least the largest GROUP template length + 1, at most TREDGPU_PILEUP_MAX_STRIDE; the ladders' own
 *                      templates do not bound it
 * With P, p, S the lengths of prefix, repeat and suffix, an item of template index tpl has h = tpl / 2 + 1 units, strand
 * tpl & 1 and T_h = P + p * h + S columns of its own.  Its forward column and forward slot on its OWN template are what
 * tredpileup_pileup counts: c or T_h - 1 - c, slot r or T_h - r.
 * Refused with TREDGPU_PILEUP_BAD_ITEM, besides everything tredpileup_pileup refuses (those checks come first, TOO_LONG
 * among them): item_ladder other than group_ladder[group]; a ladder with max_units <= 0 (a plain reference has no tract to
 * anchor on); an anchor outside 0..2; h > a; anchor WHOLE with h != a.  Every refusal is the item's own: the group has its
 * shape whether or not an item is accepted.
 * Counting.  h == a: the item counts whole, as in tredpileup_pileup, whatever its anchor.  Otherwise its forward side is
 * LEFT when (anchor == BEGIN) != (strand == 1), else RIGHT -- tags are decided on the template aligned to, so a PREF read
 * on a reverse-complement template sits at the suffix end of the forward one.
 *   LEFT   keeps forward columns f < P + p * h and forward slots s < P + p * h (slot 0 included), where they are
 *   RIGHT  keeps forward columns f >= P and forward slots P < s <= T_h, moved up by (a - h) * p
 * What the item shows of the other flank -- columns that would lie inside the group's tract -- is cut, the slot at the
 * cut is dropped, and an M, D or I operation across the cut counts on the kept side only.
 * Returns as tredpileup_pileup; -2 (nothing written) also for a NULL array, a group_ladder out of range, a group_units
 * below 1 and a stride below the largest group template + 1.  Host memory only; the same state, stream and staging.
 */
int tredpileup_pileup_anchored(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                               const char* const* suffix, const int32_t* max_units, const uint32_t* packed,
                               const int64_t* read_off, const int32_t* read_len, int64_t n_items, const int32_t* item_ladder,
                               const int32_t* item_template, const int16_t* fields, const uint32_t* ops, int32_t cap,
                               const int32_t* n_ops, const int32_t* item_group, const int32_t* item_anchor, int32_t n_groups,
                               const int32_t* group_ladder, const int32_t* group_units, int32_t stride, int32_t* out_counts,
                               int32_t* out_status);
/*
 * The repeat-unit spectrum of the same items: per group which repeat-unit words (CAG, CAA, CCG, ...) its items show and how
 * often, per item how many of its units are not the motif.  Position-free, so it takes every tagged read, the in-repeat
 * ones included, which no pileup can place.  The items as tredpileup_pileup takes them, and
 *   group_ladder[n_groups]   the group's ladder: the shape of a group is given, so every refusal is the item's own
 * Counting.  With P, p, S the lengths of prefix, repeat and suffix, an item of template index tpl has h = tpl / 2 + 1
 * units, strand tpl & 1 and T_h = P + p * h + S columns.  Its own column c is forward column c on strand 0 and T_h - 1 - c
 * on strand 1, and a read letter counts as itself on strand 0 and complemented on strand 1 (N stays N), as in
 * tredpileup_pileup.  Tract unit k (0 <= k < h) is the forward columns [P + p * k, P + p * (k + 1)).  A unit is CLEAN for
 * an item iff all its p forward columns lie inside ONE M operation of the item: a unit cut by an I, a D, a soft clip or the
 * end of the alignment is not clean; an I exactly on a unit boundary leaves both neighbours clean.  The unit's WORD is the p
 * read letters on those columns in forward order (on strand 1 the read is walked backwards and complemented).  A word with
 * an N adds 1 to with_n; any other adds 1 to bin code = sum letter_i * 4^(p - 1 - i), A 0 C 1 G 2 T 3.  A unit is TOUCHED
 * if at least one of its columns lies in the item's forward span ref_begin .. ref_end, D columns included.
 *   out_spectrum       int32 [n_groups][TREDGPU_SPECTRUM_STRIDE], written whole: bins 0 .. 4^p - 1 (zero above), then at
 *                      TREDGPU_SPECTRUM_BINS + 0 the clean units (N-free words plus with_n), + 1 with_n, + 2 the touched
 *                      units, + 3 the accepted items
 *   out_item           int32 [n_items][3]: the item's N-free clean units, how many of them equal the ladder's repeat, and
 *                      its touched units; zeros for a refused item
 *   out_status[n_items]
 * Refused per item: everything tredpileup_pileup refuses on an item of its own (TOO_LONG, then BAD_ITEM); BAD_ITEM for
 * item_ladder other than group_ladder[group] and for a ladder without a tract (max_units <= 0); TREDGPU_PILEUP_PERIOD for a
 * period above TREDGPU_SPECTRUM_MAX_PERIOD (the table has 4^p bins).
 * Every row is owned by one workgroup, which adds in LDS and stores once: exact, and independent of the order of the items.
 * Returns as tredpileup_pileup; -2 (nothing written) also for a NULL array, a group_ladder out of range and n_groups < 0.
 * Host memory only; the same state, stream and staging, and tredpileup_get_timing counts its calls too.
 */
#define TREDGPU_PILEUP_PERIOD 6         /* out_status of tredpileup_unit_spectrum: the ladder's period has no table */
#define TREDGPU_SPECTRUM_MAX_PERIOD 6
#define TREDGPU_SPECTRUM_BINS 4096      /* 4^TREDGPU_SPECTRUM_MAX_PERIOD */
#define TREDGPU_SPECTRUM_STRIDE 4100    /* the bins, then clean, with_n, touched, accepted items */
int tredpileup_unit_spectrum(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                             const char* const* suffix, const int32_t* max_units, const uint32_t* packed,
                             const int64_t* read_off, const int32_t* read_len, int64_t n_items, const int32_t* item_ladder,
                             const int32_t* item_template, const int16_t* fields, const uint32_t* ops, int32_t cap,
                             const int32_t* n_ops, const int32_t* item_group, int32_t n_groups, const int32_t* group_ladder,
                             int32_t* out_spectrum, int32_t* out_item, int32_t* out_status);
/* calls of the three entries above on this context since tredpileup_reset_timing and the summed device time of their kernels
   (HIP events, one pair around the launches of a call) */
int tredpileup_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms);
int tredpileup_reset_timing(tredgpu_ctx* ctx);
void tredpileup_release(tredgpu_ctx* ctx);
const char* tredpileup_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
