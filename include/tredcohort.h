/* tredcohort.h -- cohort allele frequencies by EM and population-aware calls on the GPU (libtredgpu.so, gfx950), under a
 * prefix of its own as tredlong.h, tredcigar.h, tredsecond.h, tredpileup.h and tredtrio.h are (tredgpu.h is the ABI of the
 * kernels the profiles under profiles/ were taken from).
 *
 * tredtrio_evaluate couples the members of one family; tredcohort_evaluate couples all samples of a locus.  One ITEM is one
 * locus with its samples, a sample is a pair list {a <= b, lw} as tredtrio.h defines it and a ploidy.  The allele frequencies
 * of the item are estimated from the samples' (h1, h2) surfaces by EM, fed back to every sample as a Hardy-Weinberg prior,
 * and every sample gets its posterior over its pairs and its cohort-aware call.  The model is the project's own (DESIGN.md 4,
 * "Cohort frequencies").
 *
 * Opt-in: nothing else in libtredgpu calls it (Engine.cohort, python -m tredparse_amd.cohort, tred.py --cohort).
 */
#ifndef TREDCOHORT_H
#define TREDCOHORT_H

#include "tredgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TREDGPU_COHORT_OK 0
#define TREDGPU_COHORT_EMPTY 1      /* no sample of the item has a pair: nothing to estimate */
#define TREDGPU_COHORT_TOO_LONG 4   /* an allele above TREDGPU_COHORT_MAX_ALLELE (the values of TREDGPU_TRIO_TOO_LONG / _BAD_ITEM) */
#define TREDGPU_COHORT_BAD_ITEM 5   /* a > b, a negative allele, an lw that is not finite or is positive, a ploidy other than 1
                                       or 2 (of any sample of the item, one without a pair included), a != b in a ploidy-1 list */

#define TREDGPU_COHORT_MAX_ALLELE 1024  /* the largest allele of any list, in repeat units: a support has 1 025 alleles at the most */
#define TREDGPU_COHORT_MAX_ITERS 4096
#ifndef TREDGPU_COHORT_CHUNK
#define TREDGPU_COHORT_CHUNK 1024       /* incidence entries of an allele one wavefront sums in the M-step (csrc/cohort.hip) */
#endif
#define TREDGPU_COHORT_LONG_LIST 1024   /* a sample of more pairs has a workgroup to itself, any other a wavefront (csrc/cohort.hip) */
#define TREDGPU_KERNEL_COHORT 21        /* the timing selector of the binding (tredtrio.h has 20) */

/* the number of EM iterations (1 .. TREDGPU_COHORT_MAX_ITERS) and the pseudo-chromosomes spread evenly over the support
   (alpha > 0, finite) */
typedef struct tredcohort_params {
    int32_t iters;
    double alpha;
} tredcohort_params;

/*
 * n_items items on the context's stream.  HOST memory only: copies in, runs, copies out, waits.
 *   item_off[n_items + 1]      item i has the samples [item_off[i], item_off[i + 1]); n_samples = item_off[n_items]
 *   sample_off[n_samples + 1], a, b, lw     sample s has the pairs [sample_off[s], sample_off[s + 1]): a <= b the alleles of
 *                      a pair in repeat units, lw <= 0 its log weight.  A sample without a pair takes no part.  Both offset
 *                      arrays begin at 0 and do not descend; the pairs of a call number INT32_MAX at the most
 *   ploidy[n_samples]  1 or 2; the pairs of a ploidy-1 sample have a == b
 *   allele_off[n_items + 1]    the room of item i in out_alleles, out_freq and out_count, sized by the caller: at least the
 *                      number of distinct alleles of the item's lists that lie in 0 .. MAX_ALLELE, for which
 *                      min(MAX_ALLELE + 1, twice the item's pairs) is always enough
 *   out_status[n_items]        TREDGPU_COHORT_*
 *   out_n_alleles[n_items]     A, the size of the support
 *   out_alleles, out_freq, out_count   [allele_off[n_items]]: the first A entries of the item's room are the support,
 *                      ascending, f after the last iteration, and n of the final E-step; the rest of the room is zero
 *   out_trace[n_items][iters][2]       per iteration t: sum_s logZ_s under f_{t-1}, and max_c |f_t(c) - f_{t-1}(c)|
 *   out_sample_call[n_samples][3]      the cohort-aware call: its index in the sample's list, its a, its b
 *   out_sample_values[n_samples][2]    logZ, post
 *   out_r                              parallel to the pairs: r of the final E-step
 * The support is the distinct alleles of the participating lists, ascending, A their count; C the sum of the participating
 * samples' ploidies; m_s = max lw of sample s (it need not be 0), w_k = exp(lw_k - m_s).  Given frequencies f:
 *   diploid  q_k = w_k f(a) f(b) (2 if a != b, else 1);   ploidy 1  q_k = w_k f(a);
 *   Z_s = sum_k q_k,  r_k = q_k / Z_s,  logZ_s = m_s + log Z_s.
 * f_0 = 1 / A; for t = 1 .. iters:  n(c) = sum_s sum_k r_k ([a_k = c] + [b_k = c]) under f_{t-1} (a ploidy-1 pair counts
 * once),  f_t(c) = (n(c) + alpha / A) / (C + alpha).  EXACTLY iters iterations: there is no early stop, and whether the
 * run converged is for the caller to say from the trace.  A last E-step under f_iters gives every sample its r, its logZ, its
 * call -- the largest q, then the smallest a, then the first in the list -- and post, the call's r; out_count is that
 * E-step's n.  alpha > 0 and the largest w of a list is 1, so Z_s > 0: there is no degenerate status.
 * An item is validated completely before anything is computed from it, and no index derived from an item is used before the
 * check that bounds it.  Statuses, in this order of precedence: BAD_ITEM, TOO_LONG, EMPTY.  Every output of such an item is
 * zero, its samples' outputs included, and the other items are unaffected; so are the outputs of a sample without a pair.
 * Every sum has an order fixed by positions inside the item alone (the sample, the pair, a before b): the result of an item
 * does not depend on the items around it or on their order, and a call repeated gives the same bits.  No floating-point
 * atomic is used.  All iterations are queued on the context's stream without a host round trip between them.
 * Returns 0, -2 bad arguments (a NULL array, parameters out of range, offsets that descend or do not begin at 0, more pairs
 * than INT32_MAX, an item with less room than it has alleles: nothing is written then), -10 HIP error;
 * tredcohort_last_error() has the text (per thread).  tredcohort_release frees what the calls on a context hold (staging
 * buffers, timing events): call it before tredgpu_destroy; calling it again, or before any call, does nothing.
 */
int tredcohort_evaluate(tredgpu_ctx* ctx, const tredcohort_params* params, int64_t n_items, const int64_t* item_off,
                        const int64_t* sample_off, const int32_t* a, const int32_t* b, const double* lw, const int32_t* ploidy,
                        const int64_t* allele_off, int32_t* out_status, int32_t* out_n_alleles, int32_t* out_alleles,
                        double* out_freq, double* out_count, double* out_trace, int32_t* out_sample_call,
                        double* out_sample_values, double* out_r);
/* calls of tredcohort_evaluate on this context since tredcohort_reset_timing and the summed device time of their kernels
   (HIP events, one pair around the launches of a call) */
int tredcohort_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms);
int tredcohort_reset_timing(tredgpu_ctx* ctx);
void tredcohort_release(tredgpu_ctx* ctx);
const char* tredcohort_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
