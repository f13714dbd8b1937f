/* tredtrio.h -- trio-aware calls and de novo expansion odds on the GPU (libtredgpu.so, gfx950), under a prefix of its own
 * as tredlong.h, tredcigar.h, tredsecond.h and tredpileup.h are (tredgpu.h is the ABI of the kernels the profiles under
 * profiles/ were taken from).
 *
 * Every other entry of the library describes ONE sample.  tredtrio_evaluate couples the (h1, h2) surfaces of a child and
 * its two parents at one locus through a transmission kernel: which pair of the child's list is the best call given what
 * the parents could have passed on, how sure that call is, how likely it is that an allele changed on the way (de novo),
 * and whether the larger allele came from the father.  The model is the project's own ("Trio evaluation").
 *
 * Opt-in: nothing else in libtredgpu calls it (Engine.trio, python -m tredparse_amd.trio, tred.py --pedigree).
 */
#ifndef TREDTRIO_H
#define TREDTRIO_H

#include "tredgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TREDGPU_TRIO_OK 0
#define TREDGPU_TRIO_EMPTY_CHILD 1  /* the child's list has no pair: nothing to call */
#define TREDGPU_TRIO_DEGENERATE 2   /* sum_k w_k t_k is 0 or not finite: call, Jmax, S and J stand, denovo and paternal are 0 */
#define TREDGPU_TRIO_TOO_LONG 4     /* an allele above TREDGPU_TRIO_MAX_ALLELE (the values of TREDGPU_PILEUP_TOO_LONG / _BAD_ITEM) */
#define TREDGPU_TRIO_BAD_ITEM 5     /* a > b, a negative allele, an lw that is not finite or is positive, ploidy not 1 or 2 */

#define TREDGPU_TRIO_MAX_ALLELE 1024    /* the largest allele of any list, in repeat units */
#define TREDGPU_TRIO_PAIR_CHUNK 1024    /* pairs of a parent's list staged in LDS at a time (csrc/trio.hip) */
#define TREDGPU_TRIO_GAMETE_TILE 64     /* distinct child alleles of one gamete workgroup, one per lane of a wavefront */
#define TREDGPU_KERNEL_TRIO 20          /* the timing selector of the binding (tredpileup.h has 19) */

/* probability that a transmission changes the allele (0 < mu < 1), geometric ratio of the step size (0 < rho < 1), share
   of the changes that are expansions (0 <= beta <= 1) */
typedef struct tredtrio_params {
    double mu, rho, beta;
} tredtrio_params;

/*
 * n_items (trio, locus) items on the context's stream.  HOST memory only: copies in, runs, copies out, waits.
 *   child_off[n_items + 1], child_a, child_b, child_lw     the child's pair lists, CSR: item i has the pairs
 *                      [child_off[i], child_off[i + 1]); a <= b are the alleles of a pair in repeat units, lw <= 0 its log
 *                      weight (log-likelihood minus the list's maximum).  child_off[0] is 0 and the offsets do not descend
 *   father_*, mother_* the parents' lists, the same way
 *   ploidy[n_items]    the CHILD's ploidy, 1 or 2.  A ploidy-1 child (a son at an X-linked locus) ignores the father
 *   father_informative[n_items], mother_informative[n_items]   0: the parent says nothing (absent, not called): its list is
 *                      not looked at and its gamete tables are 1.  A parent with an empty list is uninformative whatever
 *                      its flag says.  A ploidy-1 parent has a == b in every pair and needs nothing else
 *   out_status[n_items]     TREDGPU_TRIO_*
 *   out_call[n_items][3]    the called pair: its index in the child's list, its a, its b
 *   out_values[n_items][4]  Jmax, S, denovo, paternal
 *   out_J                   [child_off[n_items]], parallel to the child's lists: J of every pair
 * With T(c | p) the transmission table -- 1 - mu for c == p, mu beta step(c - p) above, mu (1 - beta) step(p - c) below,
 * step(1) = 1 - rho, step(d + 1) = step(d) rho, built in that order --, T0(c | p) = (1 - mu) [c == p], w_k = exp(lw_k) and
 * for parent X  g_X(c) = sum_k w_k (0.5 T(c | a_k) + 0.5 T(c | b_k)) / sum_k w_k  (g0_X with T0):
 *   child pair k = (x, y):  t = gF(x) gM(y) + [x != y] gF(y) gM(x), t0 the same of g0, pat = gF(y) gM(x) for x != y and
 *                      0.5 t for x == y;  ploidy 1: t = gM(x), t0 = g0M(x), pat = 0
 *   J_k = lw_k + log(max(t_k, e^-100));  the call is the pair of the largest J, then the smallest x, then the first in the
 *   list;  Jmax its J;  S = sum_k exp(J_k - Jmax) (the call's posterior is 1 / S);
 *   denovo = 1 - sum_k w_k t0_k / sum_k w_k t_k;  paternal = sum_k w_k pat_k / sum_k w_k t_k.
 * An item is validated completely before anything is computed from it, and no index derived from an item is used before the
 * check that bounds it.  Statuses, in this order of precedence: BAD_ITEM (in the child's list or in the list of an
 * informative parent, or the ploidy), TOO_LONG (the same lists), EMPTY_CHILD; DEGENERATE after the evaluation.  The outputs
 * of a BAD_ITEM, TOO_LONG or EMPTY_CHILD item are zero, its J included, and the other items are unaffected.
 * Every sum has a fixed order that depends on the position of a pair in its list alone: the result of an item does not
 * depend on the items around it, and a call repeated gives the same bits.  No floating-point atomic is used.
 * Returns 0, -2 bad arguments (a NULL array, parameters out of range, offsets that descend or do not begin at 0: nothing is
 * written then), -10 HIP error; tredtrio_last_error() has the text (per thread).  tredtrio_release frees what the calls on a
 * context hold (staging buffers, timing events): call it before tredgpu_destroy; calling it again, or before any call, does
 * nothing.
 */
int tredtrio_evaluate(tredgpu_ctx* ctx, const tredtrio_params* params, int64_t n_items,
                      const int64_t* child_off, const int32_t* child_a, const int32_t* child_b, const double* child_lw,
                      const int64_t* father_off, const int32_t* father_a, const int32_t* father_b, const double* father_lw,
                      const int64_t* mother_off, const int32_t* mother_a, const int32_t* mother_b, const double* mother_lw,
                      const int32_t* ploidy, const int32_t* father_informative, const int32_t* mother_informative,
                      int32_t* out_status, int32_t* out_call, double* out_values, double* out_J);
/* calls of tredtrio_evaluate on this context since tredtrio_reset_timing and the summed device time of their kernels (HIP
   events, one pair around the launches of a call) */
int tredtrio_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms);
int tredtrio_reset_timing(tredgpu_ctx* ctx);
void tredtrio_release(tredgpu_ctx* ctx);
const char* tredtrio_last_error(void);

#ifdef __cplusplus
}
#endif

#endif
