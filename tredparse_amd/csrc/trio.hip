// trio.hip -- trio-aware calls and de novo expansion odds (tredtrio_evaluate, include/tredtrio.h): per (trio, locus) item
// the pair lists {a, b, lw} of a child and its two parents, coupled through a transmission table.  A unit of its own,
// outside the source hash the profiles are tied to (csrc/Makefile); the harness is side_unit.h's.
//
// Three kernels per call.
//   * trio_prepare_kernel, one workgroup per item: every refusal of the header (the ploidy, the child's list, the lists of
//     the informative parents) -> pre[item], and the item's DISTINCT child alleles, ascending, into dist (a presence flag per
//     allele in LDS, a workgroup-wide exclusive scan over the flags).  The later kernels only ever look at items with
//     pre == OK, whose alleles all lie in 0 .. MAX_ALLELE: no index derived from an item is used before that.
//   * trio_gamete_kernel, one workgroup of four wavefronts per (item, parent, tile of 64 distinct child alleles); the work
//     units are taken grid-stride (woff: how many tiles each item has room for).  Lane l of every wavefront owns allele
//     tile0 + l.  The parent's pairs are streamed through LDS PAIR_CHUNK at a time -- a, b and w = exp(lw), the exponential
//     taken once per pair and tile --, wavefront v takes the v-th quarter of every chunk, and a lane adds
//     w (0.5 T(c | a) + 0.5 T(c | b)) into g, the same of T0 into g0, and w into W in the same loop.  a, b and w are the same
//     address in all lanes (an LDS broadcast); T comes from the table of 2 MAX_ALLELE + 1 doubles in LDS, at c - p, which
//     differs from lane to lane as the alleles do.  The four partial sums are added as (0 + 1) + (2 + 3): the order of every
//     sum is fixed by the position of a pair in its list.
//   * trio_child_kernel, one workgroup per item: the rank of an allele in dist from a table in LDS, lanes stride over the
//     child's pairs; pass 1 writes J and reduces the call (largest J, then smallest x, then first) and the three sums
//     sum w t, sum w t0, sum w pat; pass 2 reads the lane's own J back and sums exp(J - Jmax).  Per-lane strided partial sums,
//     a butterfly over the wavefront, (0 + 1) + (2 + 3) over the wavefronts.
// All results leave through plain vector stores; there is no global atomic.
#include <climits>
#include <cmath>
#include <cstring>

#include "side_unit.h"
#include "../../include/tredtrio.h"

namespace {
using namespace side_unit;

thread_local std::string g_trio_error;     // the text of tredtrio_last_error()

constexpr int CAP = TREDGPU_TRIO_MAX_ALLELE, NALLELE = CAP + 1, TABLE = 2 * CAP + 1;
constexpr int CHUNK = TREDGPU_TRIO_PAIR_CHUNK, TILE = TREDGPU_TRIO_GAMETE_TILE;
constexpr int THREADS = 256, WAVES = THREADS / 64, QUARTER = CHUNK / WAVES;
constexpr int PER = (NALLELE + THREADS - 1) / THREADS;     // alleles of a thread in the scan of the presence flags
constexpr int MAX_BLOCKS = 1 << 16;                        // workgroups of a launch at the most (the loops are grid-stride)
static_assert(TILE == 64 && WAVES == 4 && CHUNK % WAVES == 0, "a tile is one wavefront wide, a chunk has four quarters");

struct List {
    const int64_t* off;
    const int32_t *a, *b;
    const double* lw;
};

struct TrioArgs {
    List child, parent[2];                 // father, mother
    const int32_t* ploidy;
    const int32_t* informative[2];
    const double* table;                   // [TABLE]: T(c | p) at c - p + CAP
    const int64_t* doff;                   // [n_items + 1]: where an item's distinct alleles and gamete tables begin
    const int64_t* woff;                   // [n_items + 1]: tiles of 64 alleles an item has room for, summed
    int32_t *pre, *nd, *dist;              // status of the prepare kernel, distinct alleles of an item and the alleles
    double* gam;                           // [doff[n_items]][4]: gF, g0F, gM, g0M of every distinct allele
    int32_t *out_status, *out_call;
    double *out_values, *out_J;
    int64_t n_items;
    double one_minus_mu, floor;
};

// the refusals of one list, by the lanes of a workgroup; mark: the alleles of an acceptable pair are flagged
__device__ __forceinline__ void check_list(const List& l, int64_t item, bool mark, int* flags, int& bad, int& too_long) {
    const int64_t hi = l.off[item + 1];
    for (int64_t k = l.off[item] + threadIdx.x; k < hi; k += THREADS) {
        const int x = l.a[k], y = l.b[k];
        const double lw = l.lw[k];
        if (x < 0 || y < 0 || x > y || !(lw <= 0.0) || !isfinite(lw)) bad = 1;
        else if (y > CAP) too_long = 1;
        else if (mark) { flags[x] = 1; flags[y] = 1; }             // (the same value from whoever stores it)
    }
}

__global__ __launch_bounds__(THREADS) void trio_prepare_kernel(TrioArgs a) {
    __shared__ int flags[NALLELE];
    __shared__ int wave_sum[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        __syncthreads();                                           // the item before is done with flags and wave_sum
        for (int k = threadIdx.x; k < NALLELE; k += THREADS) flags[k] = 0;
        __syncthreads();
        const int pl = a.ploidy[item];
        int bad = (pl != 1 && pl != 2) ? 1 : 0, too_long = 0;
        check_list(a.child, item, true, flags, bad, too_long);
        for (int p = 0; p < 2; ++p)
            if (a.informative[p][item] != 0) check_list(a.parent[p], item, false, flags, bad, too_long);
        bad = __syncthreads_or(bad);
        too_long = __syncthreads_or(too_long);
        const bool empty = a.child.off[item + 1] == a.child.off[item];
        const int status = bad ? TREDGPU_TRIO_BAD_ITEM : too_long ? TREDGPU_TRIO_TOO_LONG : empty ? TREDGPU_TRIO_EMPTY_CHILD
                                                                                                : TREDGPU_TRIO_OK;
        // the flagged alleles in ascending order: thread t has the alleles [t PER, (t + 1) PER)
        int mine = 0;
        if (status == TREDGPU_TRIO_OK)
            for (int j = 0; j < PER; ++j) {
                const int al = threadIdx.x * PER + j;
                if (al < NALLELE && flags[al]) mine += 1;
            }
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, (unsigned)d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int v = 0; v < WAVES; ++v) {
            if (v < wave) before += wave_sum[v];
            total += wave_sum[v];
        }
        if (mine) {                                                // (status is OK: total <= min(2 pairs, NALLELE), dist's room)
            int32_t* out = a.dist + a.doff[item] + before + incl - mine;
            for (int j = 0; j < PER; ++j) {
                const int al = threadIdx.x * PER + j;
                if (al < NALLELE && flags[al]) *out++ = al;
            }
        }
        if (threadIdx.x == 0) {
            a.pre[item] = status;
            a.nd[item] = total;
        }
    }
}

__global__ __launch_bounds__(THREADS) void trio_gamete_kernel(TrioArgs a) {
    __shared__ double table[TABLE];
    __shared__ int ca[CHUNK], cb[CHUNK];
    __shared__ double cw[CHUNK];
    __shared__ double part[WAVES][3][TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < TABLE; k += THREADS) table[k] = a.table[k];
    const int64_t n_work = 2 * a.woff[a.n_items];
    for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int p = (int)(w & 1);
        const int64_t q = w >> 1;
        int64_t item = 0, hi = a.n_items;                          // the last item with woff[item] <= q: woff[hi] > q
        while (hi - item > 1) {
            const int64_t mid = (item + hi) >> 1;
            if (a.woff[mid] <= q) item = mid; else hi = mid;
        }
        if (a.pre[item] != TREDGPU_TRIO_OK) continue;              // (the same in every lane of the workgroup)
        const int tile0 = (int)(q - a.woff[item]) * TILE, nd = a.nd[item];
        if (tile0 >= nd) continue;
        const List& l = a.parent[p];
        const int64_t plo = l.off[item], phi = l.off[item + 1];
        const int j = tile0 + lane;
        double* out = a.gam + (a.doff[item] + j) * 4 + p * 2;
        // a parent that says nothing: no flag, no pair, or the father of a ploidy-1 child
        if (a.informative[p][item] == 0 || phi == plo || (p == 0 && a.ploidy[item] == 1)) {
            if (wave == 0 && j < nd) { out[0] = 1.0; out[1] = 1.0; }
            continue;
        }
        const int c = j < nd ? a.dist[a.doff[item] + j] : 0;       // (a lane beyond the list works on allele 0 and stores nothing)
        double g = 0.0, g0 = 0.0, W = 0.0;
        for (int64_t base = plo; base < phi; base += CHUNK) {
            const int m = (int)(phi - base < CHUNK ? phi - base : CHUNK);
            __syncthreads();                                       // the chunk before has been read (and the table is in)
            for (int k = threadIdx.x; k < m; k += THREADS) {
                ca[k] = l.a[base + k];
                cb[k] = l.b[base + k];
                cw[k] = exp(l.lw[base + k]);
            }
            __syncthreads();
            const int k1 = min(m, (wave + 1) * QUARTER);
            // (unrolled: the LDS reads and the products of eight pairs are in flight together, the adds keep their order)
#pragma unroll 8
            for (int k = wave * QUARTER; k < k1; ++k) {
                const int pa = ca[k], pb = cb[k];                  // 0 .. CAP, as c is: c - p + CAP is 0 .. 2 CAP
                const double wk = cw[k];
                const double t = 0.5 * table[c - pa + CAP] + 0.5 * table[c - pb + CAP];
                const double t0 = 0.5 * (c == pa ? a.one_minus_mu : 0.0) + 0.5 * (c == pb ? a.one_minus_mu : 0.0);
                g += wk * t;
                g0 += wk * t0;
                W += wk;
            }
        }
        part[wave][0][lane] = g; part[wave][1][lane] = g0; part[wave][2][lane] = W;
        __syncthreads();
        if (wave == 0 && j < nd) {
            double s[3];
            for (int i = 0; i < 3; ++i) s[i] = (part[0][i][lane] + part[1][i][lane]) + (part[2][i][lane] + part[3][i][lane]);
            out[0] = s[0] / s[2];
            out[1] = s[1] / s[2];
        }
        // (part is written again only behind the two barriers of the next informative unit's first chunk)
    }
}

// the sum of x over the workgroup, in every thread: a butterfly over the wavefront, then (0 + 1) + (2 + 3)
__device__ __forceinline__ double block_sum(double x, double* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    __syncthreads();                                               // red is free
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// candidate calls: the larger J, then the smaller x, then the earlier pair
struct Best { double J; int x; long long k; };
__device__ __forceinline__ bool better(const Best& u, const Best& v) {
    return u.J > v.J || (u.J == v.J && (u.x < v.x || (u.x == v.x && u.k < v.k)));
}

__global__ __launch_bounds__(THREADS) void trio_child_kernel(TrioArgs a) {
    __shared__ int pos[NALLELE];
    __shared__ double red[WAVES];
    __shared__ double bestJ[WAVES];
    __shared__ int bestx[WAVES];
    __shared__ long long bestk[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        __syncthreads();                                           // the item before is done with pos and the best arrays
        const int status = a.pre[item];
        const int64_t lo = a.child.off[item], hi = a.child.off[item + 1];
        if (status != TREDGPU_TRIO_OK) {                           // refused or empty: zeros
            for (int64_t k = lo + threadIdx.x; k < hi; k += THREADS) a.out_J[k] = 0.0;
            if (threadIdx.x == 0) {
                a.out_status[item] = status;
                for (int i = 0; i < 3; ++i) a.out_call[item * 3 + i] = 0;
                for (int i = 0; i < 4; ++i) a.out_values[item * 4 + i] = 0.0;
            }
            continue;
        }
        const int nd = a.nd[item];
        const int32_t* dist = a.dist + a.doff[item];
        for (int j = threadIdx.x; j < nd; j += THREADS) pos[dist[j]] = j;      // (alleles of an accepted item: 0 .. CAP)
        __syncthreads();
        const double* gam = a.gam + a.doff[item] * 4;
        const bool haploid = a.ploidy[item] == 1;
        Best best = {-INFINITY, INT_MAX, LLONG_MAX};
        double A = 0.0, B = 0.0, C = 0.0;
        for (int64_t k = lo + threadIdx.x; k < hi; k += THREADS) {
            const int x = a.child.a[k], y = a.child.b[k];          // both flagged by the prepare kernel: pos has them
            const double lw = a.child.lw[k];
            const double* gx = gam + pos[x] * 4;
            const double* gy = gam + pos[y] * 4;
            double t, t0, pat;
            if (haploid) {
                t = gx[2]; t0 = gx[3]; pat = 0.0;
            } else {
                t = gx[0] * gy[2];
                t0 = gx[1] * gy[3];
                if (x != y) {
                    pat = gy[0] * gx[2];
                    t += pat;
                    t0 += gy[1] * gx[3];
                } else {
                    pat = 0.5 * t;
                }
            }
            const double J = lw + log(fmax(t, a.floor));
            a.out_J[k] = J;
            const double w = exp(lw);
            A += w * t; B += w * t0; C += w * pat;
            const Best cand = {J, x, (long long)(k - lo)};
            if (better(cand, best)) best = cand;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const Best o = {__shfl_xor(best.J, d, 64), __shfl_xor(best.x, d, 64), __shfl_xor(best.k, d, 64)};
            if (better(o, best)) best = o;
        }
        if (lane == 0) { bestJ[wave] = best.J; bestx[wave] = best.x; bestk[wave] = best.k; }
        __syncthreads();
        for (int v = 0; v < WAVES; ++v) {
            const Best o = {bestJ[v], bestx[v], bestk[v]};
            if (better(o, best)) best = o;
        }
        if (best.k == LLONG_MAX) best.k = 0;                       // (no J compared as larger than -inf: none was a number)
        A = block_sum(A, red);
        B = block_sum(B, red);
        C = block_sum(C, red);
        double S = 0.0;
        for (int64_t k = lo + threadIdx.x; k < hi; k += THREADS) S += exp(a.out_J[k] - best.J);     // (the lane's own stores)
        S = block_sum(S, red);
        if (threadIdx.x == 0) {
            const bool degenerate = A == 0.0 || !isfinite(A);
            a.out_status[item] = degenerate ? TREDGPU_TRIO_DEGENERATE : TREDGPU_TRIO_OK;
            a.out_call[item * 3 + 0] = (int32_t)best.k;
            a.out_call[item * 3 + 1] = a.child.a[lo + best.k];
            a.out_call[item * 3 + 2] = a.child.b[lo + best.k];
            a.out_values[item * 4 + 0] = best.J;
            a.out_values[item * 4 + 1] = S;
            a.out_values[item * 4 + 2] = degenerate ? 0.0 : 1.0 - B / A;
            a.out_values[item * 4 + 3] = degenerate ? 0.0 : C / A;
        }
    }
}

struct State : StateBase {};
Registry<State> g_states;

// offsets of a CSR list: they begin at 0 and do not descend
int offsets_refusal(std::string& err, const char* who, const int64_t* off, int64_t n) {
    if (off[0] != 0) return fail(err, -2, "%s_off[0] must be 0", who);
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(err, -2, "%s_off descends at item %lld", who, (long long)i);
    return 0;
}

}  // namespace

extern "C" {

int tredtrio_evaluate(tredgpu_ctx* ctx, const tredtrio_params* params, int64_t n_items,
                      const int64_t* child_off, const int32_t* child_a, const int32_t* child_b, const double* child_lw,
                      const int64_t* father_off, const int32_t* father_a, const int32_t* father_b, const double* father_lw,
                      const int64_t* mother_off, const int32_t* mother_a, const int32_t* mother_b, const double* mother_lw,
                      const int32_t* ploidy, const int32_t* father_informative, const int32_t* mother_informative,
                      int32_t* out_status, int32_t* out_call, double* out_values, double* out_J) {
    std::string& err = g_trio_error;
    err.clear();
    if (!ctx) return fail(err, -2, "ctx is NULL");
    if (!params) return fail(err, -2, "params is NULL");
    const double mu = params->mu, rho = params->rho, beta = params->beta;
    if (!(mu > 0.0 && mu < 1.0) || !(rho > 0.0 && rho < 1.0) || !(beta >= 0.0 && beta <= 1.0))
        return fail(err, -2, "parameters out of range: 0 < mu < 1, 0 < rho < 1, 0 <= beta <= 1 (mu %g, rho %g, beta %g)", mu, rho, beta);
    if (n_items < 0 || n_items > INT32_MAX) return fail(err, -2, "n_items %lld out of range", (long long)n_items);
    if (n_items == 0) return 0;
    if (!child_off || !father_off || !mother_off || !ploidy || !father_informative || !mother_informative || !out_status ||
        !out_call || !out_values)
        return fail(err, -2, "NULL array argument");
    const size_t n = (size_t)n_items;
    int rc;
    if ((rc = offsets_refusal(err, "child", child_off, n_items))) return rc;
    if ((rc = offsets_refusal(err, "father", father_off, n_items))) return rc;
    if ((rc = offsets_refusal(err, "mother", mother_off, n_items))) return rc;
    const size_t nc = (size_t)child_off[n], nf = (size_t)father_off[n], nm = (size_t)mother_off[n];
    if ((nc && (!child_a || !child_b || !child_lw || !out_J)) || (nf && (!father_a || !father_b || !father_lw)) ||
        (nm && (!mother_a || !mother_b || !mother_lw)))
        return fail(err, -2, "NULL array argument");

    // the transmission table, by the recurrence: T(c | p) at c - p + CAP
    std::vector<double> table(TABLE);
    table[CAP] = 1.0 - mu;
    double step = 1.0 - rho;
    for (int d = 1; d <= CAP; ++d) {
        table[CAP + d] = (mu * beta) * step;
        table[CAP - d] = (mu * (1.0 - beta)) * step;
        step = step * rho;
    }
    // room for the distinct alleles of every item -- no more than twice its pairs, nor than there are alleles -- and the
    // tiles of 64 that room makes
    std::vector<int64_t> doff(n + 1, 0), woff(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        const int64_t room = std::min<int64_t>(2 * (child_off[i + 1] - child_off[i]), NALLELE);
        doff[i + 1] = doff[i] + room;
        woff[i + 1] = woff[i] + (room + TILE - 1) / TILE;
    }

    hipStream_t st;
    if ((rc = select_device(err, ctx, st))) return rc;
    State& s = *g_states.state_of(ctx);
    TrioArgs a{};
    const size_t room = (size_t)doff[n];
    std::vector<Array> arrays = {
        arr_in(a.child.off, child_off, n + 1), arr_in(a.child.a, child_a, nc), arr_in(a.child.b, child_b, nc),
        arr_in(a.child.lw, child_lw, nc),
        arr_in(a.parent[0].off, father_off, n + 1), arr_in(a.parent[0].a, father_a, nf), arr_in(a.parent[0].b, father_b, nf),
        arr_in(a.parent[0].lw, father_lw, nf),
        arr_in(a.parent[1].off, mother_off, n + 1), arr_in(a.parent[1].a, mother_a, nm), arr_in(a.parent[1].b, mother_b, nm),
        arr_in(a.parent[1].lw, mother_lw, nm),
        arr_in(a.ploidy, ploidy, n), arr_in(a.informative[0], father_informative, n),
        arr_in(a.informative[1], mother_informative, n),
        arr_in(a.table, (const double*)table.data(), table.size()), arr_in(a.doff, (const int64_t*)doff.data(), doff.size()),
        arr_in(a.woff, (const int64_t*)woff.data(), woff.size()),
        arr_scratch(a.pre, n), arr_scratch(a.nd, n), arr_scratch(a.dist, room), arr_scratch(a.gam, room * 4),
        arr_out(a.out_status, out_status, n), arr_out(a.out_call, out_call, n * 3), arr_out(a.out_values, out_values, n * 4),
        arr_out(a.out_J, out_J, nc)};
    if ((rc = stage(err, s, st, arrays))) return rc;
    a.n_items = n_items;
    a.one_minus_mu = 1.0 - mu;
    a.floor = std::exp(-100.0);

    if ((rc = timed_begin(err, s, st))) return rc;
    const dim3 per_item((unsigned)std::min<int64_t>(n_items, MAX_BLOCKS));
    const dim3 per_tile((unsigned)std::min<int64_t>(2 * woff[n], MAX_BLOCKS));
    hipLaunchKernelGGL(trio_prepare_kernel, per_item, dim3(THREADS), 0, st, a);
    if (woff[n] > 0) hipLaunchKernelGGL(trio_gamete_kernel, per_tile, dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(trio_child_kernel, per_item, dim3(THREADS), 0, st, a);
    if ((rc = timed_end(err, s, st))) return rc;
    return read_back(err, s, st, arrays);      // (table, doff and woff are read by their copies until the stream is drained)
}

int tredtrio_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) { return timing(g_trio_error, g_states, ctx, launches, total_ms, false); }

int tredtrio_reset_timing(tredgpu_ctx* ctx) { return timing(g_trio_error, g_states, ctx, nullptr, nullptr, true); }

void tredtrio_release(tredgpu_ctx* ctx) { release(g_states, ctx, {}); }

const char* tredtrio_last_error(void) { return g_trio_error.c_str(); }

}  // extern "C"
