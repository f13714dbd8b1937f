// cohort.hip -- cohort allele frequencies by EM and population-aware calls (tredcohort_evaluate, include/tredcohort.h): per
// item -- one locus with its samples -- the pair lists {a, b, lw} and the ploidies of the samples.  A unit of its own, outside
// the source hash the profiles are tied to (csrc/Makefile); the harness is side_unit.h's.
//
// The host, while it stages a call, builds the item's INCIDENCE LIST by a stable counting sort: per allele of 0 .. MAX_ALLELE
// that a list of the item names, in ascending order (a SLOT), the pairs that name it -- in the order of the samples and of
// their pairs, a before b, a pair of a ploidy-1 sample once -- and cuts every slot into chunks of CHUNK entries.  It looks at
// no lw and refuses nothing: alleles outside the range get no entry, and the item they belong to is refused by the device.
// Six kernels; the last three run once per iteration, all queued on the context's stream one after the other.  The three
// per-sample kernels give a sample of more than LONG_LIST pairs a workgroup and any other a wavefront: which, depends on the
// length of the sample's own list alone.
//   * cohort_check_kernel, per sample: every refusal a sample can cause (its ploidy, its pairs) and whether it has a pair.
//   * cohort_prepare_kernel, one workgroup per item: the samples' flags -> pre[item], by the header's precedence; C, the
//     chromosomes of the participating samples; f_0 = 1 / A at the item's slots.  The later kernels only ever look at items
//     with pre == OK, whose alleles all lie in 0 .. MAX_ALLELE: no index derived from an item is used before that.
//   * cohort_weight_kernel, per sample: m_s, and w_k = exp(lw_k - m_s), doubled for a heterozygous pair (a factor of two is
//     exact wherever it is applied), once per call.
//   * cohort_estep_kernel, per sample: f of the item is a dense table by allele in global memory (8 KB per item, read by every
//     wavefront of the item: it stays in the cache), lanes stride over the pairs, q = (w f(a)) f(b) into r, the per-lane
//     partial sums of Z go through a butterfly (a workgroup: then (0 + 1) + (2 + 3) over its wavefronts), then r = q / Z from
//     the lane's own stores and logZ_s.  The last pass (FINAL) also reduces the call -- largest q, then smallest a, then first
//     -- and zeroes what a refused item's samples own.
//   * cohort_chunk_kernel, one wavefront per chunk of the incidence list: lanes stride over the entries and gather r, a
//     butterfly, one partial count per chunk.
//   * cohort_update_kernel, one workgroup per item: a thread per slot adds the slot's chunks in order, n(c); f_t(c), the
//     largest change, and sum_s logZ_s -- per-thread strided partial sums, a butterfly over the wavefront, (0 + 1) + (2 + 3)
//     over the wavefronts -- into the trace.  After the last E-step it writes the support, f and n instead.
// The order of every sum is fixed by the position of a pair inside its item.  All results leave through plain vector stores;
// there is no global atomic.
#include <climits>
#include <cmath>
#include <cstring>

#include "side_unit.h"
#include "../../include/tredcohort.h"

namespace {
using namespace side_unit;

thread_local std::string g_cohort_error;   // the text of tredcohort_last_error()

constexpr int CAP = TREDGPU_COHORT_MAX_ALLELE, NALLELE = CAP + 1;
constexpr int CHUNK = TREDGPU_COHORT_CHUNK;
constexpr int LONG_LIST = TREDGPU_COHORT_LONG_LIST;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int FLAG_BAD = 1, FLAG_TOO_LONG = 2, FLAG_SOME = 4;      // what cohort_check_kernel says of a sample
constexpr int MAX_BLOCKS = 1 << 16;                        // workgroups of a launch at the most (the loops are grid-stride)
constexpr int64_t MAX_ITEMS = INT32_MAX / NALLELE;         // a slot index is an int32
static_assert(WAVES == 4 && CHUNK >= 64, "four wavefronts per workgroup, a chunk is at least one stride of a wavefront");

struct CohortArgs {
    const int64_t *item_off, *sample_off;
    const int32_t *a, *b;
    const double* lw;
    const int32_t* ploidy;
    const int64_t* allele_off;
    // built by the host while it stages
    const int32_t* sample_item;            // [n_samples]: the item of a sample
    const int64_t* soff;                   // [n_items + 1]: the slots of an item
    const int32_t *slot_allele, *slot_item;    // [n_slots]
    const int64_t *slot_eoff, *slot_coff;  // [n_slots + 1]: the entries and the chunks of a slot
    const int32_t* chunk_slot;             // [n_chunks]
    const int32_t* ent_pair;               // [n_entries]: the pair of an entry
    const int32_t *long_list, *short_list; // [n_long], [n_short]: the samples of more than LONG_LIST pairs, and the others
    // on the device only
    int32_t *pre, *sflag;                  // [n_items]: the status;  [n_samples]: FLAG_*
    double *chrom, *f;                     // [n_items]: C;  [n_items][NALLELE]: f by allele
    double *ms, *logz, *w;                 // [n_samples];  [n_samples];  [n_pairs]
    double* part;                          // [n_chunks]
    int32_t *out_status, *out_n_alleles, *out_alleles;
    double *out_freq, *out_count, *out_trace;
    int32_t* out_sample_call;
    double *out_sample_values, *out_r;
    int64_t n_items, n_samples, n_chunks, n_long, n_short;
    int32_t iters;
    double alpha;
};

// the sum of x over the workgroup, in every thread: a butterfly over the wavefront, then (0 + 1) + (2 + 3)
__device__ __forceinline__ double block_sum(double x, double* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    __syncthreads();                                               // red is free
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double block_max(double x, double* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = fmax(x, __shfl_xor(x, d, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// The work of the three per-sample kernels: a sample of more than LONG_LIST pairs has a workgroup to itself (the first n_long
// workgroups of the launch, by long_list), the others a wavefront each (by short_list, four to a workgroup).  Which of the
// two a sample gets depends on the length of its own list alone.  BLOCK: the workgroup's part.
template <bool BLOCK>
__device__ __forceinline__ int64_t sample_of(const CohortArgs& g) {
    if (BLOCK) return g.long_list[blockIdx.x];
    const int64_t k = ((int64_t)blockIdx.x - g.n_long) * WAVES + (threadIdx.x >> 6);
    return k < g.n_short ? g.short_list[k] : -1;
}

template <bool BLOCK>
__device__ __forceinline__ void check_sample(const CohortArgs& g, int64_t s) {
    constexpr int STRIDE = BLOCK ? THREADS : 64;
    const int tid = BLOCK ? threadIdx.x : (threadIdx.x & 63);
    const int pl = g.ploidy[s];
    const int64_t lo = g.sample_off[s], hi = g.sample_off[s + 1];
    int flags = ((pl != 1 && pl != 2) ? FLAG_BAD : 0) | (hi > lo ? FLAG_SOME : 0);
#pragma unroll 4
    for (int64_t k = lo + tid; k < hi; k += STRIDE) {
        const int x = g.a[k], y = g.b[k];
        const double lw = g.lw[k];
        if (x < 0 || y < 0 || x > y || !(lw <= 0.0) || !isfinite(lw) || (pl == 1 && x != y)) flags |= FLAG_BAD;
        else if (y > CAP) flags |= FLAG_TOO_LONG;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) flags |= __shfl_xor(flags, d, 64);
    if (BLOCK) {
        __shared__ int wave_flags[WAVES];
        if ((threadIdx.x & 63) == 0) wave_flags[threadIdx.x >> 6] = flags;
        __syncthreads();
        flags = wave_flags[0] | wave_flags[1] | wave_flags[2] | wave_flags[3];
    }
    if (tid == 0) g.sflag[s] = flags;
}

// every refusal a sample can cause, and whether it takes part -> sflag[s]
__global__ __launch_bounds__(THREADS) void cohort_check_kernel(CohortArgs g) {
    if ((int64_t)blockIdx.x < g.n_long) {
        check_sample<true>(g, sample_of<true>(g));
    } else {
        const int64_t s = sample_of<false>(g);
        if (s >= 0) check_sample<false>(g, s);
    }
}

__global__ __launch_bounds__(THREADS) void cohort_prepare_kernel(CohortArgs g) {
    __shared__ double red[WAVES];
    for (int64_t item = blockIdx.x; item < g.n_items; item += gridDim.x) {
        int flags = 0;
        double chrom = 0.0;                                        // (whole numbers below 2^33: every order gives the same sum)
        for (int64_t s = g.item_off[item] + threadIdx.x; s < g.item_off[item + 1]; s += THREADS) {
            const int fl = g.sflag[s];
            flags |= fl;
            if ((fl & FLAG_SOME) && !(fl & FLAG_BAD)) chrom += (double)g.ploidy[s];        // (not bad: the ploidy is 1 or 2)
        }
        const int bad = __syncthreads_or(flags & FLAG_BAD), too_long = __syncthreads_or(flags & FLAG_TOO_LONG);
        const int some = __syncthreads_or(flags & FLAG_SOME);
        chrom = block_sum(chrom, red);
        const int status = bad ? TREDGPU_COHORT_BAD_ITEM : too_long ? TREDGPU_COHORT_TOO_LONG : !some ? TREDGPU_COHORT_EMPTY
                                                                                                    : TREDGPU_COHORT_OK;
        if (threadIdx.x == 0) {
            g.pre[item] = status;
            g.chrom[item] = chrom;
        }
        if (status == TREDGPU_COHORT_OK) {
            // every allele of an accepted item lies in 0 .. CAP: its slots are its support (the host made them of nothing else)
            const int64_t j0 = g.soff[item], A = g.soff[item + 1] - j0;
            const double f0 = 1.0 / (double)A;
            for (int64_t j = threadIdx.x; j < A; j += THREADS) g.f[item * NALLELE + g.slot_allele[j0 + j]] = f0;
        }
    }
}

template <bool BLOCK>
__device__ __forceinline__ void weigh_sample(const CohortArgs& g, int64_t s, double* red) {
    constexpr int STRIDE = BLOCK ? THREADS : 64;
    const int tid = BLOCK ? threadIdx.x : (threadIdx.x & 63);
    if (g.pre[g.sample_item[s]] != TREDGPU_COHORT_OK) return;      // (the same in every lane that works on the sample)
    const int64_t lo = g.sample_off[s], hi = g.sample_off[s + 1];
    double m = -INFINITY;
#pragma unroll 4
    for (int64_t k = lo + tid; k < hi; k += STRIDE) m = fmax(m, g.lw[k]);
    if (BLOCK) {
        m = block_max(m, red);
    } else {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    }
    const bool diploid = g.ploidy[s] == 2;
#pragma unroll 4
    for (int64_t k = lo + tid; k < hi; k += STRIDE) {
        const double w = exp(g.lw[k] - m);
        g.w[k] = (diploid && g.a[k] != g.b[k]) ? 2.0 * w : w;
    }
    if (tid == 0) g.ms[s] = hi > lo ? m : 0.0;
}

__global__ __launch_bounds__(THREADS) void cohort_weight_kernel(CohortArgs g) {
    __shared__ double red[WAVES];
    if ((int64_t)blockIdx.x < g.n_long) {
        weigh_sample<true>(g, sample_of<true>(g), red);
    } else {
        const int64_t s = sample_of<false>(g);
        if (s >= 0) weigh_sample<false>(g, s, red);
    }
}

// candidate calls: the larger q, then the smaller a, then the earlier pair
struct Best { double q; int x; long long k; };
__device__ __forceinline__ bool better(const Best& u, const Best& v) {
    return u.q > v.q || (u.q == v.q && (u.x < v.x || (u.x == v.x && u.k < v.k)));
}

struct BestSlots {
    double q[WAVES];
    int x[WAVES];
    long long k[WAVES];
};

template <bool FINAL, bool BLOCK>
__device__ __forceinline__ void estep_sample(const CohortArgs& g, int64_t s, double* red, BestSlots* slots) {
    constexpr int STRIDE = BLOCK ? THREADS : 64;
    const int tid = BLOCK ? threadIdx.x : (threadIdx.x & 63);
    const int64_t item = g.sample_item[s];
    const int64_t lo = g.sample_off[s], hi = g.sample_off[s + 1];
    if (g.pre[item] != TREDGPU_COHORT_OK || hi == lo) {            // a refused or empty item, a sample that takes no part: zeros
        if (FINAL) {
            for (int64_t k = lo + tid; k < hi; k += STRIDE) g.out_r[k] = 0.0;
            if (tid < 3) g.out_sample_call[s * 3 + tid] = 0;
            if (tid < 2) g.out_sample_values[s * 2 + tid] = 0.0;
        }
        if (tid == 0) g.logz[s] = 0.0;
        return;                                                    // (the same in every lane that works on the sample)
    }
    const double* f = g.f + item * NALLELE;                        // (alleles of an accepted item: 0 .. CAP)
    const bool diploid = g.ploidy[s] == 2;
    double Z = 0.0;
    Best best = {-1.0, INT_MAX, LLONG_MAX};
    // (unrolled: the loads of four pairs are in flight together, the adds keep their order)
#pragma unroll 4
    for (int64_t k = lo + tid; k < hi; k += STRIDE) {
        const int x = g.a[k];
        double q = g.w[k] * f[x];
        if (diploid) q = q * f[g.b[k]];
        g.out_r[k] = q;
        Z += q;
        if (FINAL) {
            const Best cand = {q, x, (long long)(k - lo)};
            if (better(cand, best)) best = cand;
        }
    }
    if (BLOCK) {
        Z = block_sum(Z, red);
    } else {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) Z += __shfl_xor(Z, d, 64);
    }
#pragma unroll 4
    for (int64_t k = lo + tid; k < hi; k += STRIDE) g.out_r[k] = g.out_r[k] / Z;       // (the lane's own stores)
    const double logz = g.ms[s] + log(Z);
    if (tid == 0) g.logz[s] = logz;
    if (FINAL) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const Best o = {__shfl_xor(best.q, d, 64), __shfl_xor(best.x, d, 64), __shfl_xor(best.k, d, 64)};
            if (better(o, best)) best = o;
        }
        if (BLOCK) {
            const int wave = threadIdx.x >> 6;
            if ((threadIdx.x & 63) == 0) { slots->q[wave] = best.q; slots->x[wave] = best.x; slots->k[wave] = best.k; }
            __syncthreads();
            for (int v = 0; v < WAVES; ++v) {
                const Best o = {slots->q[v], slots->x[v], slots->k[v]};
                if (better(o, best)) best = o;
            }
        }
        if (best.k == LLONG_MAX) best = {0.0, 0, 0};               // (no q compared as larger than -1: none was a number)
        if (tid == 0) {
            g.out_sample_call[s * 3 + 0] = (int32_t)best.k;
            g.out_sample_call[s * 3 + 1] = g.a[lo + best.k];
            g.out_sample_call[s * 3 + 2] = g.b[lo + best.k];
            g.out_sample_values[s * 2 + 0] = logz;
            g.out_sample_values[s * 2 + 1] = best.q / Z;
        }
    }
}

template <bool FINAL>
__global__ __launch_bounds__(THREADS) void cohort_estep_kernel(CohortArgs g) {
    __shared__ double red[WAVES];
    __shared__ BestSlots slots;
    if ((int64_t)blockIdx.x < g.n_long) {
        estep_sample<FINAL, true>(g, sample_of<true>(g), red, &slots);
    } else {
        const int64_t s = sample_of<false>(g);
        if (s >= 0) estep_sample<FINAL, false>(g, s, red, &slots);
    }
}

__global__ __launch_bounds__(THREADS) void cohort_chunk_kernel(CohortArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * WAVES;
    for (int64_t c = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); c < g.n_chunks; c += stride) {
        const int64_t slot = g.chunk_slot[c];
        if (g.pre[g.slot_item[slot]] != TREDGPU_COHORT_OK) continue;
        const int64_t e0 = g.slot_eoff[slot] + (c - g.slot_coff[slot]) * CHUNK;
        const int64_t e1 = min(e0 + (int64_t)CHUNK, g.slot_eoff[slot + 1]);
        double x = 0.0;
#pragma unroll 4
        for (int64_t e = e0 + lane; e < e1; e += 64) x += g.out_r[g.ent_pair[e]];      // (the host's own indices: pairs of the call)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
        if (lane == 0) g.part[c] = x;
    }
}

// n(c) of a slot: its chunks in order
__device__ __forceinline__ double slot_count(const CohortArgs& g, int64_t slot) {
    double n = 0.0;
#pragma unroll 8
    for (int64_t c = g.slot_coff[slot]; c < g.slot_coff[slot + 1]; ++c) n += g.part[c];
    return n;
}

// t: the iteration, from 0; below 0 the pass behind the last E-step
__global__ __launch_bounds__(THREADS) void cohort_update_kernel(CohortArgs g, int t) {
    __shared__ double red[WAVES];
    for (int64_t item = blockIdx.x; item < g.n_items; item += gridDim.x) {
        const int status = g.pre[item];
        const int64_t j0 = g.soff[item], A = g.soff[item + 1] - j0;
        double* f = g.f + item * NALLELE;
        if (t < 0) {
            const int64_t lo = g.allele_off[item], room = g.allele_off[item + 1] - lo;     // (room >= A: the host has checked)
            const bool ok = status == TREDGPU_COHORT_OK;
            for (int64_t j = threadIdx.x; j < room; j += THREADS) {
                const bool in = ok && j < A;
                const int al = in ? g.slot_allele[j0 + j] : 0;
                g.out_alleles[lo + j] = al;
                g.out_freq[lo + j] = in ? f[al] : 0.0;
                g.out_count[lo + j] = in ? slot_count(g, j0 + j) : 0.0;
            }
            if (!ok)
                for (int64_t k = threadIdx.x; k < 2 * (int64_t)g.iters; k += THREADS) g.out_trace[item * 2 * g.iters + k] = 0.0;
            if (threadIdx.x == 0) {
                g.out_status[item] = status;
                g.out_n_alleles[item] = ok ? (int32_t)A : 0;
            }
            continue;
        }
        if (status != TREDGPU_COHORT_OK) continue;                 // (the same in every lane of the workgroup)
        const double pseudo = g.alpha / (double)A, denom = g.chrom[item] + g.alpha;
        double delta = 0.0;
        for (int64_t j = threadIdx.x; j < A; j += THREADS) {
            const int al = g.slot_allele[j0 + j];
            const double was = f[al], now = (slot_count(g, j0 + j) + pseudo) / denom;
            f[al] = now;
            delta = fmax(delta, fabs(now - was));
        }
        delta = block_max(delta, red);
        double L = 0.0;
        for (int64_t s = g.item_off[item] + threadIdx.x; s < g.item_off[item + 1]; s += THREADS) L += g.logz[s];
        L = block_sum(L, red);
        if (threadIdx.x == 0) {
            g.out_trace[(item * g.iters + t) * 2 + 0] = L;
            g.out_trace[(item * g.iters + t) * 2 + 1] = delta;
        }
    }
}

struct State : StateBase {};
Registry<State> g_states;

// offsets of a CSR list: they begin at 0 and do not descend
int offsets_refusal(std::string& err, const char* who, const int64_t* off, int64_t n) {
    if (off[0] != 0) return fail(err, -2, "%s_off[0] must be 0", who);
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(err, -2, "%s_off descends at %lld", who, (long long)i);
    return 0;
}

// what the host builds of a call: the incidence list of every item, allele by allele, and its chunks
struct Incidence {
    std::vector<int32_t> sample_item, slot_allele, slot_item, chunk_slot, ent_pair, long_list, short_list;
    std::vector<int64_t> soff, slot_eoff, slot_coff;
};

// A stable counting sort per item: the entries of allele c are the pairs that name it, in the order of the samples and of
// their pairs, a before b (a ploidy-1 pair once).  Alleles outside 0 .. CAP get no entry.
void build_incidence(int64_t n_items, const int64_t* item_off, const int64_t* sample_off, const int32_t* a, const int32_t* b,
                     const int32_t* ploidy, Incidence& inc) {
    const int64_t n_samples = item_off[n_items];
    inc.sample_item.resize((size_t)n_samples);
    inc.soff.assign((size_t)n_items + 1, 0);
    inc.slot_eoff.assign(1, 0);
    inc.slot_coff.assign(1, 0);
    auto in_range = [](int32_t x) { return x >= 0 && x <= CAP; };
    std::vector<int64_t> at(NALLELE);
    for (int64_t i = 0; i < n_items; ++i) {
        std::fill(at.begin(), at.end(), 0);
        for (int64_t s = item_off[i]; s < item_off[i + 1]; ++s) {
            inc.sample_item[(size_t)s] = (int32_t)i;
            (sample_off[s + 1] - sample_off[s] > LONG_LIST ? inc.long_list : inc.short_list).push_back((int32_t)s);
            const bool twice = ploidy[s] != 1;
            for (int64_t k = sample_off[s]; k < sample_off[s + 1]; ++k) {
                if (in_range(a[k])) at[a[k]] += 1;
                if (twice && in_range(b[k])) at[b[k]] += 1;
            }
        }
        int64_t e = inc.slot_eoff.back();
        for (int c = 0; c < NALLELE; ++c) {
            const int64_t count = at[c];
            at[c] = e;                                             // where the allele's next entry goes
            if (!count) continue;
            const int32_t slot = (int32_t)inc.slot_allele.size();
            inc.slot_allele.push_back(c);
            inc.slot_item.push_back((int32_t)i);
            const int64_t chunks = (count + CHUNK - 1) / CHUNK;
            inc.chunk_slot.insert(inc.chunk_slot.end(), (size_t)chunks, slot);
            e += count;
            inc.slot_eoff.push_back(e);
            inc.slot_coff.push_back(inc.slot_coff.back() + chunks);
        }
        inc.ent_pair.resize((size_t)e);
        for (int64_t s = item_off[i]; s < item_off[i + 1]; ++s) {
            const bool twice = ploidy[s] != 1;
            for (int64_t k = sample_off[s]; k < sample_off[s + 1]; ++k) {
                if (in_range(a[k])) inc.ent_pair[(size_t)at[a[k]]++] = (int32_t)k;
                if (twice && in_range(b[k])) inc.ent_pair[(size_t)at[b[k]]++] = (int32_t)k;
            }
        }
        inc.soff[(size_t)i + 1] = (int64_t)inc.slot_allele.size();
    }
}

unsigned blocks_for(int64_t waves) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + WAVES - 1) / WAVES, MAX_BLOCKS)); }

}  // namespace

extern "C" {

int tredcohort_evaluate(tredgpu_ctx* ctx, const tredcohort_params* params, int64_t n_items, const int64_t* item_off,
                        const int64_t* sample_off, const int32_t* a, const int32_t* b, const double* lw, const int32_t* ploidy,
                        const int64_t* allele_off, int32_t* out_status, int32_t* out_n_alleles, int32_t* out_alleles,
                        double* out_freq, double* out_count, double* out_trace, int32_t* out_sample_call,
                        double* out_sample_values, double* out_r) {
    std::string& err = g_cohort_error;
    err.clear();
    if (!ctx) return fail(err, -2, "ctx is NULL");
    if (!params) return fail(err, -2, "params is NULL");
    const int iters = params->iters;
    const double alpha = params->alpha;
    if (iters < 1 || iters > TREDGPU_COHORT_MAX_ITERS || !(alpha > 0.0) || !std::isfinite(alpha))
        return fail(err, -2, "parameters out of range: 1 <= iters <= %d, alpha > 0 (iters %d, alpha %g)", TREDGPU_COHORT_MAX_ITERS,
                    iters, alpha);
    if (n_items < 0 || n_items > MAX_ITEMS) return fail(err, -2, "n_items %lld out of range", (long long)n_items);
    if (n_items == 0) return 0;
    if (!item_off || !sample_off || !allele_off || !out_status || !out_n_alleles || !out_trace)
        return fail(err, -2, "NULL array argument");
    int rc;
    if ((rc = offsets_refusal(err, "item", item_off, n_items))) return rc;
    const int64_t n_samples = item_off[n_items];
    if (n_samples > INT32_MAX) return fail(err, -2, "%lld samples: more than INT32_MAX", (long long)n_samples);
    if ((rc = offsets_refusal(err, "sample", sample_off, n_samples))) return rc;
    if ((rc = offsets_refusal(err, "allele", allele_off, n_items))) return rc;
    const int64_t n_pairs = sample_off[n_samples];
    if (n_pairs > INT32_MAX) return fail(err, -2, "%lld pairs: more than INT32_MAX", (long long)n_pairs);
    if ((n_samples && (!ploidy || !out_sample_call || !out_sample_values)) || (n_pairs && (!a || !b || !lw || !out_r)) ||
        (allele_off[n_items] && (!out_alleles || !out_freq || !out_count)))
        return fail(err, -2, "NULL array argument");

    Incidence inc;
    build_incidence(n_items, item_off, sample_off, a, b, ploidy, inc);
    for (int64_t i = 0; i < n_items; ++i)
        if (allele_off[i + 1] - allele_off[i] < inc.soff[(size_t)i + 1] - inc.soff[(size_t)i])
            return fail(err, -2, "item %lld has %lld alleles and room for %lld", (long long)i,
                        (long long)(inc.soff[(size_t)i + 1] - inc.soff[(size_t)i]), (long long)(allele_off[i + 1] - allele_off[i]));

    hipStream_t st;
    if ((rc = select_device(err, ctx, st))) return rc;
    State& s = *g_states.state_of(ctx);
    CohortArgs g{};
    const size_t n = (size_t)n_items, ns = (size_t)n_samples, np = (size_t)n_pairs, room = (size_t)allele_off[n_items];
    const size_t n_slots = inc.slot_allele.size(), n_chunks = inc.chunk_slot.size();
    std::vector<Array> arrays = {
        arr_in(g.item_off, item_off, n + 1), arr_in(g.sample_off, sample_off, ns + 1), arr_in(g.a, a, np), arr_in(g.b, b, np),
        arr_in(g.lw, lw, np), arr_in(g.ploidy, ploidy, ns), arr_in(g.allele_off, allele_off, n + 1),
        arr_in(g.sample_item, (const int32_t*)inc.sample_item.data(), ns), arr_in(g.soff, (const int64_t*)inc.soff.data(), n + 1),
        arr_in(g.slot_allele, (const int32_t*)inc.slot_allele.data(), n_slots),
        arr_in(g.slot_item, (const int32_t*)inc.slot_item.data(), n_slots),
        arr_in(g.slot_eoff, (const int64_t*)inc.slot_eoff.data(), n_slots + 1),
        arr_in(g.slot_coff, (const int64_t*)inc.slot_coff.data(), n_slots + 1),
        arr_in(g.chunk_slot, (const int32_t*)inc.chunk_slot.data(), n_chunks),
        arr_in(g.ent_pair, (const int32_t*)inc.ent_pair.data(), inc.ent_pair.size()),
        arr_in(g.long_list, (const int32_t*)inc.long_list.data(), inc.long_list.size()),
        arr_in(g.short_list, (const int32_t*)inc.short_list.data(), inc.short_list.size()),
        arr_scratch(g.sflag, ns), arr_scratch(g.pre, n), arr_scratch(g.chrom, n), arr_scratch(g.f, n * NALLELE), arr_scratch(g.ms, ns),
        arr_scratch(g.logz, ns), arr_scratch(g.w, np), arr_scratch(g.part, n_chunks),
        arr_out(g.out_status, out_status, n), arr_out(g.out_n_alleles, out_n_alleles, n), arr_out(g.out_alleles, out_alleles, room),
        arr_out(g.out_freq, out_freq, room), arr_out(g.out_count, out_count, room), arr_out(g.out_trace, out_trace, n * 2 * (size_t)iters),
        arr_out(g.out_sample_call, out_sample_call, ns * 3), arr_out(g.out_sample_values, out_sample_values, ns * 2),
        arr_out(g.out_r, out_r, np)};
    if ((rc = stage(err, s, st, arrays))) return rc;
    g.n_items = n_items;
    g.n_samples = n_samples;
    g.n_chunks = (int64_t)n_chunks;
    g.n_long = (int64_t)inc.long_list.size();
    g.n_short = (int64_t)inc.short_list.size();
    g.iters = iters;
    g.alpha = alpha;

    if ((rc = timed_begin(err, s, st))) return rc;
    const dim3 per_item((unsigned)std::min<int64_t>(n_items, MAX_BLOCKS)), per_sample((unsigned)(g.n_long + (g.n_short + WAVES - 1) / WAVES)), per_chunk(blocks_for(g.n_chunks));
    if (n_samples) hipLaunchKernelGGL(cohort_check_kernel, per_sample, dim3(THREADS), 0, st, g);
    hipLaunchKernelGGL(cohort_prepare_kernel, per_item, dim3(THREADS), 0, st, g);
    if (n_samples) hipLaunchKernelGGL(cohort_weight_kernel, per_sample, dim3(THREADS), 0, st, g);
    for (int t = 0; t <= iters; ++t) {                             // the iterations, then the last E-step and its counts
        const bool last = t == iters;
        if (n_samples) {
            if (last) hipLaunchKernelGGL(cohort_estep_kernel<true>, per_sample, dim3(THREADS), 0, st, g);
            else hipLaunchKernelGGL(cohort_estep_kernel<false>, per_sample, dim3(THREADS), 0, st, g);
        }
        if (n_chunks) hipLaunchKernelGGL(cohort_chunk_kernel, per_chunk, dim3(THREADS), 0, st, g);
        hipLaunchKernelGGL(cohort_update_kernel, per_item, dim3(THREADS), 0, st, g, last ? -1 : t);
    }
    if ((rc = timed_end(err, s, st))) return rc;
    return read_back(err, s, st, arrays);      // (the host's tables are read by their copies until the stream is drained)
}

int tredcohort_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) { return timing(g_cohort_error, g_states, ctx, launches, total_ms, false); }

int tredcohort_reset_timing(tredgpu_ctx* ctx) { return timing(g_cohort_error, g_states, ctx, nullptr, nullptr, true); }

void tredcohort_release(tredgpu_ctx* ctx) { release(g_states, ctx, {}); }

const char* tredcohort_last_error(void) { return g_cohort_error.c_str(); }

}  // extern "C"
