// scan_unit.h -- the device code that the tandem-repeat scan (scan.hip, include/tredscan.h) and the interrupted-tract scan
// (tract.hip, include/tredtract.h) share: the argument block, a lane's masks e_p, the summary and ends passes over the
// tiles, the one-workgroup prefix sum of a table, and a lane's records (the runs that start in its letters and pass the
// exact test).  Each unit that includes it has its own copy of the kernels (internal linkage); the harness is side_unit.h's.
//
// The buffer of all segments is cut into tiles of TILE = 4096 letters, one wavefront each; lane l of a tile owns its letters
// [64 l, 64 l + 64) and reads them with four 16-byte loads, and the 16 letters behind them (the halo: e_p looks p <= 6 letters
// ahead) with a fifth.  From the codes it makes three 80-bit planes (bit 0, bit 1 and "is N" of every code) and from the
// planes, with shifts and XORs, the 64-bit mask e_p of its letters for every period, plus 16 more bits behind them which only
// the primitive-motif test reads.  The ends of the segments that fall into a lane's letters clear the p bits in front of
// them (nothing crosses a segment's end); a lane finds them by bisection of seg_off.
#pragma once
#include <climits>

#include "side_unit.h"
#include "../../include/tredscan.h"

namespace scan_unit {
using namespace side_unit;

constexpr int P = TREDSCAN_MAX_PERIOD, TILE = TREDSCAN_TILE, LANE = 64;
constexpr int THREADS = 256, WAVES = THREADS / 64, SCAN_THREADS = 1024, SCAN_WAVES = SCAN_THREADS / 64, BATCH = 4;
constexpr long long CONT = -1;             // a tile that is all ones: its first 0 is some later tile's
constexpr int NONE = INT_MAX;              // no 0 in a lane's mask, or in the lanes above
static_assert(TILE == 64 * LANE && P == 6, "a tile is one wavefront of 64-letter lanes; the divisor table is for periods 1 .. 6");

struct ScanArgs {
    const uint8_t* letters;                // (the buffer is whole tiles and 64 bytes long: every load below is inside it)
    const int64_t* seg_off;
    int32_t n_seg;
    int64_t first, n;                      // seg_off[0], seg_off[n_seg]
    int64_t n_tiles;
    int64_t need[P];                       // (min_copies - 1) p: the ones a run of enough copies has; -1: the period is off
    int32_t min_copies[P];
    int64_t* fz;                           // [P][n_tiles]: the first 0 of e_p in the tile, or CONT
    int64_t* nz;                           // [P][n_tiles]: the first 0 at or behind the start of the next tile
    uint8_t* last;                         // [n_tiles]: bit p - 1: the last bit of the tile's e_p
    uint32_t* count;                       // [n_tiles]: records that start in the tile
    int64_t* off;                          // [n_tiles + 1]: their exclusive prefix sum; off[n_tiles] is the total
    int64_t cap;
    int32_t *out_seg, *out_len, *out_period;
    int64_t* out_start;
};

// the first index k in 0 .. n_seg with seg_off[k] > pos, n_seg + 1 when there is none
__device__ __forceinline__ int upper_bound(const ScanArgs& a, int64_t pos) {
    int lo = 0, hi = a.n_seg + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.seg_off[mid] <= pos) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// bits [from, to) of a lane that begins at g0, as a mask (the positions may lie outside the lane)
__device__ __forceinline__ uint64_t bits_between(int64_t from, int64_t to, int64_t g0) {
    const int lo = from > g0 ? (int)(from - g0 < LANE ? from - g0 : LANE) : 0, hi = to < g0 ? 0 : (int)(to - g0 < LANE ? to - g0 : LANE);
    if (lo >= hi) return 0;
    const uint64_t ones = hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1;
    return ones << lo;
}

// e_p of the lane's 64 letters (lo) and, before the segments' ends are applied, of the 16 behind them (hi: bits 0 .. 15 - p)
__device__ __forceinline__ void lane_masks(const ScanArgs& a, const uint8_t* lut, int64_t g0, uint64_t (&lo)[P], uint32_t (&hi)[P]) {
    const uint4* src = (const uint4*)(a.letters + g0);
    uint64_t plane[3] = {0, 0, 0};
    uint32_t behind[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const uint4 v = src[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t piece[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t c = lut[(w[j >> 2] >> (8 * (j & 3))) & 255u];
            piece[0] |= (c & 1u) << j;
            piece[1] |= ((c >> 1) & 1u) << j;
            piece[2] |= (c >> 2) << j;
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            if (q < 4) plane[b] |= (uint64_t)piece[b] << (16 * q);
            else behind[b] = piece[b];
        }
    }
#pragma unroll
    for (int p = 1; p <= P; ++p) {
        uint64_t differ = plane[2];
        uint32_t differ_behind = behind[2];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            differ |= plane[b] ^ ((plane[b] >> p) | ((uint64_t)behind[b] << (64 - p)));
            differ_behind |= behind[b] ^ (behind[b] >> p);
        }
        lo[p - 1] = ~differ;
        hi[p - 1] = ~differ_behind;
    }
    // nothing below the first segment, nothing at or behind the end of the last, and no e_p across a segment's end b: the
    // bits [b - p, b).  The ends that matter lie in (g0, g0 + 64 + P)
    uint64_t keep = bits_between(a.first, a.n, g0);
    int64_t pos = g0;
    for (;;) {
        const int k = upper_bound(a, pos);
        if (k > a.n_seg) break;
        const int64_t b = a.seg_off[k];
        if (b >= g0 + LANE + P) break;
        for (int p = 1; p <= P; ++p) lo[p - 1] &= ~bits_between(b - p, b, g0);
        pos = b;
    }
#pragma unroll
    for (int p = 0; p < P; ++p) lo[p] &= keep;
}

// where the first 0 of a lane's mask is, in letters from the tile's start
__device__ __forceinline__ int first_zero(uint64_t m, int lane) { return m == ~0ull ? NONE : lane * LANE + __builtin_ctzll(~m); }

__device__ __forceinline__ void fill_lut(uint8_t* lut) {
    const int c = threadIdx.x, u = c & 0xDF;
    lut[c] = u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
    __syncthreads();
}

// per tile and period the position of the first 0 of e_p in the tile, or CONT where the tile is all ones, and the last bit
// of the tile
static __global__ __launch_bounds__(THREADS) void scan_summary_kernel(ScanArgs a) {
    __shared__ uint8_t lut[256];
    fill_lut(lut);
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;
    uint64_t lo[P];
    uint32_t hi[P];
    lane_masks(a, lut, tile * TILE + lane * LANE, lo, hi);
    uint32_t last = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        int z = first_zero(lo[p], lane);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) z = min(z, __shfl_xor(z, d, 64));
        if (lane == 0) a.fz[p * a.n_tiles + tile] = z == NONE ? CONT : tile * TILE + z;
        last |= (uint32_t)(lo[p] >> 63) << p;
    }
    if (lane == 63) a.last[tile] = (uint8_t)last;
}

// The two scans over the tiles' tables, one workgroup of 16 wavefronts each.  A wavefront has a stretch of consecutive tiles
// and its lanes consecutive tiles of it (a load is 64 entries in a row); it reduces its stretch, the 16 results meet in LDS,
// and it goes over the stretch again, 64 tiles a step with a scan over the lanes, from what came in from its side.  The
// loads of BATCH steps are issued before the first of their scans.  (One wavefront for all tiles took 0.5 ms for the 62 500
// tiles of 256 million letters; a stretch per THREAD, a load of which touches 64 cache lines, 0.1 ms.)
__device__ __forceinline__ void stretch_of(const ScanArgs& a, int wave, int64_t& lo, int64_t& hi) {
    const int64_t per = ((a.n_tiles + SCAN_WAVES - 1) / SCAN_WAVES + 63) / 64 * 64;
    lo = wave * per < a.n_tiles ? wave * per : a.n_tiles;
    hi = lo + per < a.n_tiles ? lo + per : a.n_tiles;
}

// One workgroup per period: nz[t] is the first fz[u] with u > t that is a position, and n behind the last tile.  Positions
// grow with the tile, so that is the minimum over u > t with "all ones" as the largest value there is.
static __global__ __launch_bounds__(SCAN_THREADS) void scan_ends_kernel(ScanArgs a) {
    __shared__ long long wave_min[SCAN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t* __restrict__ fz = a.fz + blockIdx.x * a.n_tiles;
    int64_t* __restrict__ nz = a.nz + blockIdx.x * a.n_tiles;
    int64_t lo, hi;
    stretch_of(a, wave, lo, hi);
    long long x = LLONG_MAX;
    for (int64_t t = lo + lane; t < hi; t += 64) {
        const long long v = fz[t];
        if (v != CONT && v < x) x = v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long y = __shfl_xor(x, d, 64);
        x = y < x ? y : x;
    }
    if (lane == 0) wave_min[wave] = x;
    __syncthreads();
    long long carry = a.n;                                         // the first position behind the stretch
    for (int v = wave + 1; v < SCAN_WAVES; ++v) carry = wave_min[v] < carry ? wave_min[v] : carry;
    const int64_t steps = (hi - lo + 63) / 64;
    for (int64_t c = steps - 1; c >= 0; c -= BATCH) {
        long long v[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int64_t t = lo + (c - j) * 64 + lane;
            const long long f = c - j >= 0 && t < hi ? fz[t] : CONT;
            v[j] = f == CONT ? LLONG_MAX : f;
        }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            if (c - j < 0) continue;                               // (the same in every lane)
            long long m = v[j];                                    // the minimum of this lane and those above
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long long y = __shfl_down(m, (unsigned)d, 64);
                if (lane + d < 64 && y < m) m = y;
            }
            long long above = __shfl_down(m, 1u, 64);
            if (lane == 63 || carry < above) above = carry;
            const int64_t t = lo + (c - j) * 64 + lane;
            if (t < hi) nz[t] = above;
            const long long all = __shfl(m, 0, 64);
            carry = all < carry ? all : carry;
        }
    }
}

// off[t] = count[0] + .. + count[t - 1] for the n_tiles entries of a table, and off[n_tiles] their total: one workgroup,
// the order of the additions fixed.  (Reads a.count, a.off and a.n_tiles alone: tract.hip runs it over its own tables.
// Workgroup b of a launch of several has row b of a table of rows: count + b n_tiles, off + b (n_tiles + 1).)
static __global__ __launch_bounds__(SCAN_THREADS) void scan_offsets_kernel(ScanArgs a) {
    __shared__ long long wave_sum[SCAN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a.count += blockIdx.x * a.n_tiles;
    a.off += blockIdx.x * (a.n_tiles + 1);
    int64_t lo, hi;
    stretch_of(a, wave, lo, hi);
    long long x = 0;
    for (int64_t t = lo + lane; t < hi; t += 64) x += a.count[t];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    if (lane == 0) wave_sum[wave] = x;
    __syncthreads();
    long long carry = 0, total = 0;
    for (int v = 0; v < SCAN_WAVES; ++v) {
        if (v < wave) carry += wave_sum[v];
        total += wave_sum[v];
    }
    const int64_t steps = (hi - lo + 63) / 64;
    for (int64_t c = 0; c < steps; c += BATCH) {
        long long v[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            const int64_t t = lo + (c + j) * 64 + lane;
            v[j] = t < hi ? a.count[t] : 0;
        }
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
            long long incl = v[j];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long long up = __shfl_up(incl, (unsigned)d, 64);
                if (lane >= d) incl += up;
            }
            const int64_t t = lo + (c + j) * 64 + lane;
            if (t < hi) a.off[t] = carry + incl - v[j];
            carry += __shfl(incl, 63, 64);
        }
    }
    if (threadIdx.x == 0) a.off[a.n_tiles] = total;
}

// what a lane knows of a period once the masks are made
struct Period {
    uint64_t e;                            // the lane's e_p
    uint32_t behind;                       // and the bits behind it (the primitive test's)
    int above;                             // the first 0 in the lanes above, from the tile's start, or NONE
    long long beyond;                      // the first 0 behind the tile
};

// the position of the first 0 behind bit i of the lane's mask (bit i is set)
__device__ __forceinline__ int64_t run_end(const Period& s, int i, int64_t g0, int64_t tile0) {
    const uint64_t zeros = ~s.e & (~0ull << i);
    return zeros ? g0 + __builtin_ctzll(zeros) : s.above != NONE ? tile0 + s.above : s.beyond;
}

// has the motif at bit i of period p the period d: e_d is set at i .. i + p - d - 1
__device__ __forceinline__ bool has_period(const Period& s, int i, int span) {
    const uint64_t w = (s.e >> i) | (i ? (uint64_t)s.behind << (64 - i) : 0);
    const uint64_t want = (1ull << span) - 1;
    return (w & want) == want;
}

// The records that start in a lane's letters, per period, as masks, and what run_end needs to measure them; returns their
// number.  A lane's run starts are mask arithmetic (the bit is set, the bit before it is not: the lane below has that bit,
// the tile before has it for lane 0); the starts that can have min_copies copies are those with (min_copies - 1) p ones
// behind them, an AND of shifted masks over the lane's and the next lane's bits (log2 steps).  They are rare.  For each the
// end is the first 0 behind it: in the lane's own mask, else in the lanes above (a suffix minimum over the wavefront), else
// the tile's value from scan_ends_kernel.  No lane walks along a run.  The exact test: L / p >= min_copies, motif primitive.
// Every lane of the wavefront calls it (it shuffles).
__device__ __forceinline__ int lane_records(const ScanArgs& a, const uint8_t* lut, int lane, int64_t tile, Period (&s)[P], uint64_t (&rec)[P]) {
    const int64_t tile0 = tile * TILE, g0 = tile0 + lane * LANE;
    uint64_t lo[P];
    uint32_t hi[P];
    lane_masks(a, lut, g0, lo, hi);
    const uint32_t before = tile > 0 ? a.last[tile - 1] : 0;
    int mine = 0;
#pragma unroll
    for (int p = 1; p <= P; ++p) {
        Period& sp = s[p - 1];
        sp.e = lo[p - 1];
        sp.behind = hi[p - 1];
        sp.beyond = a.nz[(p - 1) * a.n_tiles + tile];
        int z = first_zero(sp.e, lane);                            // the suffix minimum over the lanes above
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_down(z, (unsigned)d, 64);
            if (lane + d < 64) z = min(z, y);
        }
        const int above = __shfl_down(z, 1u, 64);
        sp.above = lane == 63 ? NONE : above;
        rec[p - 1] = 0;
        const int64_t need = a.need[p - 1];
        if (need < 0) continue;                                    // (the same in every lane)
        const uint64_t below = __shfl_up(sp.e, 1u, 64);
        const uint64_t prev = lane == 0 ? (before >> (p - 1)) & 1u : below >> 63;
        uint64_t x = sp.e, next = __shfl_down(sp.e, 1u, 64);       // x: bit i is set where `len` ones begin at i
        if (lane == 63) next = ~0ull;                              // (what is not known counts as ones: the test below is exact)
        const int k = need < 64 ? (int)need : 64;
        int len = 1;
        while (len < k) {
            const int by = min(len, k - len);
            x &= (x >> by) | (next << (64 - by));
            next &= (next >> by) | (~0ull << (64 - by));
            len += by;
        }
        uint64_t cand = sp.e & ~((sp.e << 1) | prev) & x;
        while (cand) {
            const int i = __builtin_ctzll(cand);
            cand &= cand - 1;
            const int64_t length = run_end(sp, i, g0, tile0) - (g0 + i) + p;
            bool ok = length / p >= a.min_copies[p - 1];
            if (p == 2 || p == 3 || p == 5) ok = ok && !has_period(s[0], i, p - 1);
            if (p == 4) ok = ok && !has_period(s[1], i, 2);
            if (p == 6) ok = ok && !has_period(s[1], i, 4) && !has_period(s[2], i, 3);
            if (ok) rec[p - 1] |= 1ull << i;
        }
        mine += __builtin_popcountll(rec[p - 1]);
    }
    return mine;
}

}  // namespace scan_unit
