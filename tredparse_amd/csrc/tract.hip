// tract.hip -- interrupted tandem repeats of a letter sequence (tredtract_scan, include/tredtract.h): the perfect runs of
// seed_copies copies and more (the seeds), joined where at most max_gap substituted letters separate two of one template,
// as records in (segment, start, period) order.  A unit of its own, outside the source hash the profiles are tied to
// (csrc/Makefile); the harness is side_unit.h's, the tiles, masks and tile passes are scan_unit.h's, shared with scan.hip.
//
// Under the rule seed_copies p > max_gap + 2 p - 2 a seed's only possible partner to the left is its predecessor among the
// seeds of its period (tredtract.h), so a tract is a stretch of consecutive entries of the per-period seed list:
//   * scan_summary_kernel, scan_ends_kernel: the scan's, with seed_copies in the place of min_copies.
//   * tract_seeds_kernel<false>: lane_records' masks; the count of seeds per tile AND period.
//   * scan_offsets_kernel, a workgroup per period over its row of the table [period][tile]: where a tile's seeds go in the
//     period's list, and how long the list is.  The host reads the six lengths, lays the lists one behind the other and
//     sizes the seed buffer.  (One workgroup over all six rows was a third of the call's device time.)
//   * tract_seeds_kernel<true>: the same masks, a prefix sum over the lanes per period, each seed's global start and length
//     stored.  Within a period the list ascends by start.
//   * tract_link_kernel, a lane per seed: the predecessor is the entry before it unless it is the first of its period or lies
//     in another segment; the link is the gap's size and a compare of p letters; the gap's mismatches are counted from at
//     most 64 letters of the buffer.  One byte per seed (bit 0: the seed is a tract's head; above it the mismatches of the
//     gap in front of a linked seed), and per workgroup of 256 seeds the sums of both.
//   * scan_offsets_kernel over the workgroups' head counts and over their mismatch sums (reduce, scan, apply: the sums of a
//     workgroup are added in a fixed order, and so are the workgroups').
//   * tract_heads_kernel: a workgroup scans its 256 bytes again and adds what came before it; a head's inclusive head count
//     is its tract's number, under which it stores its own index and the mismatch prefix.
//   * tract_records_kernel<false>: the same scan; a tail (the next seed is a head, or there is none) has its tract's seeds,
//     mismatches and span as differences to what the head stored, and applies the min_copies test; the workgroup's count.
//   * scan_offsets_kernel over those counts; the host reads the total.
//   * tract_records_kernel<true>: each record stored at its place: the lists of the periods one behind the other, each by
//     (segment, start).  The C entry merges the six lists on the host (stable, the lower period first): records are as
//     rare as the scan's.
// Temporary memory: 169 bytes per tile of 4096 letters and 17 bytes per seed (and 36 per 256 seeds).  All results leave
// through plain vector stores; no atomic.
#include <cstring>
#include <vector>

#include "scan_unit.h"
#include "../../include/tredtract.h"

namespace {
using namespace scan_unit;

thread_local std::string g_tract_error;    // the text of tredtract_last_error()

constexpr int CHUNK = THREADS;             // the seeds of one workgroup of the per-seed kernels: one per thread

struct TractArgs {
    ScanArgs s;                            // the seed passes': min_copies and need hold seed_copies
    int32_t min_copies[P], max_gap[P];     // the whole copies a tract needs; the most letters of a gap
    uint32_t* cnt;                         // [P][n_tiles]: the seeds of a period that start in the tile
    int64_t* soff;                         // [P][n_tiles + 1]: their exclusive prefix sum within the period, and the period's total
    int64_t base[P + 1];                   // where the list of period p begins in the seed list, at [p - 1]; base[P]: n_seeds
    int64_t n_seeds, n_blocks;
    uint32_t *start, *len;                 // [n_seeds]: a seed's first letter in the buffer, its length
    uint8_t* link;                         // [n_seeds]: bit 0: a head; bits 1 ..: the mismatches of the gap in front (a linked seed's)
    uint32_t *head_idx, *head_mm;          // [tracts]: the head's index, the mismatch prefix at the head (modulo 2^32)
    uint32_t *blk_head, *blk_mm, *blk_rec; // [n_blocks]: heads, mismatches, records of a workgroup's seeds
    int64_t *off_head, *off_mm, *off_rec;  // [n_blocks + 1]: their exclusive prefix sums
    int32_t *out_seg, *out_len, *out_period, *out_seeds, *out_mismatch;   // [records], the periods' lists one behind the other
    int64_t* out_start;
};

template <bool WRITE>
__global__ __launch_bounds__(THREADS) void tract_seeds_kernel(TractArgs a) {
    __shared__ uint8_t lut[256];
    fill_lut(lut);
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= a.s.n_tiles) return;
    const int64_t tile0 = tile * TILE, g0 = tile0 + lane * LANE;
    Period s[P];
    uint64_t rec[P];                       // the seeds that start in the lane, per period
    lane_records(a.s, lut, lane, tile, s, rec);
#pragma unroll
    for (int p = 1; p <= P; ++p) {
        const int mine = __builtin_popcountll(rec[p - 1]);
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, (unsigned)d, 64);
            if (lane >= d) incl += up;
        }
        if (!WRITE) {
            if (lane == 63) a.cnt[(p - 1) * a.s.n_tiles + tile] = (uint32_t)incl;
            continue;
        }
        int64_t at = a.base[p - 1] + a.soff[(p - 1) * (a.s.n_tiles + 1) + tile] + incl - mine;
        uint64_t m = rec[p - 1];
        while (m) {
            const int i = __builtin_ctzll(m);
            m &= m - 1;
            if (at < a.n_seeds) {                                  // (always: the list was sized from these counts)
                a.start[at] = (uint32_t)(g0 + i);
                a.len[at] = (uint32_t)(run_end(s[p - 1], i, g0, tile0) - (g0 + i) + p);
            }
            at += 1;
        }
    }
}

__device__ __forceinline__ int code_of(uint8_t c) {
    const int u = c & 0xDF;
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}

// the period of entry i of the seed list (empty lists have equal bounds)
__device__ __forceinline__ int period_of(const TractArgs& a, int64_t i) {
    int p = 1;
#pragma unroll
    for (int k = 1; k < P; ++k) p += i >= a.base[k];
    return p;
}

// the inclusive prefix sum of x over the workgroup's threads, the order of the additions fixed; lds: WAVES entries
__device__ __forceinline__ uint32_t block_incl_sum(uint32_t x, uint32_t* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(x, (unsigned)d, 64);
        if (lane >= d) x += up;
    }
    __syncthreads();                                               // (lds may still be read from the call before)
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    for (int v = 0; v < wave; ++v) x += lds[v];
    return x;
}

// a link byte as one number: the head bit in the upper half, the gap's mismatches in the lower (256 seeds of 64: 14 bits)
__device__ __forceinline__ uint32_t packed_of(uint32_t byte) { return ((byte & 1u) << 16) | (byte >> 1); }

__global__ __launch_bounds__(THREADS) void tract_link_kernel(TractArgs a) {
    __shared__ uint32_t lds[WAVES];
    const int64_t i = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
    uint32_t byte = 0;
    if (i < a.n_seeds) {
        const int p = period_of(a, i);
        uint32_t head = 1, mm = 0;
        if (i > a.base[p - 1]) {
            const int64_t a1 = a.start[i - 1], b1 = a1 + a.len[i - 1], a2 = a.start[i], g = a2 - b1;
            if (g >= 1 && g <= a.max_gap[p - 1] && a1 >= a.s.seg_off[upper_bound(a.s, a2) - 1]) {   // (a seed lies in one segment)
                const uint8_t* s = a.s.letters;
                const int phase = (int)((a2 - a1) % p);
                bool same = true;
                for (int j = 0; j < p; ++j) same = same && code_of(s[a2 + j]) == code_of(s[a1 + (phase + j) % p]);
                if (same) {
                    head = 0;
                    for (int64_t x = b1; x < a2; ++x) mm += code_of(s[x]) != code_of(s[a1 + (x - a1) % p]);
                }
            }
        }
        byte = head | (mm << 1);
        a.link[i] = (uint8_t)byte;
    }
    const uint32_t sum = block_incl_sum(packed_of(byte), lds);
    if (threadIdx.x == THREADS - 1) {
        a.blk_head[blockIdx.x] = sum >> 16;
        a.blk_mm[blockIdx.x] = sum & 0xFFFFu;
    }
}

__global__ __launch_bounds__(THREADS) void tract_heads_kernel(TractArgs a) {
    __shared__ uint32_t lds[WAVES];
    const int64_t i = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
    const uint32_t byte = i < a.n_seeds ? a.link[i] : 0;
    const uint32_t sum = block_incl_sum(packed_of(byte), lds);
    if (byte & 1u) {
        const int64_t t = a.off_head[blockIdx.x] + (sum >> 16) - 1;
        a.head_idx[t] = (uint32_t)i;
        a.head_mm[t] = (uint32_t)a.off_mm[blockIdx.x] + (sum & 0xFFFFu);
    }
}

template <bool WRITE>
__global__ __launch_bounds__(THREADS) void tract_records_kernel(TractArgs a) {
    __shared__ uint32_t lds[WAVES];
    const int64_t i = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
    const uint32_t byte = i < a.n_seeds ? a.link[i] : 0;
    const uint32_t sum = block_incl_sum(packed_of(byte), lds);
    const bool tail = i < a.n_seeds && (i + 1 == a.n_seeds || (a.link[i + 1] & 1u));
    uint32_t rec = 0, mm = 0, h = 0;
    int64_t first = 0, length = 0;
    int p = 1;
    if (tail) {
        const int64_t t = a.off_head[blockIdx.x] + (sum >> 16) - 1;
        h = a.head_idx[t];
        mm = (uint32_t)a.off_mm[blockIdx.x] + (sum & 0xFFFFu) - a.head_mm[t];   // (a tract's mismatches are below 2^30)
        p = period_of(a, i);
        first = a.start[h];
        length = (int64_t)a.start[i] + a.len[i] - first;
        rec = length / p >= a.min_copies[p - 1];
    }
    const uint32_t at = block_incl_sum(rec, lds);
    if (!WRITE) {
        if (threadIdx.x == THREADS - 1) a.blk_rec[blockIdx.x] = at;
        return;
    }
    if (!rec) return;
    const int64_t r = a.off_rec[blockIdx.x] + at - 1;
    const int seg = upper_bound(a.s, first) - 1;
    a.out_seg[r] = seg;
    a.out_start[r] = first - a.s.seg_off[seg];
    a.out_len[r] = (int32_t)length;
    a.out_period[r] = p;
    a.out_seeds[r] = (int32_t)(i - h + 1);
    a.out_mismatch[r] = (int32_t)mm;
}

struct State : StateBase {
    Dev seq, seg, work, seeds, out;        // the letters (whole tiles and 64 bytes), seg_off, the tiles' tables, the seeds' and the workgroups' tables, the records
};
Registry<State> g_states;

// off[r][0 .. n] = the exclusive prefix sum of count[r][0 .. n) for each of `rows` rows: scan_offsets_kernel over a table of
// this unit's
void launch_offsets(const ScanArgs& s, hipStream_t st, uint32_t* count, int64_t* off, int64_t n, int rows = 1) {
    ScanArgs o = s;
    o.count = count;
    o.off = off;
    o.n_tiles = n;
    hipLaunchKernelGGL(scan_offsets_kernel, dim3(rows), dim3(SCAN_THREADS), 0, st, o);
}

}  // namespace

extern "C" {

int tredtract_scan(tredgpu_ctx* ctx, const uint8_t* letters, const int64_t* seg_off, int32_t n_seg, const int32_t* min_copies,
                   const int32_t* seed_copies, const int32_t* max_gap, int64_t out_cap, int32_t* out_seg, int64_t* out_start,
                   int32_t* out_len, int32_t* out_period, int32_t* out_seeds, int32_t* out_mismatch, int64_t* out_n) {
    std::string& err = g_tract_error;
    err.clear();
    if (!ctx) return fail(err, -2, "ctx is NULL");
    if (!seg_off || !min_copies || !seed_copies || !max_gap || !out_n) return fail(err, -2, "NULL array argument");
    if (n_seg < 0) return fail(err, -2, "n_seg %d is negative", n_seg);
    if (out_cap < 0) return fail(err, -2, "out_cap %lld is negative", (long long)out_cap);
    if (out_cap > 0 && (!out_seg || !out_start || !out_len || !out_period || !out_seeds || !out_mismatch)) return fail(err, -2, "NULL array argument");
    if (seg_off[0] < 0) return fail(err, -2, "seg_off[0] is negative");
    for (int32_t k = 0; k < n_seg; ++k)
        if (seg_off[k + 1] < seg_off[k]) return fail(err, -2, "seg_off descends at segment %d", k);
    const int64_t n = seg_off[n_seg];
    if (n > TREDSCAN_MAX_LETTERS) return fail(err, -2, "%lld letters: more than TREDSCAN_MAX_LETTERS (%lld)", (long long)n, (long long)TREDSCAN_MAX_LETTERS);
    if (n > 0 && !letters) return fail(err, -2, "NULL array argument");
    bool any = false;
    for (int p = 0; p < P; ++p) {
        if (min_copies[p] == 1 || min_copies[p] < 0) return fail(err, -2, "min_copies[%d] is %d: 0 (off) or 2 and above", p, min_copies[p]);
        any = any || min_copies[p] > 0;
    }
    if (!any) return fail(err, -2, "every period is switched off");
    for (int p = 0; p < P; ++p) {
        if (min_copies[p] == 0) continue;
        if (seed_copies[p] < 2 || seed_copies[p] > min_copies[p])
            return fail(err, -2, "seed_copies[%d] is %d: 2 <= seed_copies <= min_copies (%d)", p, seed_copies[p], min_copies[p]);
        if (max_gap[p] < 0 || max_gap[p] > TREDTRACT_MAX_GAP)
            return fail(err, -2, "max_gap[%d] is %d: 0 <= max_gap <= TREDTRACT_MAX_GAP (%d)", p, max_gap[p], TREDTRACT_MAX_GAP);
        if ((int64_t)seed_copies[p] * (p + 1) <= (int64_t)max_gap[p] + 2 * (p + 1) - 2)
            return fail(err, -2, "period %d: seed_copies * p > max_gap + 2 p - 2 does not hold (seed_copies %d, max_gap %d)", p + 1, seed_copies[p], max_gap[p]);
    }

    hipStream_t st;
    int rc;
    if ((rc = select_device(err, ctx, st))) return rc;
    State& s = *g_states.state_of(ctx);
    TractArgs a{};
    a.s.n_seg = n_seg;
    a.s.first = seg_off[0];
    a.s.n = n;
    a.s.n_tiles = (n + TILE - 1) / TILE;
    for (int p = 0; p < P; ++p) {
        const bool on = min_copies[p] > 0;
        a.min_copies[p] = min_copies[p];
        a.max_gap[p] = on ? max_gap[p] : 0;
        a.s.min_copies[p] = on ? seed_copies[p] : 0;
        a.s.need[p] = on ? (int64_t)(seed_copies[p] - 1) * (p + 1) : -1;
    }
    // (The buffers, the events, timing and release are side_unit.h's; its staging list is not used, as in scan.hip: the
    //  room for the seeds and for the records is known only once a count has been read.)
    std::vector<int64_t> h_start;
    std::vector<int32_t> h_int;            // seg, len, period, seeds, mismatch: `total` entries each
    int64_t total = 0;
    if (a.s.n_tiles > 0) {
        const size_t tiles = (size_t)a.s.n_tiles;
        // fz and nz [P][tiles], soff [P][tiles + 1], cnt [P][tiles], last [tiles]: in this order, the widest first
        const size_t work = (3 * P * tiles + P) * sizeof(int64_t) + P * tiles * sizeof(uint32_t) + tiles;
        if ((rc = ensure(err, s.seq, tiles * TILE + 64, st))) return rc;
        if ((rc = ensure(err, s.seg, ((size_t)n_seg + 1) * sizeof(int64_t), st))) return rc;
        if ((rc = ensure(err, s.work, work, st))) return rc;
        a.s.letters = (const uint8_t*)s.seq.p;
        a.s.seg_off = (const int64_t*)s.seg.p;
        a.s.fz = (int64_t*)s.work.p;
        a.s.nz = a.s.fz + P * tiles;
        a.soff = a.s.nz + P * tiles;
        a.cnt = (uint32_t*)(a.soff + P * (tiles + 1));
        a.s.last = (uint8_t*)(a.cnt + P * tiles);
        SIDE_UNIT_CHK(err, hipMemcpyAsync(s.seq.p, letters, (size_t)n, hipMemcpyHostToDevice, st));
        SIDE_UNIT_CHK(err, hipMemcpyAsync(s.seg.p, seg_off, ((size_t)n_seg + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        const dim3 grid((unsigned)((tiles + WAVES - 1) / WAVES));
        if ((rc = timed_begin(err, s, st))) return rc;             // the event pair is around all launches of the call
        hipLaunchKernelGGL(scan_summary_kernel, grid, dim3(THREADS), 0, st, a.s);
        hipLaunchKernelGGL(scan_ends_kernel, dim3(P), dim3(SCAN_THREADS), 0, st, a.s);
        hipLaunchKernelGGL(tract_seeds_kernel<false>, grid, dim3(THREADS), 0, st, a);
        launch_offsets(a.s, st, a.cnt, a.soff, (int64_t)tiles, P);
        SIDE_UNIT_CHK(err, hipGetLastError());
        int64_t in_period[P];
        for (int p = 0; p < P; ++p)
            SIDE_UNIT_CHK(err, hipMemcpyAsync(&in_period[p], a.soff + p * (tiles + 1) + tiles, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        SIDE_UNIT_CHK(err, hipStreamSynchronize(st));
        for (int p = 0; p < P; ++p) a.base[p + 1] = a.base[p] + in_period[p];
        a.n_seeds = a.base[P];
        if (a.n_seeds > INT32_MAX) return fail(err, -2, "%lld seeds: more than 31 bits count", (long long)a.n_seeds);
        if (a.n_seeds > 0) {
            const size_t seeds = (size_t)a.n_seeds, blocks = (seeds + CHUNK - 1) / CHUNK;
            a.n_blocks = (int64_t)blocks;
            // off_head, off_mm, off_rec [blocks + 1]; start, len, head_idx, head_mm [seeds]; blk_head, blk_mm, blk_rec [blocks]; link [seeds]
            if ((rc = ensure(err, s.seeds, 3 * (blocks + 1) * sizeof(int64_t) + (4 * seeds + 3 * blocks) * sizeof(uint32_t) + seeds, st))) return rc;
            a.off_head = (int64_t*)s.seeds.p;
            a.off_mm = a.off_head + blocks + 1;
            a.off_rec = a.off_mm + blocks + 1;
            a.start = (uint32_t*)(a.off_rec + blocks + 1);
            a.len = a.start + seeds;
            a.head_idx = a.len + seeds;
            a.head_mm = a.head_idx + seeds;
            a.blk_head = a.head_mm + seeds;
            a.blk_mm = a.blk_head + blocks;
            a.blk_rec = a.blk_mm + blocks;
            a.link = (uint8_t*)(a.blk_rec + blocks);
            const dim3 sgrid((unsigned)blocks);
            hipLaunchKernelGGL(tract_seeds_kernel<true>, grid, dim3(THREADS), 0, st, a);
            hipLaunchKernelGGL(tract_link_kernel, sgrid, dim3(THREADS), 0, st, a);
            launch_offsets(a.s, st, a.blk_head, a.off_head, a.n_blocks);
            launch_offsets(a.s, st, a.blk_mm, a.off_mm, a.n_blocks);
            hipLaunchKernelGGL(tract_heads_kernel, sgrid, dim3(THREADS), 0, st, a);
            hipLaunchKernelGGL(tract_records_kernel<false>, sgrid, dim3(THREADS), 0, st, a);
            launch_offsets(a.s, st, a.blk_rec, a.off_rec, a.n_blocks);
            SIDE_UNIT_CHK(err, hipGetLastError());
            SIDE_UNIT_CHK(err, hipMemcpyAsync(&total, a.off_rec + blocks, sizeof total, hipMemcpyDeviceToHost, st));
            SIDE_UNIT_CHK(err, hipStreamSynchronize(st));
            if (total > 0) {
                // out_start [total], then out_seg, out_len, out_period, out_seeds and out_mismatch [total] each
                const size_t recs = (size_t)total;
                if ((rc = ensure(err, s.out, recs * (sizeof(int64_t) + 5 * sizeof(int32_t)), st))) return rc;
                a.out_start = (int64_t*)s.out.p;
                a.out_seg = (int32_t*)(a.out_start + recs);
                a.out_len = a.out_seg + recs;
                a.out_period = a.out_len + recs;
                a.out_seeds = a.out_period + recs;
                a.out_mismatch = a.out_seeds + recs;
                hipLaunchKernelGGL(tract_records_kernel<true>, sgrid, dim3(THREADS), 0, st, a);
            }
        }
        if ((rc = timed_end(err, s, st))) return rc;
        if (total > 0 && out_cap > 0) {
            h_start.resize((size_t)total);
            h_int.resize(5 * (size_t)total);
            SIDE_UNIT_CHK(err, hipMemcpyAsync(h_start.data(), a.out_start, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            SIDE_UNIT_CHK(err, hipMemcpyAsync(h_int.data(), a.out_seg, 5 * (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        SIDE_UNIT_CHK(err, hipStreamSynchronize(st));
    } else {                                                       // (a call without a letter is a call too)
        if ((rc = timed_begin(err, s, st))) return rc;
        if ((rc = timed_end(err, s, st))) return rc;
    }
    if (!h_start.empty()) {
        // The device's records are the six periods' lists one behind the other, each ascending by (segment, start): a
        // stable 6-way merge into (segment, start, period) order, of which the first out_cap are the caller's.
        const size_t recs = (size_t)total;
        const int32_t *seg = h_int.data(), *len = seg + recs, *period = len + recs, *seeds = period + recs, *mismatch = seeds + recs;
        size_t at[P + 1], end[P];
        at[0] = 0;
        for (int p = 1; p <= P; ++p) {
            at[p] = at[p - 1];
            while (at[p] < recs && period[at[p]] <= p) at[p] += 1;
            end[p - 1] = at[p];
        }
        const int64_t keep = std::min<int64_t>(total, out_cap);
        for (int64_t k = 0; k < keep; ++k) {
            int best = -1;
            for (int p = 0; p < P; ++p) {
                if (at[p] == end[p]) continue;
                if (best < 0 || seg[at[p]] < seg[at[best]] || (seg[at[p]] == seg[at[best]] && h_start[at[p]] < h_start[at[best]])) best = p;
            }
            const size_t r = at[best]++;
            out_seg[k] = seg[r];
            out_start[k] = h_start[r];
            out_len[k] = len[r];
            out_period[k] = period[r];
            out_seeds[k] = seeds[r];
            out_mismatch[k] = mismatch[r];
        }
    }
    *out_n = total;
    return 0;
}

int tredtract_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) { return timing(g_tract_error, g_states, ctx, launches, total_ms, false); }

int tredtract_reset_timing(tredgpu_ctx* ctx) { return timing(g_tract_error, g_states, ctx, nullptr, nullptr, true); }

void tredtract_release(tredgpu_ctx* ctx) { release(g_states, ctx, {&State::seq, &State::seg, &State::work, &State::seeds, &State::out}); }

const char* tredtract_last_error(void) { return g_tract_error.c_str(); }

}  // extern "C"
