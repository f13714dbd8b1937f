// scan.hip -- perfect tandem repeats of a letter sequence (tredscan_scan, include/tredscan.h): the maximal runs of every
// period 1 .. 6 with enough whole copies and a primitive motif, as records in (segment, start, period) order.  A unit of its
// own, outside the source hash the profiles are tied to (csrc/Makefile); the harness is side_unit.h's.
//
// The tiles, a lane's masks e_p, the summary and ends passes, the prefix sum of a table and a lane's records are scan_unit.h's,
// which tract.hip (include/tredtract.h) includes too.
//
// Three passes over the letters, each of which makes the masks again (they are cheaper to make than to store), and two
// small scans between them:
//   * scan_summary_kernel: per tile and period the position of the first 0 of e_p in the tile, or CONT where the tile is all
//     ones, and the last bit of the tile.
//   * scan_ends_kernel, one workgroup per period: from right to left over the tiles, the first 0 at or behind the start of
//     the NEXT tile -- where a run that is still open at a tile's end stops, however many tiles it goes on for.
//   * scan_records_kernel<false>: a lane's records (lane_records: run starts by mask arithmetic, ends from the lanes above or
//     scan_ends_kernel's table; no lane walks along a run: a satellite of a megabase costs what any other sequence costs)
//     as a mask per period; the tile's count is stored.
//   * scan_offsets_kernel, one workgroup: the exclusive prefix sum of the tiles' counts, and the total.
//   * scan_records_kernel<true>: the same masks again, a prefix sum over the lanes, and each record stored at its place.
// Temporary memory: 109 bytes per tile of 4096 letters.  All results leave through plain vector stores; no atomic.
#include <cstring>

#include "scan_unit.h"

namespace {
using namespace scan_unit;

thread_local std::string g_scan_error;     // the text of tredscan_last_error()

template <bool WRITE>
__global__ __launch_bounds__(THREADS) void scan_records_kernel(ScanArgs a) {
    __shared__ uint8_t lut[256];
    fill_lut(lut);
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;
    const int64_t tile0 = tile * TILE, g0 = tile0 + lane * LANE;
    Period s[P];
    uint64_t rec[P];                       // the records that start in the lane, per period
    const int mine = lane_records(a, lut, lane, tile, s, rec);
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, (unsigned)d, 64);
        if (lane >= d) incl += up;
    }
    if (!WRITE) {
        if (lane == 63) a.count[tile] = (uint32_t)incl;
        return;
    }
    int64_t at = a.off[tile] + incl - mine;
    uint64_t any = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) any |= rec[p];
    while (any) {
        const int i = __builtin_ctzll(any);
        any &= any - 1;
        const int64_t g = g0 + i;
        const int seg = upper_bound(a, g) - 1;                     // (a record's letter lies in a segment)
        const int64_t start = g - a.seg_off[seg];
#pragma unroll
        for (int p = 1; p <= P; ++p) {
            if (!((rec[p - 1] >> i) & 1ull)) continue;
            if (at < a.cap) {
                a.out_seg[at] = seg;
                a.out_start[at] = start;
                a.out_len[at] = (int32_t)(run_end(s[p - 1], i, g0, tile0) - g + p);
                a.out_period[at] = p;
            }
            at += 1;
        }
    }
}

struct State : StateBase {
    Dev seq, seg, work, out;               // the letters (whole tiles and 64 bytes), seg_off, the tiles' tables, the records
};
Registry<State> g_states;

size_t round_up(size_t x, size_t to) { return (x + to - 1) / to * to; }

}  // namespace

extern "C" {

int tredscan_scan(tredgpu_ctx* ctx, const uint8_t* letters, const int64_t* seg_off, int32_t n_seg, const int32_t* min_copies,
                  int64_t out_cap, int32_t* out_seg, int64_t* out_start, int32_t* out_len, int32_t* out_period, int64_t* out_n) {
    std::string& err = g_scan_error;
    err.clear();
    if (!ctx) return fail(err, -2, "ctx is NULL");
    if (!seg_off || !min_copies || !out_n) return fail(err, -2, "NULL array argument");
    if (n_seg < 0) return fail(err, -2, "n_seg %d is negative", n_seg);
    if (out_cap < 0) return fail(err, -2, "out_cap %lld is negative", (long long)out_cap);
    if (out_cap > 0 && (!out_seg || !out_start || !out_len || !out_period)) return fail(err, -2, "NULL array argument");
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

    hipStream_t st;
    int rc;
    if ((rc = select_device(err, ctx, st))) return rc;
    State& s = *g_states.state_of(ctx);
    ScanArgs a{};
    a.n_seg = n_seg;
    a.first = seg_off[0];
    a.n = n;
    a.n_tiles = (n + TILE - 1) / TILE;
    a.cap = out_cap;
    for (int p = 0; p < P; ++p) {
        a.min_copies[p] = min_copies[p];
        a.need[p] = min_copies[p] > 0 ? (int64_t)(min_copies[p] - 1) * (p + 1) : -1;
    }
    // (The buffers, the events, timing and release are side_unit.h's; its staging list is not used: the letters' buffer is
    //  longer than what is copied into it, and the room for the records is known only once the count has been read.)
    int64_t total = 0;
    if (a.n_tiles > 0) {
        const size_t tiles = (size_t)a.n_tiles;
        // fz and nz [P][tiles], off [tiles + 1], count [tiles], last [tiles]: in this order, the widest first
        const size_t work = (2 * P * tiles + tiles + 1) * sizeof(int64_t) + tiles * sizeof(uint32_t) + tiles;
        if ((rc = ensure(err, s.seq, tiles * TILE + 64, st))) return rc;
        if ((rc = ensure(err, s.seg, ((size_t)n_seg + 1) * sizeof(int64_t), st))) return rc;
        if ((rc = ensure(err, s.work, work, st))) return rc;
        a.letters = (const uint8_t*)s.seq.p;
        a.seg_off = (const int64_t*)s.seg.p;
        a.fz = (int64_t*)s.work.p;
        a.nz = a.fz + P * tiles;
        a.off = a.nz + P * tiles;
        a.count = (uint32_t*)(a.off + tiles + 1);
        a.last = (uint8_t*)(a.count + tiles);
        SIDE_UNIT_CHK(err, hipMemcpyAsync(s.seq.p, letters, (size_t)n, hipMemcpyHostToDevice, st));
        SIDE_UNIT_CHK(err, hipMemcpyAsync(s.seg.p, seg_off, ((size_t)n_seg + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        const dim3 grid((unsigned)((tiles + WAVES - 1) / WAVES));  // (2^30 letters: 65536 workgroups)
        if ((rc = timed_begin(err, s, st))) return rc;             // the event pair is around the five launches
        hipLaunchKernelGGL(scan_summary_kernel, grid, dim3(THREADS), 0, st, a);
        hipLaunchKernelGGL(scan_ends_kernel, dim3(P), dim3(SCAN_THREADS), 0, st, a);
        hipLaunchKernelGGL(scan_records_kernel<false>, grid, dim3(THREADS), 0, st, a);
        hipLaunchKernelGGL(scan_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, a);
        SIDE_UNIT_CHK(err, hipGetLastError());
        SIDE_UNIT_CHK(err, hipMemcpyAsync(&total, a.off + tiles, sizeof total, hipMemcpyDeviceToHost, st));
        SIDE_UNIT_CHK(err, hipStreamSynchronize(st));
        const size_t keep = (size_t)std::min<int64_t>(total, out_cap);
        if (keep > 0) {
            // out_start [keep], then out_seg, out_len and out_period [keep] each
            if ((rc = ensure(err, s.out, keep * (sizeof(int64_t) + 3 * sizeof(int32_t)), st))) return rc;
            a.out_start = (int64_t*)s.out.p;
            a.out_seg = (int32_t*)(a.out_start + keep);
            a.out_len = a.out_seg + keep;
            a.out_period = a.out_len + keep;
            a.cap = (int64_t)keep;
            hipLaunchKernelGGL(scan_records_kernel<true>, grid, dim3(THREADS), 0, st, a);
        }
        if ((rc = timed_end(err, s, st))) return rc;
        if (keep > 0) {
            SIDE_UNIT_CHK(err, hipMemcpyAsync(out_start, a.out_start, keep * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            SIDE_UNIT_CHK(err, hipMemcpyAsync(out_seg, a.out_seg, keep * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            SIDE_UNIT_CHK(err, hipMemcpyAsync(out_len, a.out_len, keep * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            SIDE_UNIT_CHK(err, hipMemcpyAsync(out_period, a.out_period, keep * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        SIDE_UNIT_CHK(err, hipStreamSynchronize(st));
    } else {                                                       // (a call without a letter is a call too)
        if ((rc = timed_begin(err, s, st))) return rc;
        if ((rc = timed_end(err, s, st))) return rc;
    }
    *out_n = total;
    return 0;
}

int tredscan_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) { return timing(g_scan_error, g_states, ctx, launches, total_ms, false); }

int tredscan_reset_timing(tredgpu_ctx* ctx) { return timing(g_scan_error, g_states, ctx, nullptr, nullptr, true); }

void tredscan_release(tredgpu_ctx* ctx) { release(g_states, ctx, {&State::seq, &State::seg, &State::work, &State::out}); }

const char* tredscan_last_error(void) { return g_scan_error.c_str(); }

}  // extern "C"
