// sw_second.hip -- the second-best alignment of ssw_align (tredsecond_sw_second, include/tredsecond.h): score1 /
// ref_end1 / score2 / ref_end2 of a (read, template) pair as the reference's src/ssw.c reports them, for reads of up to
// TREDGPU_MAX_LONG_READ_LEN bp on templates of up to TREDGPU_MAX_LONG_TEMPLATE_LEN columns.  A unit of its own, outside
// the source hash the profiles are tied to (csrc/Makefile).  The header has the four rules the values follow.
//
// Mapping.  ONE WAVEFRONT takes one item; the items of a call are sorted into row classes by the host and a class's
// items are taken grid-stride by at most MAX_WAVES wavefronts of that class's kernel.
//   * lane l holds the R consecutive rows l * R .. l * R + R - 1, R = 1, 2, 4, 8, 16, 32 for reads whose 16-row padding
//     ends at 64, 128, 256, 512, 1 024, 2 048 rows: a 150 bp read (160 rows) has R = 4 and 40 busy lanes where R = 8
//     would leave 44 of 64 idle.
//   * the columns of the item's own template are swept once: trunk letters up to the template's unit, then the branch.
//     A column is sw_long.hip's formulation in plain int32 without a start payload: every value is score + (row + col) *
//     gap_extend, so that E is a running max along the row and F a running max down the column; F enters a lane as an
//     exclusive max scan over the wave of the lanes' (H - (gap_open - gap_extend)) maxima -- exact because gap_extend <=
//     gap_open (scoring_refusal).  The scan, the diagonal hand-over and the column maxima use __shfl_up / __shfl_xor
//     (ds_bpermute), as sw_long.hip does: that form is the one this project has pinned against the reference on this
//     compiler; DPP row operations would take the LDS crossbar out of the ~20 dependent steps of a column and are the
//     first thing to try for speed (DESIGN, "Second-best alignment").
//   * rows L .. round16(L) - 1 are padding rows scoring 0 against every letter (the code of N) -- not the long kernel's
//     -16 -- and rows from round16(L) on are computed and never looked at (no row depends on a row below it).
//   * both of the reference's passes come out of the one sweep, since the rows below round8(L) do not depend on those
//     under them: colw[c] is the column maximum over rows < round8(L) (the word pass's maxColumn), colb[c] over rows <
//     round16(L) (the byte pass's).  Both live in LDS as uint16 (2 x 4 096 x 2 = 16 KB; 16 384 is the largest score):
//     one wave reduction per column for colw, and for the at most 8 further rows -- which lie in 8 / R adjacent lanes, or
//     in one -- a reduction over those lanes and one v_readlane.
//   * after the sweep score1 / ref_end1 are the wave-wide arg-max of colw[c] << 16 | (0xFFFF - c) (the first column that
//     reaches the maximum), rule 2 picks the array and rule 3 is the same arg-max over the allowed columns.
//   * nothing is written to global memory but the item's four values and its status.
#include "side_unit.h"
#include "../../include/tredlong.h"
#include "../../include/tredsecond.h"

namespace {
using namespace side_unit;

thread_local std::string g_second_error;   // the text of tredsecond_last_error()

// wavefronts of a class's launch at the most: ten 16 KB workgroups fit a CU's 160 KB of LDS, 256 CUs.  A column is a chain
// of dependent cross-lane steps, so a SIMD with one wavefront mostly waits: 1 024 wavefronts took 8.1 ms for the 103 691
// items of tools/second_bench.py (DESIGN has the figure with 2 560)
constexpr int MAX_WAVES = 2560;
constexpr int N_CLASSES = 6;               // R = 1 << class
constexpr int SNEG = -(1 << 29);
constexpr int COLS = 4096;                 // entries of a column-maximum array: c < TREDGPU_MAX_LONG_TEMPLATE_LEN
static_assert(COLS > TREDGPU_MAX_LONG_TEMPLATE_LEN && (64 << (N_CLASSES - 1)) >= TREDGPU_MAX_LONG_READ_LEN,
              "the arrays and the largest row class hold the long path's limits");

struct SecondArgs {
    const uint32_t* packed;
    const int64_t* read_off;
    const int32_t *read_len, *item_ladder, *item_template, *mask_len;
    const LadderRecord* ladders;
    const uint8_t* letters;
    int32_t n_ladders;
    int32_t match, mismatch, gap_open, gap_extend;
    const int32_t* list;       // the items of this launch's row class
    int32_t n_list;
    int32_t* out;              // [n_items][4]
    int32_t* out_status;
};

__device__ __forceinline__ int wave_max(int x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x = max(x, __shfl_xor(x, d, 64));
    return x;
}

// One DP column for this lane's R rows; returns through mw / mb the lane's maxima over its first nw / nb rows, as plain
// scores (0 where it has no such row).
template <int R>
__device__ __forceinline__ void second_column(const uint32_t (&code)[(R + 3) / 4], int (&H)[R], int (&E)[R], int row0, int col,
                                              uint32_t lut, int ge, int c0, int nw, int nb, int& mw, int& mb) {
    const int lane = threadIdx.x;
    // H of the row above this lane's first row, previous column; above row 0 lies the floor of (-1, col - 1)
    int diag = __shfl_up(H[R - 1], 1u, 64);
    if (lane == 0) diag = (col - 2) * ge;
    const int s_fix = 2 * ge - 16;
    const int zhi = (row0 + col) * ge;
    int run = SNEG;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t off = (code[r >> 2] >> ((r & 3) * 8)) & 0xFFu;
        const int s = (int)((lut >> off) & 31u) + s_fix;
        const int v = max(max(diag + s, zhi + r * ge), E[r]);   // the diagonal, the floor (score 0), E
        diag = H[r];
        H[r] = v;                                               // without the vertical-gap term for now
        const int q = v - c0;
        run = max(run, q);
        E[r] = max(E[r], q);                                    // E of the next column
    }
    // exclusive max scan over the 64 lanes: F entering this lane from the rows above it
    int F = wave_excl_max(run, lane, SNEG);
    int m8 = SNEG, w = SNEG, b = SNEG;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int ht = H[r];
        H[r] = max(ht, F);
        F = max(F, ht - c0);
        m8 = max(m8, H[r] - r * ge);
        if ((r & 7) == 7 || r == R - 1) {                       // nw and nb are multiples of min(R, 8)
            if (r < nw) w = max(w, m8);
            if (r < nb) b = max(b, m8);
            m8 = SNEG;
        }
    }
    mw = max(w - zhi, 0);
    mb = max(b - zhi, 0);
}

// the four values of an item on one wavefront; every lane returns the status, lane 0's res is the result
template <int R>
__device__ int second_item(const SecondArgs& a, int64_t item, uint16_t* colw, uint16_t* colb, int (&res)[4]) {
    const int lane = threadIdx.x;
    const int lad = a.item_ladder[item], tpl = a.item_template[item], L = a.read_len[item];
    Template t;
    if (!template_of(a, lad, tpl, t) || L < 0) return TREDGPU_SECOND_BAD_ITEM;
    const int trunk = t.trunk, tlen = t.tlen;
    if (L > TREDGPU_MAX_LONG_READ_LEN || L > 64 * R || tlen > TREDGPU_MAX_LONG_TEMPLATE_LEN) return TREDGPU_SECOND_TOO_LONG;
    const uint8_t *tr = t.tr, *br = t.br;
    const uint32_t* rec = a.packed + a.read_off[item];
    const int nb_words = (L + 15) >> 4;
    const int ge = a.gap_extend, c0 = a.gap_open - a.gap_extend;

    const int row0 = lane * R;
    const int P8 = (L + 7) & ~7, P16 = (L + 15) & ~15;
    const int nw = min(max(P8 - row0, 0), R), nb = min(max(P16 - row0, 0), R);
    uint32_t code[(R + 3) / 4];
    int H[R], E[R];
#pragma unroll
    for (int k = 0; k < (R + 3) / 4; ++k) code[k] = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = row0 + r;
        const int c = i < L ? read_code(rec, nb_words, i) : 4;       // a padding row scores like N
        code[r >> 2] |= (uint32_t)(5 * c) << ((r & 3) * 8);
        H[r] = (i - 1) * ge;                                         // the floor of column -1
        E[r] = SNEG;
    }
    const uint32_t lut0 = score_lut(0, a.match, a.mismatch), lut1 = score_lut(1, a.match, a.mismatch),
                   lut2 = score_lut(2, a.match, a.mismatch), lut3 = score_lut(3, a.match, a.mismatch),
                   lut4 = score_lut(4, a.match, a.mismatch);
    // the lanes that hold the rows round8(L) .. round16(L) - 1: G adjacent ones from lane P8 / R on
    constexpr int G = R >= 8 ? 1 : 8 / R;
    const bool extra = P16 > P8;
    const int extra_lane = extra ? P8 / R : 0;

    for (int cbase = 0; cbase < tlen; cbase += 64) {
        const int cc = cbase + lane;
        const int letv = cc < tlen ? (cc < trunk ? tr[cc] : br[cc - trunk]) : 4;
        const int n = min(64, tlen - cbase);
#pragma unroll 1
        for (int k = 0; k < n; ++k) {                               // (a column depends on the one before: nothing to overlap)
            const int let = __builtin_amdgcn_readlane(letv, k);
            const uint32_t lut = let == 0 ? lut0 : let == 1 ? lut1 : let == 2 ? lut2 : let == 3 ? lut3 : lut4;
            int mw, mb;
            second_column<R>(code, H, E, row0, cbase + k, lut, ge, c0, nw, nb, mw, mb);
            const int cw = wave_max(mw);
            int xb = mb;
#pragma unroll
            for (int dd = 1; dd < G; dd <<= 1) xb = max(xb, __shfl_xor(xb, dd, 64));
            const int cb = extra ? max(cw, __builtin_amdgcn_readlane(xb, extra_lane)) : cw;
            if (lane == 0) { colw[cbase + k] = (uint16_t)cw; colb[cbase + k] = (uint16_t)cb; }
        }
    }
    __syncthreads();

    // score1 / ref_end1: the first column that reaches the maximum
    uint32_t k1 = 0;
    for (int c = lane; c < tlen; c += 64) {
        const uint32_t v = colw[c];
        if (v) k1 = max(k1, v << 16 | (uint32_t)(0xFFFF - c));
    }
    k1 = (uint32_t)wave_max((int)k1);                               // (a score is below 2^15)
    const int score1 = (int)(k1 >> 16);
    const int end1 = score1 ? 0xFFFF - (int)(k1 & 0xFFFFu) : -1;
    const bool byte_pass = score1 + a.mismatch < 255;
    const uint16_t* colmax = byte_pass ? colb : colw;
    const int mask = min(a.mask_len[item], 1 << 16);
    const int left = max(end1 - mask, 0);
    const int right = min(end1 + mask, tlen) + (byte_pass ? 1 : 0);
    uint32_t k2 = 0;
    for (int c = lane; c < tlen; c += 64) {
        const uint32_t v = colmax[c];
        if (v && (c < left || c >= right)) k2 = max(k2, v << 16 | (uint32_t)(0xFFFF - c));
    }
    k2 = (uint32_t)wave_max((int)k2);
    const int score2 = (int)(k2 >> 16);
    res[0] = score1;
    res[1] = end1;
    res[2] = mask < 15 ? 0 : score2;
    res[3] = mask < 15 ? -1 : score2 ? 0xFFFF - (int)(k2 & 0xFFFFu) : 0;
    return TREDGPU_SECOND_OK;
}

template <int R>
__global__ __launch_bounds__(64) void second_kernel(SecondArgs a) {
    __shared__ uint16_t colw[COLS], colb[COLS];
    for (int k = blockIdx.x; k < a.n_list; k += gridDim.x) {
        const int64_t item = a.list[k];
        int res[4] = {0, 0, 0, 0};
        __syncthreads();                                            // the item before has read the arrays
        const int status = second_item<R>(a, item, colw, colb, res);
        if (threadIdx.x == 0) {
            for (int v = 0; v < 4; ++v) a.out[item * 4 + v] = status == TREDGPU_SECOND_OK ? res[v] : 0;
            a.out_status[item] = status;
        }
    }
}

struct State : StateBase {};
Registry<State> g_states;

}  // namespace

extern "C" {

int tredsecond_sw_second(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                         const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                         const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                         const int32_t* mask_len, const tredgpu_sw_params* p, int32_t* out, int32_t* out_status) {
    std::string& err = g_second_error;
    err.clear();
    const Table t{n_ladders, prefix, repeat, suffix, max_units};
    int rc = call_refusal(err, ctx, true, t, n_items, 1, p,
                          {packed, read_off, read_len, item_ladder, item_template, mask_len, out, out_status});
    if (rc || n_items == 0) return rc;
    const size_t n = (size_t)n_items;
    if ((rc = reads_refusal(err, read_off, read_len, n, TREDGPU_MAX_LONG_READ_LEN))) return rc;
    hipStream_t st;
    if ((rc = select_device(err, ctx, st))) return rc;
    State& s = *g_states.state_of(ctx);
    if ((rc = set_ladders(err, s, st, t, 0))) return rc;           // (a template beyond the limit is the item's TOO_LONG)

    // the items by row class; one the kernel refuses by its read's length goes to the first
    std::vector<int32_t> list;
    std::vector<int64_t> first;
    bucket_order(n, N_CLASSES, [&](size_t k) {
        const int L = read_len[k];
        int c = 0;
        while (c < N_CLASSES - 1 && L > (64 << c)) ++c;
        return L < 0 || L > TREDGPU_MAX_LONG_READ_LEN ? 0 : c;
    }, list, first);

    SecondArgs a{};
    fill_table(a, s, *p);
    const int32_t* d_list = nullptr;
    const std::vector<Array> arrays = {
        arr_in(a.packed, packed, (size_t)read_off[n]), arr_in(a.read_off, read_off, n + 1), arr_in(a.read_len, read_len, n),
        arr_in(a.item_ladder, item_ladder, n), arr_in(a.item_template, item_template, n), arr_in(a.mask_len, mask_len, n),
        arr_in(d_list, list.data(), n), arr_out(a.out, out, n * 4), arr_out(a.out_status, out_status, n)};
    if ((rc = stage(err, s, st, arrays))) return rc;

    if ((rc = timed_begin(err, s, st))) return rc;
    auto launch = [&](int c, auto kernel) {
        a.list = d_list + first[c];
        a.n_list = (int32_t)(first[c + 1] - first[c]);
        if (a.n_list) hipLaunchKernelGGL(kernel, dim3((unsigned)std::min(a.n_list, MAX_WAVES)), dim3(64), 0, st, a);
    };
    launch(0, second_kernel<1>);
    launch(1, second_kernel<2>);
    launch(2, second_kernel<4>);
    launch(3, second_kernel<8>);
    launch(4, second_kernel<16>);
    launch(5, second_kernel<32>);
    if ((rc = timed_end(err, s, st))) return rc;
    return read_back(err, s, st, arrays);                          // (list is read by its copy until the stream is drained)
}

int tredsecond_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) { return timing(g_second_error, g_states, ctx, launches, total_ms, false); }

int tredsecond_reset_timing(tredgpu_ctx* ctx) { return timing(g_second_error, g_states, ctx, nullptr, nullptr, true); }

void tredsecond_release(tredgpu_ctx* ctx) { release(g_states, ctx, {}); }

const char* tredsecond_last_error(void) { return g_second_error.c_str(); }

}  // extern "C"
