// sw_cigar.hip -- the CIGAR of an alignment (include/tredcigar.h): the reference's banded_sw (src/ssw.c:549-736) restated
// cell for cell on the rectangle ref[ref_begin..ref_end] x read[read_begin..read_end] of an alignment the SW kernels
// have already placed.  A unit of its own, outside the source hash the profiles are tied to (csrc/Makefile).
//
// Mapping.  The pass is a serial recurrence three ways (E down the columns, F along the row, H on the diagonal) over a
// band that is 3-7 cells wide for most alignments, and the reference's result depends on the order and the storage of
// that recurrence (what a cell above the band's end reads, which stale entries a row overwrites), so the port keeps
// its three row arrays and its index arithmetic and gives ONE LANE ONE ITEM: 64 independent items per wavefront, no
// exchange between lanes, no barrier.
//   narrow tier (cigar_narrow_kernel): bands up to 65 cells (width_d) and width_d * readLen <= 16 384.  The three row
//     arrays (h_b, e_b, h_c: 68 int16 each) live in LDS, lane-interleaved ([entry][lane]: a wavefront's access to one
//     entry is 64 consecutive int16, no bank conflict): 3 * 68 * 64 * 2 = 26 112 bytes per wavefront, so six wavefronts
//     share a CU's 160 KB.  The direction plane -- the three codes of a cell in ONE byte: bit 0 E's (2/3), bit 1 F's
//     (4/5), bits 2-4 H's (1-5) -- is 16 KB per lane in a workspace the context owns, lane-interleaved as well
//     ([cell][lane]): a store of the wavefront is one 64-byte line.  Lanes take items grid-stride, so the workspace is
//     min(items, 16 384) lanes * 16 KB.
//   wide tier (cigar_wide_kernel): an item whose band outgrows that (an indel of more than 32 bases, a long read whose
//     band doubled to 33, fields that do not belong to the pair) is put on a list by the narrow kernel and done by one
//     wavefront of 64 lanes with rows and plane in global memory: 1 026 entries per row array and 1 021 * 480 bytes of
//     plane per lane (the band stops doubling once it covers the rectangle), 31 MB in all.
#include "cigar_unit.h"

namespace {
using namespace cigar_unit;

struct CigarArgs : Args {  // plane: narrow [wavefront][cell][lane]; wide [lane][cell]
    int16_t* wide_rows;    // wide: [lane][3][WIDE_ROW]
    int32_t* wide_list;    // items the narrow kernel hands on; wide_list[n_items] is their count
};

constexpr int NARROW_ROW = 68;            // entries per row array: width = 2 * band + 3 <= 67
constexpr int NARROW_PLANE = 16384;       // cells of direction plane per lane
constexpr int NARROW_MAX_LANES = 16384;
constexpr int WIDE_ROW = 1026;            // width <= 2 * 511 + 3
constexpr int WIDE_PLANE = 1021 * 480 + 1023;
constexpr int WIDE_LANES = 64;
constexpr int NEEDS_WIDE = -1;

// the storage of one lane's pass: entry k of a row array is rows[(row * row_len + k) * rs], cell c is plane[c * ps]
struct Store {
    int16_t* rows;
    int rs, row_len;
    uint8_t* plane;
    size_t ps;
    int plane_cap;
    __device__ int16_t& hb(int k) const { return rows[(size_t)k * rs]; }
    __device__ int16_t& eb(int k) const { return rows[(size_t)(row_len + k) * rs]; }
    __device__ int16_t& hc(int k) const { return rows[(size_t)(2 * row_len + k) * rs]; }
    __device__ uint8_t& cell(int c) const { return plane[(size_t)c * ps]; }
};

// set_u / set_d of ssw.c:55-58: the band coordinate of column j in row i
__device__ __forceinline__ int band_x(int w, int i, int j) {
    const int x = i - w;
    return j - (x > 0 ? x : 0);
}

// the pass and the traceback of an item the decode accepted; NEEDS_WIDE when a pass does not fit the store (nothing has been
// written to the outputs then)
__device__ int cigar_pass(const CigarArgs& a, int64_t item, const Item& it, const Store& st) {
    const int score = it.score, ref_begin = it.ref_begin, read_begin = it.read_begin, trunk = it.trunk;
    const int refLen = it.refLen, readLen = it.readLen;
    const uint8_t *tr = it.tr, *br = it.br;
    const int gO = a.gap_open, gE = a.gap_extend;
    const int cover = max(refLen, readLen) - 1;
    int bw = abs(refLen - readLen) + 1;
    int best = 0, width_d;

    for (;;) {                                                        // ssw.c:572-633
        const int width = bw * 2 + 3;
        width_d = bw * 2 + 1;
        if (width > st.row_len - 1 || width_d * readLen > st.plane_cap) return NEEDS_WIDE;
        for (int j = 1; j < width - 1; ++j) st.hb(j) = 0;
        for (int i = 0; i < readLen; ++i) {
            const int ri = read_begin + i;
            const int q = read_code(it.rec, it.nb, ri);
            const int beg = max(0, i - bw), end = min(refLen - 1, i + bw);
            const int edge = min(end + 1, width - 1);
            int f = 0, u = 0;
            st.hb(0) = 0; st.eb(0) = 0; st.hb(edge) = 0; st.eb(edge) = 0; st.hc(0) = 0;
            const int x0 = max(i - bw, 0), x1 = max(i - 1 - bw, 0);    // band origins of this row and the one above
            for (int j = beg; j <= end; ++j) {
                u = j - x0 + 1;
                const int e = j - x1 + 1, b = u - 1, dg = e - 1;
                int t1 = (i == 0 ? 0 : (int)st.hb(e)) - gO;
                int t2 = (i == 0 ? 0 : (int)st.eb(e)) - gE;
                const int ev = t1 > t2 ? t1 : t2;
                st.eb(u) = (int16_t)ev;
                const int de = t1 > t2 ? 3 : 2;
                t1 = st.hc(b) - gO;
                t2 = f - gE;
                f = t1 > t2 ? t1 : t2;
                const int df = t1 > t2 ? 5 : 4;
                const int e1 = ev > 0 ? ev : 0, f1 = f > 0 ? f : 0;
                t1 = e1 > f1 ? e1 : f1;
                const int rj = ref_begin + j;
                const int r = rj < trunk ? tr[rj] : br[rj - trunk];
                t2 = st.hb(dg) + ((r == 4 || q == 4) ? 0 : r == q ? a.match : -a.mismatch);
                const int h = t1 > t2 ? t1 : t2;
                st.hc(u) = (int16_t)h;
                best = h > best ? h : best;
                const int dh = t1 <= t2 ? 1 : (e1 > f1 ? de : df);
                st.cell(width_d * i + (j - x0)) = dir_pack(de, df, dh);
            }
            for (int j = 1; j <= u; ++j) st.hb(j) = st.hc(j);
        }
        if (best >= score) break;
        if (bw >= cover) return TREDGPU_CIGAR_NO_PATH;
        bw = min(bw * 2, cover);              // every band that covers the rectangle computes the same cells
    }

    return traceback(a, item, it, bw, [&](int i, int j) { return (int)st.cell(width_d * i + band_x(bw, i, j)); });
}

// one item, start to end
__device__ int cigar_item(const CigarArgs& a, int64_t item, const Store& st) {
    return decode_item(a, item, TREDGPU_MAX_READ_LEN, TREDGPU_MAX_TEMPLATE_LEN,
                       [&](const Item& it) { return cigar_pass(a, item, it, st); });
}

__device__ void cigar_finish(const CigarArgs& a, int64_t item, int status) {
    store_status(a, item, status);
    if (status != TREDGPU_CIGAR_OK) zero_ops(a, item, 0, 1);
}

__global__ __launch_bounds__(64) void cigar_narrow_kernel(CigarArgs a) {
    __shared__ int16_t rows[3 * NARROW_ROW * 64];
    const int lane = threadIdx.x;
    Store st;
    st.rows = rows + lane;
    st.rs = 64;
    st.row_len = NARROW_ROW;
    st.plane = a.plane + (size_t)blockIdx.x * 64 * NARROW_PLANE + lane;
    st.ps = 64;
    st.plane_cap = NARROW_PLANE;
    for (int64_t item = (int64_t)blockIdx.x * 64 + lane; item < a.n_items; item += (int64_t)gridDim.x * 64) {
        zero_ops(a, item, 0, 1);
        const int status = cigar_item(a, item, st);
        if (status == NEEDS_WIDE) a.wide_list[atomicAdd(&a.wide_list[a.n_items], 1)] = (int32_t)item;
        else cigar_finish(a, item, status);
    }
}

__global__ __launch_bounds__(64) void cigar_wide_kernel(CigarArgs a) {
    const int lane = threadIdx.x;
    Store st;
    st.rows = a.wide_rows + (size_t)lane * 3 * WIDE_ROW;
    st.rs = 1;
    st.row_len = WIDE_ROW;
    st.plane = a.plane + (size_t)lane * WIDE_PLANE;
    st.ps = 1;
    st.plane_cap = WIDE_PLANE;
    const int n = a.wide_list[a.n_items];
    for (int k = lane; k < n; k += WIDE_LANES) {
        const int64_t item = a.wide_list[k];
        const int status = cigar_item(a, item, st);
        cigar_finish(a, item, status == NEEDS_WIDE ? TREDGPU_CIGAR_TOO_LONG : status);
    }
}

// ---- host side (side_unit.h) --------------------------------------------------------------------------------------------
thread_local std::string g_cigar_error;

struct State : StateBase { Dev narrow_plane, wide_plane, wide_rows, wide_list; };
Registry<State> g_states;

}  // namespace

extern "C" {

const char* tredcigar_last_error(void) { return g_cigar_error.c_str(); }

int tredcigar_sw_cigar(tredgpu_ctx* ctx, int mem, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                       const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                       const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                       const int16_t* fields, const tredgpu_sw_params* p, int32_t cap, uint32_t* out_ops,
                       int32_t* out_n_ops, int32_t* out_status) {
    std::string& err = g_cigar_error;
    err.clear();
    const bool host = mem == TREDGPU_MEM_HOST;
    const Table t{n_ladders, prefix, repeat, suffix, max_units};
    int rc = call_refusal(err, ctx, host || mem == TREDGPU_MEM_DEVICE, t, n_items, cap, p,
                          {packed, read_off, read_len, item_ladder, item_template, fields, out_ops, out_n_ops, out_status});
    if (rc || n_items == 0) return rc;
    hipStream_t st;
    if ((rc = select_device(err, ctx, st))) return rc;
    State* s = g_states.state_of(ctx);
    if ((rc = set_ladders(err, *s, st, t, 0))) return rc;

    const size_t n = (size_t)n_items;
    CigarArgs a{};
    fill_args(a, *s, packed, read_off, read_len, n_items, item_ladder, item_template, fields, *p, cap, out_ops, out_n_ops, out_status);
    std::vector<Array> arrays;                                   // device memory: nothing is staged
    if (host) {
        if ((rc = reads_refusal(err, read_off, read_len, n, -1))) return rc;
        arrays = host_arrays(a);
        if ((rc = stage(err, *s, st, arrays))) return rc;
    }
    const int blocks = (int)std::min<size_t>((n + 63) / 64, NARROW_MAX_LANES / 64);
    if ((rc = ensure(err, s->narrow_plane, (size_t)blocks * 64 * NARROW_PLANE, st))) return rc;
    if ((rc = ensure(err, s->wide_plane, (size_t)WIDE_LANES * WIDE_PLANE, st))) return rc;
    if ((rc = ensure(err, s->wide_rows, (size_t)WIDE_LANES * 3 * WIDE_ROW * sizeof(int16_t), st))) return rc;
    if ((rc = ensure(err, s->wide_list, (n + 1) * sizeof(int32_t), st))) return rc;
    a.wide_list = (int32_t*)s->wide_list.p;
    a.wide_rows = (int16_t*)s->wide_rows.p;
    SIDE_UNIT_CHK(err, hipMemsetAsync(a.wide_list + n, 0, sizeof(int32_t), st));
    SIDE_UNIT_CHK(err, hipMemsetAsync(a.out_n_ops, 0, n * sizeof(int32_t), st));
    if ((rc = timed_begin(err, *s, st))) return rc;
    a.plane = (uint8_t*)s->narrow_plane.p;
    hipLaunchKernelGGL(cigar_narrow_kernel, dim3(blocks), dim3(64), 0, st, a);
    SIDE_UNIT_CHK(err, hipGetLastError());
    a.plane = (uint8_t*)s->wide_plane.p;
    hipLaunchKernelGGL(cigar_wide_kernel, dim3(1), dim3(WIDE_LANES), 0, st, a);
    if ((rc = timed_end(err, *s, st))) return rc;
    return host ? read_back(err, *s, st, arrays) : 0;
}

int tredcigar_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) { return timing(g_cigar_error, g_states, ctx, launches, total_ms, false); }

int tredcigar_reset_timing(tredgpu_ctx* ctx) { return timing(g_cigar_error, g_states, ctx, nullptr, nullptr, true); }

void tredcigar_release(tredgpu_ctx* ctx) {
    release(g_states, ctx, {&State::narrow_plane, &State::wide_plane, &State::wide_rows, &State::wide_list});
}

}  // extern "C"
