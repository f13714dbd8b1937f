// sw_cigar_long.hip -- the CIGAR of a long alignment (tredlong_sw_cigar, include/tredlong.h): sw_cigar.hip's contract --
// the reference's banded_sw (src/ssw.c:549-736) cell for cell -- for reads of up to TREDGPU_MAX_LONG_READ_LEN bp on
// templates of up to TREDGPU_MAX_LONG_TEMPLATE_LEN columns.  A unit of its own, outside the source hash the profiles are
// tied to (csrc/Makefile).
//
// Mapping.  sw_cigar.hip gives one lane one item, which is right for bands of 3-7 cells and seconds per item for a
// rectangle of 8.4 M cells.  Here ONE WAVEFRONT takes one item and its 64 lanes lie across the band of a row:
//   * a row is done in chunks of 64 band columns.  All of a row's loads (h_b[e], e_b[e], h_b[d]) read what the rows
//     before left: the serial loop writes e_b[u] with u <= e and h_b only after the row, so chunk after chunk, loads
//     before stores, is the serial order.  H goes to h_c and is copied to h_b after the row, as the reference does it
//     (entries behind the row's last cell keep what older rows left there).
//   * E and the diagonal term are per column.  F is one max-scan along the row: with G_j = F_j + j * gE,
//     G_j = max(G_beg, max_{k<j} (H~_k - gO + (k + 1) * gE)), H~ = max(e1, diag), G_beg = -gE + beg * gE -- exact because
//     gE <= gO (scoring_refusal), so F_{j-1} - gO never beats F_{j-1} - gE.  Inside a chunk it is a wave-level inclusive
//     max-scan (six shuffles), between chunks a carried maximum.  F's direction is 5 where G_j > G_{j-1}.
//     tests/cigar_rowpar_model.py is this form in NumPy, compared with the serial model cell for cell.
//   * the three row arrays (h_b, e_b, h_c: int16, refLen + 2 <= 4 097 live entries) and the rectangle's reference
//     letters are in LDS: 3 * 8 200 + 4 096 bytes, 28 704 with alignment, per wavefront: five wavefronts in a CU's 160 KB.
//   * the direction plane -- sw_cigar.hip's byte per cell -- is in global memory, row i at i * stride, stride =
//     min(2 * band + 1, refLen): a chunk's store is 64 consecutive bytes.  A slot owns plane for the call's largest
//     rectangle (cigar_long_plan.h), the context keeps the workspace (grow-only, 1 GiB at the most).
//   * the traceback is lane 0's; items are taken grid-stride by at most cigar_long_plan::SLOTS wavefronts.
#include "cigar_long_plan.h"
#include "cigar_unit.h"
#include "../../include/tredlong.h"

namespace tredgpu {
extern thread_local std::string g_long_error;   // sw_long.hip: the text of tredlong_last_error()
void long_classify_release(tredgpu_ctx* ctx);   // sw_long.hip: what tredlong_sw_classify holds for the context
}

namespace {
using namespace cigar_unit;
using tredgpu::g_long_error;

static_assert(cigar_long_plan::MAX_READ == TREDGPU_MAX_LONG_READ_LEN && cigar_long_plan::MAX_TEMPLATE == TREDGPU_MAX_LONG_TEMPLATE_LEN,
              "cigar_long_plan.h restates the limits of tredlong.h");

struct LongCigarArgs : Args {  // plane: [slot][slot_bytes]
    size_t slot_bytes;
};

constexpr int ROW = 4100;                 // entries per row array: e <= refLen + 1, edge <= refLen
constexpr int LNEG = -(1 << 29);

// the passes and the traceback of an item the decode accepted, on one wavefront; every lane returns the status
__device__ int long_cigar_item(const LongCigarArgs& a, int64_t item, const Item& it, uint8_t* plane, int16_t* hb, int16_t* eb,
                               int16_t* hc, uint8_t* refc) {
    const int lane = threadIdx.x;
    const int score = it.score, ref_begin = it.ref_begin, read_begin = it.read_begin, trunk = it.trunk;
    const int refLen = it.refLen, readLen = it.readLen;
    if ((size_t)refLen * readLen > a.slot_bytes) return TREDGPU_CIGAR_TOO_LONG;   // (the host sized the slot from these fields)
    const uint8_t *tr = it.tr, *br = it.br;
    const int gO = a.gap_open, gE = a.gap_extend;
    for (int c = lane; c < refLen; c += 64) {
        const int rj = ref_begin + c;
        refc[c] = rj < trunk ? tr[rj] : br[rj - trunk];
    }
    const int cover = max(refLen, readLen) - 1;
    int bw = abs(refLen - readLen) + 1;
    int best = 0, stride;

    for (;;) {                                                        // ssw.c:572-633
        const int width = bw * 2 + 3;
        stride = min(bw * 2 + 1, refLen);
        __syncthreads();
        for (int j = 1 + lane; j < min(width - 1, refLen + 2); j += 64) hb[j] = 0;
        int lane_best = 0;
        for (int i = 0; i < readLen; ++i) {
            const int ri = read_begin + i;
            const int q = read_code(it.rec, it.nb, ri);
            const int beg = max(0, i - bw), end = min(refLen - 1, i + bw);
            const int edge = min(end + 1, width - 1);
            const int s = beg - max(i - 1 - bw, 0);                   // the band's origin moved with this row (0 / 1)
            const int ncell = end - beg + 1;
            __syncthreads();                                          // the copy of the row before (the zeroing, in row 0)
            if (lane == 0) { hb[0] = 0; eb[0] = 0; hb[edge] = 0; eb[edge] = 0; }
            __syncthreads();
            uint8_t* prow = plane + (size_t)i * stride;
            int carry = -gE + beg * gE, prev_g = carry;               // F of the row's first cell is 0 - gE, direction 4
            for (int c0 = 0; c0 < ncell; c0 += 64) {
                const int c = c0 + lane;
                const bool live = c < ncell;
                const int j = beg + c, u = c + 1, e = u + s;
                int he = 0, ee = 0, hd = 0, r = 4;
                if (live) {
                    if (i > 0) { he = hb[e]; ee = eb[e]; }
                    hd = hb[e - 1];
                    r = refc[j];
                }
                int t1 = he - gO, t2 = ee - gE;
                const int ev = max(t1, t2);
                const int de = t1 > t2 ? 3 : 2;
                const int e1 = max(ev, 0);
                const int dg = hd + ((r == 4 || q == 4) ? 0 : r == q ? a.match : -a.mismatch);
                const int ht = max(e1, dg);
                const int x = wave_incl_max(live ? ht - gO + (j + 1) * gE : LNEG, lane);
                int ex = __shfl_up(x, 1u, 64);
                if (lane == 0) ex = LNEG;
                const int g = max(carry, ex);
                int gp = __shfl_up(g, 1u, 64);
                if (lane == 0) gp = prev_g;
                const int df = g > gp ? 5 : 4;
                const int f = g - j * gE;
                const int f1 = max(f, 0);
                t1 = max(e1, f1);
                const int h = max(t1, dg);
                const int dh = t1 <= dg ? 1 : (e1 > f1 ? de : df);
                if (live) {
                    eb[u] = (int16_t)ev;
                    hc[u] = (int16_t)h;
                    prow[c] = dir_pack(de, df, dh);
                    lane_best = max(lane_best, h);
                }
                carry = max(carry, __shfl(x, 63, 64));
                prev_g = __shfl(g, 63, 64);
            }
            __syncthreads();
            for (int c = lane; c < ncell; c += 64) hb[c + 1] = hc[c + 1];
        }
        best = max(best, __shfl(wave_incl_max(lane_best, lane), 63, 64));
        if (best >= score) break;
        if (bw >= cover) return TREDGPU_CIGAR_NO_PATH;
        bw = min(bw * 2, cover);              // every band that covers the rectangle computes the same cells
    }
    __syncthreads();                          // the plane is this wavefront's own: its stores are visible to lane 0

    int status = TREDGPU_CIGAR_OK;
    if (lane == 0)
        status = traceback(a, item, it, bw, [&](int i, int j) { return (int)plane[(size_t)i * stride + (j - max(0, i - bw))]; });
    return __shfl(status, 0, 64);
}

__global__ __launch_bounds__(64) void cigar_long_kernel(LongCigarArgs a) {
    __shared__ int16_t rows[3 * ROW];
    __shared__ uint8_t refc[4096];
    const int lane = threadIdx.x;
    uint8_t* plane = a.plane + (size_t)blockIdx.x * a.slot_bytes;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        zero_ops(a, item, lane, 64);
        __syncthreads();
        const int status = decode_item(a, item, TREDGPU_MAX_LONG_READ_LEN, TREDGPU_MAX_LONG_TEMPLATE_LEN, [&](const Item& it) {
            return long_cigar_item(a, item, it, plane, rows, rows + ROW, rows + 2 * ROW, refc);
        });
        __syncthreads();
        if (status != TREDGPU_CIGAR_OK) zero_ops(a, item, lane, 64);
        if (lane == 0) store_status(a, item, status);
    }
}

// ---- host side (side_unit.h) --------------------------------------------------------------------------------------------
struct State : StateBase { Dev plane; };   // sized exactly: plan.total() is what the slots of a launch address
Registry<State> g_states;

}  // namespace

extern "C" {

int tredlong_sw_cigar(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                      const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                      const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                      const int16_t* fields, const tredgpu_sw_params* p, int32_t cap, uint32_t* out_ops,
                      int32_t* out_n_ops, int32_t* out_status) {
    std::string& err = g_long_error;
    err.clear();
    const Table t{n_ladders, prefix, repeat, suffix, max_units};
    int rc = call_refusal(err, ctx, true, t, n_items, cap, p,
                          {packed, read_off, read_len, item_ladder, item_template, fields, out_ops, out_n_ops, out_status});
    if (rc || n_items == 0) return rc;
    const size_t n = (size_t)n_items;
    if ((rc = reads_refusal(err, read_off, read_len, n, TREDGPU_MAX_LONG_READ_LEN))) return rc;
    hipStream_t st;
    if ((rc = select_device(err, ctx, st))) return rc;
    State* s = g_states.state_of(ctx);
    if ((rc = set_ladders(err, *s, st, t, TREDGPU_MAX_LONG_TEMPLATE_LEN))) return rc;

    const cigar_long_plan::Plan plan = cigar_long_plan::plan(fields, n_items);
    LongCigarArgs a{};
    fill_args(a, *s, packed, read_off, read_len, n_items, item_ladder, item_template, fields, *p, cap, out_ops, out_n_ops, out_status);
    const std::vector<Array> arrays = host_arrays(a);
    if ((rc = stage(err, *s, st, arrays))) return rc;
    if ((rc = ensure(err, s->plane, plan.total(), st, false))) return rc;
    a.plane = (uint8_t*)s->plane.p;
    a.slot_bytes = plan.slot_bytes;
    SIDE_UNIT_CHK(err, hipMemsetAsync(a.out_n_ops, 0, n * sizeof(int32_t), st));
    if ((rc = timed_begin(err, *s, st))) return rc;
    hipLaunchKernelGGL(cigar_long_kernel, dim3(plan.slots), dim3(64), 0, st, a);
    if ((rc = timed_end(err, *s, st))) return rc;
    return read_back(err, *s, st, arrays);
}

int tredlong_cigar_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) { return timing(g_long_error, g_states, ctx, launches, total_ms, false); }

int tredlong_cigar_reset_timing(tredgpu_ctx* ctx) { return timing(g_long_error, g_states, ctx, nullptr, nullptr, true); }

void tredlong_release(tredgpu_ctx* ctx) {
    release(g_states, ctx, {&State::plane});
    tredgpu::long_classify_release(ctx);
}

}  // extern "C"
