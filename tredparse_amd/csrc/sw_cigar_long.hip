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
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

#include <hip/hip_runtime.h>
#include "cigar_long_plan.h"
#include "ladder_host.h"
#include "../../include/tredcigar.h"
#include "../../include/tredlong.h"

namespace tredgpu {
extern thread_local std::string g_long_error;   // sw_long.hip: the text of tredlong_last_error()
}

namespace {
using namespace ladder_host;
using tredgpu::g_long_error;

static_assert(cigar_long_plan::MAX_READ == TREDGPU_MAX_LONG_READ_LEN && cigar_long_plan::MAX_TEMPLATE == TREDGPU_MAX_LONG_TEMPLATE_LEN,
              "cigar_long_plan.h restates the limits of tredlong.h");

struct LongCigarLadder {
    int32_t alen[2], blen[2];
    int32_t trunk_off[2], branch_off[2];   // byte offsets into the letter pool (one code 0..4 per byte)
    int32_t period, max_units;
};

struct LongCigarArgs {
    const uint32_t* packed;
    const int64_t* read_off;
    const int32_t* read_len;
    const int32_t* item_ladder;
    const int32_t* item_template;
    const int16_t* fields;
    const LongCigarLadder* ladders;
    const uint8_t* letters;
    int32_t n_ladders;
    int64_t n_items;
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t cap;
    uint32_t* out_ops;
    int32_t* out_n_ops;
    int32_t* out_status;
    uint8_t* plane;          // [slot][slot_bytes]
    size_t slot_bytes;
};

constexpr int ROW = 4100;                 // entries per row array: e <= refLen + 1, edge <= refLen
constexpr int LNEG = -(1 << 29);

__device__ __forceinline__ int wave_incl_max(int x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, (unsigned)d, 64);
        if (lane >= d) x = max(x, y);
    }
    return x;
}

// one item on one wavefront; every lane returns the status
__device__ int long_cigar_item(const LongCigarArgs& a, int64_t item, uint8_t* plane, int16_t* hb, int16_t* eb, int16_t* hc,
                               uint8_t* refc) {
    const int lane = threadIdx.x;
    uint32_t* ops = a.out_ops + (size_t)item * a.cap;
    const int lad = a.item_ladder[item], tpl = a.item_template[item];
    const int16_t* fl = a.fields + (size_t)item * 5;
    const int score = fl[0], ref_begin = fl[1], ref_end = fl[2], read_begin = fl[3], read_end = fl[4];
    const int L = a.read_len[item];
    if (lad < 0 || lad >= a.n_ladders) return TREDGPU_CIGAR_BAD_ITEM;
    const LongCigarLadder d = a.ladders[lad];
    if (tpl < 0 || tpl >= (d.max_units > 0 ? 2 * d.max_units : 1)) return TREDGPU_CIGAR_BAD_ITEM;
    const int strand = d.max_units > 0 ? (tpl & 1) : 0;
    const int trunk = d.alen[strand] + (d.max_units > 0 ? d.period * (tpl / 2 + 1) : 0);
    const int tlen = trunk + d.blen[strand];
    if (L > TREDGPU_MAX_LONG_READ_LEN || tlen > TREDGPU_MAX_LONG_TEMPLATE_LEN) return TREDGPU_CIGAR_TOO_LONG;
    if (ref_begin < 0 || ref_end < ref_begin || ref_end >= tlen || read_begin < 0 || read_end < read_begin || read_end >= L)
        return TREDGPU_CIGAR_BAD_ITEM;
    const int refLen = ref_end - ref_begin + 1, readLen = read_end - read_begin + 1;
    if ((size_t)refLen * readLen > a.slot_bytes) return TREDGPU_CIGAR_TOO_LONG;   // (the host sized the slot from these fields)
    const uint8_t* tr = a.letters + d.trunk_off[strand];
    const uint8_t* br = a.letters + d.branch_off[strand];
    const uint32_t* rec = a.packed + a.read_off[item];
    const int nb = (L + 15) >> 4;
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
            const int q = ((rec[nb + (ri >> 5)] >> (ri & 31)) & 1u) ? 4 : (int)((rec[ri >> 4] >> ((ri & 15) * 2)) & 3u);
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
                    prow[c] = (uint8_t)((de - 2) | ((df - 4) << 1) | (dh << 2));
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
    if (lane == 0) {                                                                    // ssw.c:636-715
        int i = readLen - 1, j = refLen - 1, e = 0, l = 0, which = 2, op = 0, prev = 0;
        auto emit = [&](uint32_t v) { if (l < a.cap) ops[l] = v; ++l; };
        while (i > 0) {
            const int beg = max(0, i - bw);
            if (j < beg || j > i + bw) { status = TREDGPU_CIGAR_OFF_EDGE; break; }      // a cell this pass never wrote
            const int c = plane[(size_t)i * stride + (j - beg)];
            const int step = which == 0 ? 2 + (c & 1) : which == 1 ? 4 + ((c >> 1) & 1) : (c >> 2);
            switch (step) {
                case 1: --i; --j; which = 2; op = 0; break;
                case 2: --i; which = 0; op = 1; break;
                case 3: --i; which = 2; op = 1; break;
                case 4: --j; which = 1; op = 2; break;
                default: --j; which = 2; op = 2; break;
            }
            if (op == prev) ++e;
            else { emit((uint32_t)e << 4 | prev); prev = op; e = 1; }
        }
        if (status == TREDGPU_CIGAR_OK) {
            if (op == 0) emit((uint32_t)(e + 1) << 4);
            else { emit((uint32_t)e << 4 | op); emit(1u << 4); }
            a.out_n_ops[item] = l;
            if (l > a.cap) status = TREDGPU_CIGAR_OVERFLOW;
            else
                for (int p = 0, t = l - 1; p < t; ++p, --t) { const uint32_t v = ops[p]; ops[p] = ops[t]; ops[t] = v; }   // :717-726
        }
    }
    return __shfl(status, 0, 64);
}

__global__ __launch_bounds__(64) void cigar_long_kernel(LongCigarArgs a) {
    __shared__ int16_t rows[3 * ROW];
    __shared__ uint8_t refc[4096];
    const int lane = threadIdx.x;
    uint8_t* plane = a.plane + (size_t)blockIdx.x * a.slot_bytes;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        uint32_t* ops = a.out_ops + (size_t)item * a.cap;
        for (int k = lane; k < a.cap; k += 64) ops[k] = 0;
        __syncthreads();
        const int status = long_cigar_item(a, item, plane, rows, rows + ROW, rows + 2 * ROW, refc);
        __syncthreads();
        if (status != TREDGPU_CIGAR_OK)                                  // (sw_cigar.hip's cigar_finish)
            for (int k = lane; k < a.cap; k += 64) ops[k] = 0;
        if (lane == 0) {
            a.out_status[item] = status;
            if (status != TREDGPU_CIGAR_OK && status != TREDGPU_CIGAR_OVERFLOW) a.out_n_ops[item] = 0;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
#define LCCHK(expr)                                                                                      \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(g_long_error, -10, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

struct Dev {
    void* p = nullptr;
    size_t cap = 0;
};

// what the calls on one context hold (grow-only, reused across calls)
struct State {
    std::string ladder_key;
    int n_ladders = 0;
    Dev ladders, letters, plane, st[9];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t used = 0;
    int64_t launches = 0;
    double total_ms = 0;
};

std::mutex g_mu;
std::map<tredgpu_ctx*, State*> g_states;

State* state_of(tredgpu_ctx* ctx) {
    std::lock_guard<std::mutex> lock(g_mu);
    State*& s = g_states[ctx];
    if (!s) s = new State();
    return s;
}

// slack: staging buffers grow by a quarter more than asked; the plane is sized exactly (its cap is a promise)
int ensure(Dev& b, size_t bytes, hipStream_t st, bool slack = true) {
    bytes = std::max<size_t>(bytes, 16);
    if (b.cap >= bytes) return 0;
    if (b.p) {
        LCCHK(hipStreamSynchronize(st));        // the buffer may still be in use by enqueued work
        LCCHK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = slack ? bytes + bytes / 4 : bytes;
    LCCHK(hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

// the ladder table of the call, in sw_cigar.hip's layout; uploaded only when it differs from the previous call's
int set_ladders(State* s, hipStream_t st, int32_t n, const char* const* prefix, const char* const* repeat,
                const char* const* suffix, const int32_t* max_units) {
    std::string key;
    for (int i = 0; i < n; ++i) {
        if (!prefix[i] || !repeat[i] || !suffix[i]) return fail(g_long_error, -2, "ladder %d: NULL sequence", i);
        key += prefix[i]; key += '|'; key += repeat[i]; key += '|'; key += suffix[i]; key += '|';
        key += std::to_string(max_units[i]); key += ';';
    }
    if (s->n_ladders == n && key == s->ladder_key) return 0;
    std::vector<LongCigarLadder> lad((size_t)n);
    std::vector<uint8_t> pool;
    auto append = [&pool](const Codes& v) {
        const int off = (int)pool.size();
        pool.insert(pool.end(), v.begin(), v.end());
        return off;
    };
    Strands S;
    for (int i = 0; i < n; ++i) {
        LongCigarLadder& d = lad[i];
        memset(&d, 0, sizeof d);
        if (const char* why = build_strands(prefix[i], repeat[i], suffix[i], max_units[i], S))
            return fail(g_long_error, -2, "ladder %d: %s", i, why);
        const size_t T = (size_t)S.alen[0] + S.blen[0] + (size_t)S.period * S.max_units;
        if (T > TREDGPU_MAX_LONG_TEMPLATE_LEN)
            return fail(g_long_error, -2, "ladder %d: longest template %zu exceeds TREDGPU_MAX_LONG_TEMPLATE_LEN=%d", i, T,
                        TREDGPU_MAX_LONG_TEMPLATE_LEN);
        d.period = S.period;
        d.max_units = S.max_units;
        for (int k = 0; k < S.n_strands; ++k) {
            d.alen[k] = S.alen[k];
            d.blen[k] = S.blen[k];
            d.trunk_off[k] = append(S.trunk[k]);
            d.branch_off[k] = append(S.branch[k]);
        }
    }
    pool.resize(pool.size() + 16, 4);
    int rc;
    if ((rc = ensure(s->ladders, lad.size() * sizeof(LongCigarLadder), st))) return rc;
    if ((rc = ensure(s->letters, pool.size(), st))) return rc;
    LCCHK(hipStreamSynchronize(st));
    if (n) LCCHK(hipMemcpy(s->ladders.p, lad.data(), lad.size() * sizeof(LongCigarLadder), hipMemcpyHostToDevice));
    LCCHK(hipMemcpy(s->letters.p, pool.data(), pool.size(), hipMemcpyHostToDevice));
    s->ladder_key.swap(key);
    s->n_ladders = n;
    return 0;
}

}  // namespace

extern "C" {

int tredlong_sw_cigar(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                      const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                      const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                      const int16_t* fields, const tredgpu_sw_params* p, int32_t cap, uint32_t* out_ops,
                      int32_t* out_n_ops, int32_t* out_status) {
    g_long_error.clear();
    if (!ctx) return fail(g_long_error, -2, "ctx is NULL");
    if (n_items < 0 || n_items > 0x7fffffff || n_ladders <= 0 || cap <= 0) return fail(g_long_error, -2, "n_items, n_ladders and cap must be positive");
    if (!prefix || !repeat || !suffix || !max_units) return fail(g_long_error, -2, "NULL ladder argument");
    if (!p) return fail(g_long_error, -2, "params is NULL");
    if (const char* why = scoring_refusal(*p, false)) return fail(g_long_error, -2, "%s", why);
    if (n_items == 0) return 0;
    if (!packed || !read_off || !read_len || !item_ladder || !item_template || !fields || !out_ops || !out_n_ops || !out_status)
        return fail(g_long_error, -2, "NULL array argument");
    const size_t n = (size_t)n_items;
    if (read_off[0] < 0 || read_off[n] < read_off[0]) return fail(g_long_error, -2, "read_off must be monotone");
    for (size_t k = 0; k < n; ++k) {            // the kernel reads the words of every read it accepts: they are among those copied
        const int L = read_len[k];
        if (L < 0 || L > TREDGPU_MAX_LONG_READ_LEN) continue;
        if (read_off[k] < 0 || read_off[k] + ((L + 15) >> 4) + ((L + 31) >> 5) > read_off[n])
            return fail(g_long_error, -2, "item %zu: its read does not lie inside packed[0 .. read_off[n_items])", k);
    }
    hipStream_t st = (hipStream_t)tredgpu_get_stream(ctx);
    int dev = 0;
    LCCHK(hipStreamGetDevice(st, &dev));
    LCCHK(hipSetDevice(dev));
    State* s = state_of(ctx);
    int rc;
    if ((rc = set_ladders(s, st, n_ladders, prefix, repeat, suffix, max_units))) return rc;

    const cigar_long_plan::Plan plan = cigar_long_plan::plan(fields, n_items);
    LongCigarArgs a;
    memset(&a, 0, sizeof a);
    const size_t sizes[9] = {(size_t)read_off[n] * 4, (n + 1) * 8, n * 4, n * 4, n * 4, n * 10,
                             n * cap * sizeof(uint32_t), n * 4, n * 4};
    const void* src[6] = {packed, read_off, read_len, item_ladder, item_template, fields};
    for (int k = 0; k < 9; ++k)
        if ((rc = ensure(s->st[k], sizes[k], st))) return rc;
    if ((rc = ensure(s->plane, plan.total(), st, false))) return rc;
    for (int k = 0; k < 6; ++k)
        if (sizes[k]) LCCHK(hipMemcpyAsync(s->st[k].p, src[k], sizes[k], hipMemcpyHostToDevice, st));
    a.packed = (const uint32_t*)s->st[0].p;
    a.read_off = (const int64_t*)s->st[1].p;
    a.read_len = (const int32_t*)s->st[2].p;
    a.item_ladder = (const int32_t*)s->st[3].p;
    a.item_template = (const int32_t*)s->st[4].p;
    a.fields = (const int16_t*)s->st[5].p;
    a.out_ops = (uint32_t*)s->st[6].p;
    a.out_n_ops = (int32_t*)s->st[7].p;
    a.out_status = (int32_t*)s->st[8].p;
    a.ladders = (const LongCigarLadder*)s->ladders.p;
    a.letters = (const uint8_t*)s->letters.p;
    a.n_ladders = n_ladders;
    a.n_items = n_items;
    a.match = p->match; a.mismatch = p->mismatch; a.gap_open = p->gap_open; a.gap_extend = p->gap_extend;
    a.cap = cap;
    a.plane = (uint8_t*)s->plane.p;
    a.slot_bytes = plan.slot_bytes;
    LCCHK(hipMemsetAsync(a.out_n_ops, 0, n * sizeof(int32_t), st));
    if (s->used == s->events.size()) {
        if (s->used >= 256) {                   // bounded pool: fold what is already finished
            LCCHK(hipStreamSynchronize(st));
            tredlong_cigar_timing(ctx, nullptr, nullptr);
        } else {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            LCCHK(hipEventCreate(&e0));
            LCCHK(hipEventCreate(&e1));
            s->events.emplace_back(e0, e1);
        }
    }
    LCCHK(hipEventRecord(s->events[s->used].first, st));
    hipLaunchKernelGGL(cigar_long_kernel, dim3(plan.slots), dim3(64), 0, st, a);
    LCCHK(hipGetLastError());
    LCCHK(hipEventRecord(s->events[s->used].second, st));
    s->used += 1;
    LCCHK(hipMemcpyAsync(out_ops, a.out_ops, n * cap * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    LCCHK(hipMemcpyAsync(out_n_ops, a.out_n_ops, n * 4, hipMemcpyDeviceToHost, st));
    LCCHK(hipMemcpyAsync(out_status, a.out_status, n * 4, hipMemcpyDeviceToHost, st));
    LCCHK(hipStreamSynchronize(st));
    return 0;
}

int tredlong_cigar_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) {
    if (!ctx) return fail(g_long_error, -2, "ctx is NULL");
    State* s = state_of(ctx);
    LCCHK(hipStreamSynchronize((hipStream_t)tredgpu_get_stream(ctx)));
    for (size_t i = 0; i < s->used; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s->events[i].first, s->events[i].second) == hipSuccess) {
            s->total_ms += ms;
            s->launches += 1;
        }
    }
    s->used = 0;
    if (launches) *launches = s->launches;
    if (total_ms) *total_ms = s->total_ms;
    return 0;
}

int tredlong_cigar_reset_timing(tredgpu_ctx* ctx) {
    int rc = tredlong_cigar_timing(ctx, nullptr, nullptr);
    if (rc) return rc;
    State* s = state_of(ctx);
    s->launches = 0;
    s->total_ms = 0;
    return 0;
}

void tredlong_release(tredgpu_ctx* ctx) {
    State* s = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        auto it = g_states.find(ctx);
        if (it == g_states.end()) return;
        s = it->second;
        g_states.erase(it);
    }
    (void)hipStreamSynchronize((hipStream_t)tredgpu_get_stream(ctx));
    for (Dev* b : {&s->ladders, &s->letters, &s->plane})
        if (b->p) (void)hipFree(b->p);
    for (Dev& b : s->st)
        if (b.p) (void)hipFree(b.p);
    for (auto& ev : s->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    delete s;
}

}  // extern "C"
