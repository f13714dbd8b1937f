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
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

#include <hip/hip_runtime.h>
#include "ladder_host.h"
#include "../../include/tredcigar.h"

namespace {
using namespace ladder_host;

struct CigarLadder {
    int32_t alen[2], blen[2];
    int32_t trunk_off[2], branch_off[2];   // byte offsets into the letter pool (one code 0..4 per byte)
    int32_t period, max_units;
};

struct CigarArgs {
    const uint32_t* packed;
    const int64_t* read_off;
    const int32_t* read_len;
    const int32_t* item_ladder;
    const int32_t* item_template;
    const int16_t* fields;
    const CigarLadder* ladders;
    const uint8_t* letters;
    int32_t n_ladders;
    int64_t n_items;
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t cap;
    uint32_t* out_ops;
    int32_t* out_n_ops;
    int32_t* out_status;
    uint8_t* plane;        // narrow: [wavefront][cell][lane]; wide: [lane][cell]
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

// one item, start to end; NEEDS_WIDE when a pass does not fit the store (nothing has been written to the outputs then)
__device__ int cigar_item(const CigarArgs& a, int64_t item, const Store& st) {
    uint32_t* ops = a.out_ops + (size_t)item * a.cap;
    const int lad = a.item_ladder[item], tpl = a.item_template[item];
    const int16_t* fl = a.fields + (size_t)item * 5;
    const int score = fl[0], ref_begin = fl[1], ref_end = fl[2], read_begin = fl[3], read_end = fl[4];
    const int L = a.read_len[item];
    if (lad < 0 || lad >= a.n_ladders) return TREDGPU_CIGAR_BAD_ITEM;
    const CigarLadder d = a.ladders[lad];
    if (tpl < 0 || tpl >= (d.max_units > 0 ? 2 * d.max_units : 1)) return TREDGPU_CIGAR_BAD_ITEM;
    const int strand = d.max_units > 0 ? (tpl & 1) : 0;
    const int trunk = d.alen[strand] + (d.max_units > 0 ? d.period * (tpl / 2 + 1) : 0);
    const int tlen = trunk + d.blen[strand];
    if (L > TREDGPU_MAX_READ_LEN || tlen > TREDGPU_MAX_TEMPLATE_LEN) return TREDGPU_CIGAR_TOO_LONG;
    if (ref_begin < 0 || ref_end < ref_begin || ref_end >= tlen || read_begin < 0 || read_end < read_begin || read_end >= L)
        return TREDGPU_CIGAR_BAD_ITEM;
    const uint8_t* tr = a.letters + d.trunk_off[strand];
    const uint8_t* br = a.letters + d.branch_off[strand];
    const uint32_t* rec = a.packed + a.read_off[item];
    const int nb = (L + 15) >> 4;
    const int refLen = ref_end - ref_begin + 1, readLen = read_end - read_begin + 1;
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
            const int q = ((rec[nb + (ri >> 5)] >> (ri & 31)) & 1u) ? 4 : (int)((rec[ri >> 4] >> ((ri & 15) * 2)) & 3u);
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
                st.cell(width_d * i + (j - x0)) = (uint8_t)((de - 2) | ((df - 4) << 1) | (dh << 2));
            }
            for (int j = 1; j <= u; ++j) st.hb(j) = st.hc(j);
        }
        if (best >= score) break;
        if (bw >= cover) return TREDGPU_CIGAR_NO_PATH;
        bw = min(bw * 2, cover);              // every band that covers the rectangle computes the same cells
    }

    int i = readLen - 1, j = refLen - 1, e = 0, l = 0, which = 2, op = 0, prev = 0;   // ssw.c:636-715
    auto emit = [&](uint32_t v) { if (l < a.cap) ops[l] = v; ++l; };
    while (i > 0) {
        if (j < max(0, i - bw) || j > i + bw) return TREDGPU_CIGAR_OFF_EDGE;          // a cell this pass never wrote
        const int c = st.cell(width_d * i + band_x(bw, i, j));
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
    if (op == 0) emit((uint32_t)(e + 1) << 4);
    else { emit((uint32_t)e << 4 | op); emit(1u << 4); }
    a.out_n_ops[item] = l;
    if (l > a.cap) return TREDGPU_CIGAR_OVERFLOW;
    for (int s = 0, t = l - 1; s < t; ++s, --t) { const uint32_t v = ops[s]; ops[s] = ops[t]; ops[t] = v; }   // :717-726
    return TREDGPU_CIGAR_OK;
}

__device__ void cigar_finish(const CigarArgs& a, int64_t item, int status) {
    a.out_status[item] = status;
    if (status == TREDGPU_CIGAR_OK) return;
    if (status != TREDGPU_CIGAR_OVERFLOW) a.out_n_ops[item] = 0;
    for (int k = 0; k < a.cap; ++k) a.out_ops[(size_t)item * a.cap + k] = 0;
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
        for (int k = 0; k < a.cap; ++k) a.out_ops[(size_t)item * a.cap + k] = 0;
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

// ---- host side ------------------------------------------------------------------------------------------------------
thread_local std::string g_cigar_error;

#define CIGCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(g_cigar_error, -10, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

struct Dev {
    void* p = nullptr;
    size_t cap = 0;
};

// what the calls on one context hold (grow-only, reused across calls)
struct State {
    std::string ladder_key;
    int n_ladders = 0;
    Dev ladders, letters, narrow_plane, wide_plane, wide_rows, wide_list, st[9];
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

int ensure(Dev& b, size_t bytes, hipStream_t st) {
    bytes = std::max<size_t>(bytes, 16);
    if (b.cap >= bytes) return 0;
    if (b.p) {
        CIGCHK(hipStreamSynchronize(st));       // the buffer may still be in use by enqueued work
        CIGCHK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    CIGCHK(hipMalloc(&b.p, bytes + bytes / 4));
    b.cap = bytes + bytes / 4;
    return 0;
}

// the ladder table of the call (layout of tredgpu_set_ladders: trunk = prefix + repeat * max_units / rc(suffix) +
// rc(repeat) * max_units, branch = suffix / rc(prefix)); uploaded only when it differs from the previous call's
int set_ladders(State* s, hipStream_t st, int32_t n, const char* const* prefix, const char* const* repeat,
                const char* const* suffix, const int32_t* max_units) {
    std::string key;
    for (int i = 0; i < n; ++i) {
        if (!prefix[i] || !repeat[i] || !suffix[i]) return fail(g_cigar_error, -2, "ladder %d: NULL sequence", i);
        key += prefix[i]; key += '|'; key += repeat[i]; key += '|'; key += suffix[i]; key += '|';
        key += std::to_string(max_units[i]); key += ';';
    }
    if (s->n_ladders == n && key == s->ladder_key) return 0;
    std::vector<CigarLadder> lad((size_t)n);
    std::vector<uint8_t> pool;
    auto append = [&pool](const Codes& v) {
        const int off = (int)pool.size();
        pool.insert(pool.end(), v.begin(), v.end());
        return off;
    };
    Strands S;
    for (int i = 0; i < n; ++i) {
        CigarLadder& d = lad[i];
        memset(&d, 0, sizeof d);
        if (const char* why = build_strands(prefix[i], repeat[i], suffix[i], max_units[i], S))
            return fail(g_cigar_error, -2, "ladder %d: %s", i, why);
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
    if ((rc = ensure(s->ladders, lad.size() * sizeof(CigarLadder), st))) return rc;
    if ((rc = ensure(s->letters, pool.size(), st))) return rc;
    CIGCHK(hipStreamSynchronize(st));
    if (n) CIGCHK(hipMemcpy(s->ladders.p, lad.data(), lad.size() * sizeof(CigarLadder), hipMemcpyHostToDevice));
    CIGCHK(hipMemcpy(s->letters.p, pool.data(), pool.size(), hipMemcpyHostToDevice));
    s->ladder_key.swap(key);
    s->n_ladders = n;
    return 0;
}

}  // namespace

extern "C" {

const char* tredcigar_last_error(void) { return g_cigar_error.c_str(); }

int tredcigar_sw_cigar(tredgpu_ctx* ctx, int mem, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                       const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                       const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                       const int16_t* fields, const tredgpu_sw_params* p, int32_t cap, uint32_t* out_ops,
                       int32_t* out_n_ops, int32_t* out_status) {
    g_cigar_error.clear();
    if (!ctx) return fail(g_cigar_error, -2, "ctx is NULL");
    if (mem != TREDGPU_MEM_HOST && mem != TREDGPU_MEM_DEVICE) return fail(g_cigar_error, -2, "mem must be TREDGPU_MEM_HOST or TREDGPU_MEM_DEVICE");
    if (n_items < 0 || n_items > 0x7fffffff || n_ladders <= 0 || cap <= 0) return fail(g_cigar_error, -2, "n_items, n_ladders and cap must be positive");
    if (!prefix || !repeat || !suffix || !max_units) return fail(g_cigar_error, -2, "NULL ladder argument");
    if (!p) return fail(g_cigar_error, -2, "params is NULL");
    if (const char* why = scoring_refusal(*p, false)) return fail(g_cigar_error, -2, "%s", why);
    if (n_items == 0) return 0;
    if (!packed || !read_off || !read_len || !item_ladder || !item_template || !fields || !out_ops || !out_n_ops || !out_status)
        return fail(g_cigar_error, -2, "NULL array argument");
    hipStream_t st = (hipStream_t)tredgpu_get_stream(ctx);
    int dev = 0;
    CIGCHK(hipStreamGetDevice(st, &dev));
    CIGCHK(hipSetDevice(dev));
    State* s = state_of(ctx);
    int rc;
    if ((rc = set_ladders(s, st, n_ladders, prefix, repeat, suffix, max_units))) return rc;

    CigarArgs a;
    memset(&a, 0, sizeof a);
    const size_t n = (size_t)n_items;
    if (mem == TREDGPU_MEM_HOST) {
        if (read_off[0] < 0 || read_off[n] < read_off[0]) return fail(g_cigar_error, -2, "read_off must be monotone");
        const size_t sizes[9] = {(size_t)read_off[n] * 4, (n + 1) * 8, n * 4, n * 4, n * 4, n * 10,
                                 n * cap * sizeof(uint32_t), n * 4, n * 4};
        const void* src[6] = {packed, read_off, read_len, item_ladder, item_template, fields};
        for (int k = 0; k < 9; ++k)
            if ((rc = ensure(s->st[k], sizes[k], st))) return rc;
        for (int k = 0; k < 6; ++k)
            if (sizes[k]) CIGCHK(hipMemcpyAsync(s->st[k].p, src[k], sizes[k], hipMemcpyHostToDevice, st));
        a.packed = (const uint32_t*)s->st[0].p;
        a.read_off = (const int64_t*)s->st[1].p;
        a.read_len = (const int32_t*)s->st[2].p;
        a.item_ladder = (const int32_t*)s->st[3].p;
        a.item_template = (const int32_t*)s->st[4].p;
        a.fields = (const int16_t*)s->st[5].p;
        a.out_ops = (uint32_t*)s->st[6].p;
        a.out_n_ops = (int32_t*)s->st[7].p;
        a.out_status = (int32_t*)s->st[8].p;
    } else {
        a.packed = packed; a.read_off = read_off; a.read_len = read_len;
        a.item_ladder = item_ladder; a.item_template = item_template; a.fields = fields;
        a.out_ops = out_ops; a.out_n_ops = out_n_ops; a.out_status = out_status;
    }
    a.ladders = (const CigarLadder*)s->ladders.p;
    a.letters = (const uint8_t*)s->letters.p;
    a.n_ladders = n_ladders;
    a.n_items = n_items;
    a.match = p->match; a.mismatch = p->mismatch; a.gap_open = p->gap_open; a.gap_extend = p->gap_extend;
    a.cap = cap;
    const int blocks = (int)std::min<size_t>((n + 63) / 64, NARROW_MAX_LANES / 64);
    if ((rc = ensure(s->narrow_plane, (size_t)blocks * 64 * NARROW_PLANE, st))) return rc;
    if ((rc = ensure(s->wide_plane, (size_t)WIDE_LANES * WIDE_PLANE, st))) return rc;
    if ((rc = ensure(s->wide_rows, (size_t)WIDE_LANES * 3 * WIDE_ROW * sizeof(int16_t), st))) return rc;
    if ((rc = ensure(s->wide_list, (n + 1) * sizeof(int32_t), st))) return rc;
    a.wide_list = (int32_t*)s->wide_list.p;
    a.wide_rows = (int16_t*)s->wide_rows.p;
    CIGCHK(hipMemsetAsync(a.wide_list + n, 0, sizeof(int32_t), st));
    CIGCHK(hipMemsetAsync(a.out_n_ops, 0, n * sizeof(int32_t), st));
    if (s->used == s->events.size()) {
        if (s->used >= 256) {                   // bounded pool: fold what is already finished
            CIGCHK(hipStreamSynchronize(st));
            tredcigar_get_timing(ctx, nullptr, nullptr);
        } else {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            CIGCHK(hipEventCreate(&e0));
            CIGCHK(hipEventCreate(&e1));
            s->events.emplace_back(e0, e1);
        }
    }
    CIGCHK(hipEventRecord(s->events[s->used].first, st));
    a.plane = (uint8_t*)s->narrow_plane.p;
    hipLaunchKernelGGL(cigar_narrow_kernel, dim3(blocks), dim3(64), 0, st, a);
    CIGCHK(hipGetLastError());
    a.plane = (uint8_t*)s->wide_plane.p;
    hipLaunchKernelGGL(cigar_wide_kernel, dim3(1), dim3(WIDE_LANES), 0, st, a);
    CIGCHK(hipGetLastError());
    CIGCHK(hipEventRecord(s->events[s->used].second, st));
    s->used += 1;
    if (mem == TREDGPU_MEM_HOST) {
        CIGCHK(hipMemcpyAsync(out_ops, a.out_ops, n * cap * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CIGCHK(hipMemcpyAsync(out_n_ops, a.out_n_ops, n * 4, hipMemcpyDeviceToHost, st));
        CIGCHK(hipMemcpyAsync(out_status, a.out_status, n * 4, hipMemcpyDeviceToHost, st));
        CIGCHK(hipStreamSynchronize(st));
    }
    return 0;
}

int tredcigar_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) {
    if (!ctx) return fail(g_cigar_error, -2, "ctx is NULL");
    State* s = state_of(ctx);
    CIGCHK(hipStreamSynchronize((hipStream_t)tredgpu_get_stream(ctx)));
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

int tredcigar_reset_timing(tredgpu_ctx* ctx) {
    int rc = tredcigar_get_timing(ctx, nullptr, nullptr);
    if (rc) return rc;
    State* s = state_of(ctx);
    s->launches = 0;
    s->total_ms = 0;
    return 0;
}

void tredcigar_release(tredgpu_ctx* ctx) {
    State* s = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        auto it = g_states.find(ctx);
        if (it == g_states.end()) return;
        s = it->second;
        g_states.erase(it);
    }
    (void)hipStreamSynchronize((hipStream_t)tredgpu_get_stream(ctx));
    for (Dev* b : {&s->ladders, &s->letters, &s->narrow_plane, &s->wide_plane, &s->wide_rows, &s->wide_list})
        if (b->p) (void)hipFree(b->p);
    for (Dev& b : s->st)
        if (b.p) (void)hipFree(b.p);
    for (auto& ev : s->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    delete s;
}

}  // extern "C"
