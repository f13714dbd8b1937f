// sw_long.hip -- exact template-ladder Smith-Waterman for long reads and long ladders (gfx950, MI355X).
//
// The opt-in long-read path (include/tredlong.h; Context.set_long_reads in tredparse_amd/_lib.py routes to it): reads
// of 481..TREDGPU_MAX_LONG_READ_LEN bp and ladders whose longest template has 512..TREDGPU_MAX_LONG_TEMPLATE_LEN
// columns, which sw_cont_kernel's packed 32-bit values cannot hold.
// It computes what sw_cont_kernel computes -- per template the s_align fields of ssw_align (forward pass + reverse
// pass, the reference's src/ssw.c:780-871) and per read the tag / h / score of _parseReadSW
// (tredparse/bam_parser.py:123-182) -- with the same formulation and tie rules, in wider values:
//  * every DP value is an int64: high word = score + (row + col) * gap_extend (the anti-diagonal-scaled score of
//    sw_ladder.hip), low word = start column << 16 | start row.  Integer max picks (score, largest start column,
//    largest start row): the reverse pass's begin cell.  The floor Z(i, c) (score 0, start (c+1, i+1)) and the E / F
//    recurrences fed from H without the vertical-gap term are those of sweep_column.
//  * end cell: the first column that reaches the template's max, then the smallest row -- kept per lane as the
//    key (score, -column, -row) and reduced over the wave at each template end.
//  * one wavefront per read and strand pass: lane l holds rows l*R .. l*R+R-1 (R = 8, 16, 32 for reads up to 512,
//    1024, 2048 bp); the vertical-gap term crosses lanes as an exclusive max scan over the 64 lanes.
//  * shared trunk: templates prefix + repeat*u + suffix share the trunk prefix + repeat*max_units, swept once per
//    strand.  At template u's end column the trunk state is parked in LDS, the |suffix| columns of that template are
//    swept from it, and the trunk resumes: (|trunk| + max_units * |suffix|) columns per strand instead of the
//    O(max_units^2) of separate alignments.
// No pruning: every template of both strands is aligned (the path serves rare reads; the per-template dump needs all).
#include <algorithm>
#include <cstring>

#include "ladder_host.h"
#include "tredgpu_internal.h"
#include "../../include/tredlong.h"

namespace tredgpu {
namespace {

struct LongLadder {
    LadderDesc d;   // tredgpu_set_ladders' layout (kmer fields unused)
};

constexpr int LNEG = -(1 << 30);

__device__ __forceinline__ long long mk(int hi, uint32_t lo) { return (long long)(((uint64_t)(uint32_t)hi << 32) | lo); }
__device__ __forceinline__ int hi_of(long long v) { return (int)((uint64_t)v >> 32); }
__device__ __forceinline__ uint32_t lo_of(long long v) { return (uint32_t)v; }
// add d to the score word (the start payload in the low word is untouched)
__device__ __forceinline__ long long add_hi(long long v, int d) { return mk(hi_of(v) + d, lo_of(v)); }
__device__ __forceinline__ long long max64(long long a, long long b) { return a > b ? a : b; }

__device__ __forceinline__ long long shfl_up64(long long v, int d) { return __shfl_up(v, (unsigned)d, 64); }
__device__ __forceinline__ long long shfl_xor64(long long v, int d) { return __shfl_xor(v, d, 64); }

// Ladder letters: 8 per 32-bit word (tredgpu_set_ladders); wave-uniform index.
__device__ __forceinline__ int ladder_letter(const uint32_t* seqw, int word_off, int idx) {
    const uint32_t w = seqw[word_off + (idx >> 3)];
    return (int)((w >> ((idx & 7) * 4)) & 7u);
}

template <int R>
struct LongRows {
    uint32_t code[R / 4];  // per row one byte: 5 * (read code 0..3, 4 = N, 5 = padding): the bit offset into the score table
    int row0;
};

// Per lane: the best cell seen so far as (key, start payload); key = score << 32 | (0xFFFF - col) << 16 | (0xFFFF - row)
struct LongBest {
    long long key;
    uint32_t start;
};

// One DP column (template column `col`, letter `let`) for this lane's R rows.
//   lut: 5-bit fields, field k = score of read code k against `let`, + 16
template <int R>
__device__ __forceinline__ void long_column(const LongRows<R>& J, long long (&H)[R], long long (&E)[R], LongBest& B,
                                            int col, uint32_t lut, int ge, int c0) {
    const int lane = __lane_id();
    // H of the row above this lane's first row, previous column; above row 0 lies Z(-1, col-1)
    long long diag = shfl_up64(H[R - 1], 1);
    if (lane == 0) diag = mk((col - 2) * ge, (uint32_t)col << 16);
    const int s_fix = 2 * ge - 16;
    const int zhi = (J.row0 + col) * ge;
    const uint32_t zlo = ((uint32_t)(col + 1) << 16) + (uint32_t)(J.row0 + 1);
    long long run = mk(LNEG, 0);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t off = (J.code[r >> 2] >> ((r & 3) * 8)) & 0xFFu;
        const int s = (int)((lut >> off) & 31u) + s_fix;
        const long long t1 = add_hi(diag, s);                 // extend (row-1, col-1), or start here after its floor
        const long long z = mk(zhi + r * ge, zlo + (uint32_t)r);   // Z(row, col)
        const long long v = max64(max64(t1, z), E[r]);
        diag = H[r];
        H[r] = v;                                             // without the vertical-gap term for now
        const long long q = add_hi(v, -c0);
        run = max64(run, q);
        E[r] = max64(E[r], q);                                // E~ for the next column (fed from H without F)
    }
    // exclusive max scan over the 64 lanes: F~ entering this lane from the rows above it
    long long x = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = shfl_up64(x, d);
        if (lane >= d) x = max64(x, y);
    }
    long long F = shfl_up64(x, 1);
    if (lane == 0) F = mk(LNEG, 0);
    int m = LNEG;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long ht = H[r];
        H[r] = max64(ht, F);
        F = max64(F, add_hi(ht, -c0));
        m = max(m, hi_of(H[r]) - r * ge);
    }
    // a new best cell of this lane: strictly more than its best (a later column never wins a tie).  Padding rows
    // (row >= L, scored -16 against every letter) take part: a padding cell scores less than some real cell of the same
    // or an earlier column (its value comes from a real cell above by a vertical gap, or from the last real row by a
    // -16 diagonal step, or from a padding cell of an earlier column), so it never wins a template's reduction.
    const int top = m - (J.row0 + col) * ge;
    if (top > hi_of(B.key)) {
        int row = 0;
        uint32_t st = 0;
#pragma unroll
        for (int r = R - 1; r >= 0; --r) {
            const bool hit = hi_of(H[r]) - r * ge == m;
            row = hit ? r : row;
            st = hit ? lo_of(H[r]) : st;
        }
        B.key = mk(top, ((uint32_t)(0xFFFF - col) << 16) | (uint32_t)(0xFFFF - (J.row0 + row)));
        B.start = st;
    }
}

__device__ __forceinline__ uint32_t score_lut(int let, const tredgpu_sw_params& p) {
    uint32_t lut = 0;
    for (int k = 0; k < 6; ++k) {
        int s;
        if (k == 5) s = -16;                            // padding row (see long_column)
        else if (k == 4 || let > 3) s = 0;              // N on either side scores 0 (ssw_wrap.py:162-167)
        else s = k == let ? p.match : -p.mismatch;
        lut |= (uint32_t)(s + 16) << (5 * k);
    }
    return lut;
}

template <int R>
__global__ __launch_bounds__(64) void sw_long_kernel(SwArgs a, const LongLadder* lads, const int2* list, const int32_t* count) {
    // the trunk state parked while a template's suffix is swept: H and E of every row
    __shared__ long long park[2 * R * 64];
    const int lane = __lane_id();
    const int n = *count;
    const int ge = a.p.gap_extend, c0 = a.p.gap_open - a.p.gap_extend, flank = a.p.flank;
    for (int it = blockIdx.x; it < n; it += gridDim.x) {
        const int2 ent = list[it];
        const int64_t rd = ent.x;
        const LadderDesc& ld = lads[ent.y].d;
        const int L = a.read_len[rd];
        if (L > 64 * R || L > TREDGPU_MAX_LONG_READ_LEN) {   // out of this path's range: flagged, not aligned
            if (lane == 0) { a.out_tag[rd] = TREDGPU_TAG_INVALID; a.out_h[rd] = 0; a.out_score[rd] = 0; }
            continue;
        }
        LongRows<R> J;
        J.row0 = lane * R;
        {
            const uint32_t* rec = a.packed + a.read_off[rd];
            const int nb = (L + 15) >> 4;
#pragma unroll
            for (int k = 0; k < R / 4; ++k) J.code[k] = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = J.row0 + r;
                int code = 5;
                if (i < L) code = ((rec[nb + (i >> 5)] >> (i & 31)) & 1u) ? 4 : (int)((rec[i >> 4] >> ((i & 15) * 2)) & 3u);
                J.code[r >> 2] |= (uint32_t)(5 * code) << ((r & 3) * 8);
            }
        }
        const int period = ld.period, max_units = ld.max_units;
        const int mu_rept = a.p.clip ? (L + period - 1) / period : max_units;
        int bestS = 0, bestU = 0, bestTag = TREDGPU_TAG_NONE;   // arg-max (score, -units), first in db order
        for (int s = 0; s < ld.n_strands; ++s) {
            const int alen = ld.alen[s], blen = ld.blen[s];
            const int ncols = alen + period * max_units;
            long long H[R], E[R];
#pragma unroll
            for (int r = 0; r < R; ++r) { H[r] = mk((J.row0 + r - 1) * ge, (uint32_t)(J.row0 + r + 1)); E[r] = mk(LNEG, 0); }
            LongBest T{mk(0, 0), 0};
            int u = max_units > 0 ? 1 : 0;
            int next_end = max_units > 0 ? alen + period - 1 : alen - 1;
            for (int col = 0; col < ncols; ++col) {
                long_column<R>(J, H, E, T, col, score_lut(ladder_letter(a.seqw, ld.trunk_off[s], col), a.p), ge, c0);
                if (col != next_end) continue;
                // ---- template u ends here on the trunk: sweep its suffix from the parked trunk state ----
                LongBest B = T;
                if (blen > 0) {
#pragma unroll
                    for (int r = 0; r < R; ++r) { park[(2 * r) * 64 + lane] = H[r]; park[(2 * r + 1) * 64 + lane] = E[r]; }
                    for (int j = 0; j < blen; ++j)
                        long_column<R>(J, H, E, B, col + 1 + j, score_lut(ladder_letter(a.seqw, ld.branch_off[s], j), a.p), ge, c0);
#pragma unroll
                    for (int r = 0; r < R; ++r) { H[r] = park[(2 * r) * 64 + lane]; E[r] = park[(2 * r + 1) * 64 + lane]; }
                }
                // the template's best cell over the wave: largest key (score, first column, smallest row)
                long long k = B.key;
                uint32_t st = B.start;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const long long k2 = shfl_xor64(k, d);
                    const uint32_t s2 = (uint32_t)__shfl_xor((int)st, d, 64);
                    st = k2 > k ? s2 : st;
                    k = max64(k, k2);
                }
                const int Tlen = alen + period * u + blen;
                const int score = hi_of(k);
                const bool hit = score > 0;
                const int ref_end = hit ? 0xFFFF - (int)(lo_of(k) >> 16) : -1;
                const int read_end = hit ? 0xFFFF - (int)(lo_of(k) & 0xFFFFu) : 0;
                const int ref_begin = hit ? (int)(st >> 16) : -1;
                const int read_begin = hit ? (int)(st & 0xFFFFu) : 0;
                const int min_len = min(L, Tlen) >> 1;              // bam_parser.py:133
                const int min_score = max(min_len, 30);             // :134
                const bool pass = score >= min_score && (read_end - read_begin + 1) >= min_len;  // ssw_wrap.py:217
                const int aL = ref_begin, aR = Tlen - ref_end - 1, bL = read_begin, bR = L - read_end - 1;
                const int hang = min(min(aR + bL, aL + bR), min(aL + aR, bL + bR));  // bam_parser.py:113-121
                const bool prefix_read = ref_begin < flank;                           // :139
                const bool suffix_read = ref_end > Tlen - flank - 1;                  // :140
                int tag;
                if (hang >= flank) tag = TREDGPU_TAG_HANG;
                else if (prefix_read) tag = suffix_read ? TREDGPU_TAG_FULL : TREDGPU_TAG_PREF;
                else if (suffix_read) tag = TREDGPU_TAG_POST;
                else if (u >= mu_rept - 1 && u * period <= L) tag = TREDGPU_TAG_REPT;
                else tag = TREDGPU_TAG_NONE;
                if (!pass) tag = TREDGPU_TAG_NONE;
                if (tag != TREDGPU_TAG_NONE && (bestTag == TREDGPU_TAG_NONE || score > bestS || (score == bestS && u < bestU))) {
                    bestS = score; bestU = u; bestTag = tag;
                }
                if (a.out_dump != nullptr && lane == 0) {
                    const int kk = max_units > 0 ? 2 * (u - 1) + s : 0;
                    if (kk < a.dump_templates) {
                        int16_t* dd = a.out_dump + ((int64_t)rd * a.dump_templates + kk) * 6;
                        dd[0] = (int16_t)(hit ? score : 0);
                        dd[1] = (int16_t)ref_begin;
                        dd[2] = (int16_t)ref_end;
                        dd[3] = (int16_t)read_begin;
                        dd[4] = (int16_t)read_end;
                        dd[5] = (int16_t)tag;
                    }
                }
                ++u;
                next_end += period;
            }
        }
        if (lane == 0) {
            a.out_tag[rd] = (uint8_t)bestTag;
            a.out_h[rd] = (int16_t)(bestTag == TREDGPU_TAG_NONE ? 0 : bestU);
            a.out_score[rd] = (int16_t)(bestTag == TREDGPU_TAG_NONE ? 0 : bestS);
        }
    }
}

}  // namespace
}  // namespace tredgpu

// ---- C entry points (include/tredlong.h) ----------------------------------------------------------------------
using namespace tredgpu;
using namespace ladder_host;

namespace tredgpu {
thread_local std::string g_long_error;   // the text of tredlong_last_error(); sw_cigar_long.hip writes it as well
}

namespace {

// device buffers of one call, released on every way out
struct DevBufs {
    std::vector<void*> p;
    ~DevBufs() { for (void* q : p) (void)hipFree(q); }
    template <typename T>
    hipError_t get(T** out, size_t n) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(n * sizeof(T), 16));
        if (e == hipSuccess) { p.push_back(q); *out = (T*)q; }
        return e;
    }
};

#define LCHK(expr)                                                                                       \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(g_long_error, -10, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

}  // namespace

extern "C" {

const char* tredlong_last_error(void) { return g_long_error.c_str(); }

int tredlong_sw_classify(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                             const char* const* suffix, const int32_t* max_units, const uint32_t* packed,
                             const int64_t* read_off, const int32_t* read_len, int64_t n_reads, const int32_t* read_ladder,
                             const tredgpu_sw_params* p, uint8_t* out_tag, int16_t* out_h, int16_t* out_score,
                             int16_t* out_dump, int32_t dump_templates) {
    g_long_error.clear();
    if (!ctx || !p) return fail(g_long_error, -2, "ctx or params is NULL");
    if (n_ladders <= 0 || !prefix || !repeat || !suffix || !max_units) return fail(g_long_error, -2, "bad ladder arguments");
    if (n_reads < 0) return fail(g_long_error, -2, "negative n_reads");
    if (n_reads > 0 && (!packed || !read_off || !read_len || !read_ladder || !out_tag || !out_h || !out_score))
        return fail(g_long_error, -2, "NULL array argument");
    if (out_dump && dump_templates <= 0) return fail(g_long_error, -2, "dump_templates must be > 0 with out_dump");
    if (const char* why = scoring_refusal(*p, true)) return fail(g_long_error, -2, "%s", why);
    // ladders: the layout of tredgpu_set_ladders (letters 8 per word, every segment on a word boundary)
    std::vector<uint32_t> seq;
    auto append = [&seq](const Codes& v) {
        const int off = (int)seq.size();
        seq.resize(seq.size() + (v.size() + 7) / 8 + 1, 0x44444444u);
        for (size_t i = 0; i < v.size(); ++i) {
            uint32_t& w = seq[off + i / 8];
            w = (w & ~(0xFu << ((i % 8) * 4))) | ((uint32_t)v[i] << ((i % 8) * 4));
        }
        return off;
    };
    std::vector<LongLadder> lad((size_t)n_ladders);
    Strands S;
    for (int i = 0; i < n_ladders; ++i) {
        LadderDesc& d = lad[i].d;
        memset(&lad[i], 0, sizeof lad[i]);
        if (const char* why = build_strands(prefix[i], repeat[i], suffix[i], max_units[i], S))
            return fail(g_long_error, -2, "ladder %d: %s", i, why);
        const size_t T = (size_t)S.alen[0] + S.blen[0] + (size_t)S.period * S.max_units;
        if (S.max_units == 0 && (T < 1 || T > TREDGPU_MAX_LONG_TEMPLATE_LEN))
            return fail(g_long_error, -2, "ladder %d: reference length %zu not in [1,%d]", i, T, TREDGPU_MAX_LONG_TEMPLATE_LEN);
        if (T > TREDGPU_MAX_LONG_TEMPLATE_LEN)
            return fail(g_long_error, -2, "ladder %d: longest template %zu exceeds TREDGPU_MAX_LONG_TEMPLATE_LEN=%d", i, T,
                        TREDGPU_MAX_LONG_TEMPLATE_LEN);
        for (int s = 0; s < S.n_strands; ++s) {
            d.alen[s] = S.alen[s];
            d.blen[s] = S.blen[s];
            d.trunk_off[s] = append(S.trunk[s]);
            d.branch_off[s] = append(S.branch[s]);
        }
        d.period = S.max_units > 0 ? S.period : 1;     // a plain reference: one template, one unit column wide
        d.max_units = S.max_units;
        d.n_strands = S.n_strands;
    }
    seq.resize(seq.size() + 4, 0x44444444u);
    if (n_reads == 0) return 0;
    // reads by row class (up to 512 / 1024 / 2048 bp)
    std::vector<int2> lists[3];
    for (int64_t r = 0; r < n_reads; ++r) {
        const int L = read_len[r];
        if (L < 0 || L > TREDGPU_MAX_LONG_READ_LEN)
            return fail(g_long_error, -5, "read of %d bp exceeds TREDGPU_MAX_LONG_READ_LEN=%d", L, TREDGPU_MAX_LONG_READ_LEN);
        if (read_ladder[r] < 0 || read_ladder[r] >= n_ladders) return fail(g_long_error, -2, "read %lld: ladder %d not given", (long long)r, read_ladder[r]);
        if (read_off[r + 1] - read_off[r] != ((L + 15) >> 4) + ((L + 31) >> 5))
            return fail(g_long_error, -2, "read %lld: read_off does not match read_len (tredgpu_pack_reads layout)", (long long)r);
        lists[L <= 512 ? 0 : (L <= 1024 ? 1 : 2)].push_back(make_int2((int)r, read_ladder[r]));
    }
    hipStream_t st = (hipStream_t)tredgpu_get_stream(ctx);
    int dev = 0;
    LCHK(hipStreamGetDevice(st, &dev));
    LCHK(hipSetDevice(dev));
    DevBufs b;
    uint32_t* d_packed; int64_t* d_off; int32_t* d_len; LongLadder* d_lad; uint32_t* d_seq; int2* d_list; int32_t* d_cnt;
    uint8_t* d_tag; int16_t *d_h, *d_score, *d_dump = nullptr;
    const size_t words = (size_t)read_off[n_reads], dump_n = out_dump ? (size_t)n_reads * dump_templates * 6 : 0;
    const size_t n_list = lists[0].size() + lists[1].size() + lists[2].size();
    LCHK(b.get(&d_packed, words));
    LCHK(b.get(&d_off, (size_t)n_reads + 1));
    LCHK(b.get(&d_len, (size_t)n_reads));
    LCHK(b.get(&d_lad, lad.size()));
    LCHK(b.get(&d_seq, seq.size()));
    LCHK(b.get(&d_list, n_list));
    LCHK(b.get(&d_cnt, 3));
    LCHK(b.get(&d_tag, (size_t)n_reads));
    LCHK(b.get(&d_h, (size_t)n_reads));
    LCHK(b.get(&d_score, (size_t)n_reads));
    if (out_dump) LCHK(b.get(&d_dump, dump_n));
    std::vector<int2> all;
    int32_t cnt[3];
    for (int k = 0; k < 3; ++k) { cnt[k] = (int32_t)lists[k].size(); all.insert(all.end(), lists[k].begin(), lists[k].end()); }
    LCHK(hipMemcpyAsync(d_packed, packed, words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    LCHK(hipMemcpyAsync(d_off, read_off, ((size_t)n_reads + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    LCHK(hipMemcpyAsync(d_len, read_len, (size_t)n_reads * sizeof(int32_t), hipMemcpyHostToDevice, st));
    LCHK(hipMemcpyAsync(d_lad, lad.data(), lad.size() * sizeof(LongLadder), hipMemcpyHostToDevice, st));
    LCHK(hipMemcpyAsync(d_seq, seq.data(), seq.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    LCHK(hipMemcpyAsync(d_list, all.data(), n_list * sizeof(int2), hipMemcpyHostToDevice, st));
    LCHK(hipMemcpyAsync(d_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice, st));
    if (out_dump) LCHK(hipMemsetAsync(d_dump, 0xFF, dump_n * sizeof(int16_t), st));
    SwArgs a;
    memset(&a, 0, sizeof a);
    a.packed = d_packed;
    a.read_off = d_off;
    a.read_len = d_len;
    a.seqw = d_seq;
    a.out_tag = d_tag;
    a.out_h = d_h;
    a.out_score = d_score;
    a.out_dump = d_dump;
    a.dump_templates = dump_templates;
    a.p = *p;
    // one wavefront per workgroup; each loops over its class's list
    const int2* at = d_list;
    if (cnt[0]) sw_long_kernel<8><<<(unsigned)std::min(cnt[0], 2048), 64, 0, st>>>(a, d_lad, at, d_cnt);
    at += cnt[0];
    if (cnt[1]) sw_long_kernel<16><<<(unsigned)std::min(cnt[1], 2048), 64, 0, st>>>(a, d_lad, at, d_cnt + 1);
    at += cnt[1];
    if (cnt[2]) sw_long_kernel<32><<<(unsigned)std::min(cnt[2], 2048), 64, 0, st>>>(a, d_lad, at, d_cnt + 2);
    LCHK(hipGetLastError());
    LCHK(hipMemcpyAsync(out_tag, d_tag, (size_t)n_reads, hipMemcpyDeviceToHost, st));
    LCHK(hipMemcpyAsync(out_h, d_h, (size_t)n_reads * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    LCHK(hipMemcpyAsync(out_score, d_score, (size_t)n_reads * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    if (out_dump) LCHK(hipMemcpyAsync(out_dump, d_dump, dump_n * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    LCHK(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
