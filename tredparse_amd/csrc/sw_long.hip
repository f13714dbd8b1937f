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
#include "side_unit.h"
#include "../../include/tredlong.h"

namespace tredgpu {
namespace {
using namespace side_unit;

struct LongArgs {
    const LadderRecord* ladders;
    const uint8_t* letters;
    int32_t n_ladders;
    int32_t match, mismatch, gap_open, gap_extend;
    const uint32_t* packed;
    const int64_t* read_off;
    const int32_t *read_len, *read_ladder;
    int32_t flank, clip;
    const int32_t* list;       // the reads of this launch's row class
    int32_t n_list;
    uint8_t* out_tag;
    int16_t *out_h, *out_score, *out_dump;
    int32_t dump_templates;
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

// Ladder letters: one per byte of the pool; the index is wave-uniform, and the letter comes out of the aligned word that
// holds its byte (the pool ends in 16 bytes of padding, and its buffer begins on a word boundary).
__device__ __forceinline__ int ladder_letter(const uint8_t* letters, int off, int idx) {
    const int at = off + idx;
    const uint32_t w = ((const uint32_t*)letters)[at >> 2];
    return (int)((w >> ((at & 3) * 8)) & 7u);
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
    long long F = wave_excl_max(run, lane, mk(LNEG, 0));
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

template <int R>
__global__ __launch_bounds__(64) void sw_long_kernel(LongArgs a) {
    // the trunk state parked while a template's suffix is swept: H and E of every row
    __shared__ long long park[2 * R * 64];
    const int lane = __lane_id();
    const int n = a.n_list;
    const int ge = a.gap_extend, c0 = a.gap_open - a.gap_extend, flank = a.flank;
    for (int it = blockIdx.x; it < n; it += gridDim.x) {
        const int64_t rd = a.list[it];
        const LadderRecord& ld = a.ladders[a.read_ladder[rd]];       // (the host has checked the index)
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
                if (i < L) code = read_code(rec, nb, i);
                J.code[r >> 2] |= (uint32_t)(5 * code) << ((r & 3) * 8);
            }
        }
        const int max_units = ld.max_units, n_strands = max_units > 0 ? 2 : 1;
        const int period = max_units > 0 ? ld.period : 1;           // a plain reference: one template, one unit column wide
        const int mu_rept = a.clip ? (L + period - 1) / period : max_units;
        int bestS = 0, bestU = 0, bestTag = TREDGPU_TAG_NONE;   // arg-max (score, -units), first in db order
        for (int s = 0; s < n_strands; ++s) {
            const int alen = ld.alen[s], blen = ld.blen[s];
            const int ncols = alen + period * max_units;
            long long H[R], E[R];
#pragma unroll
            for (int r = 0; r < R; ++r) { H[r] = mk((J.row0 + r - 1) * ge, (uint32_t)(J.row0 + r + 1)); E[r] = mk(LNEG, 0); }
            LongBest T{mk(0, 0), 0};
            int u = max_units > 0 ? 1 : 0;
            int next_end = max_units > 0 ? alen + period - 1 : alen - 1;
            for (int col = 0; col < ncols; ++col) {
                long_column<R>(J, H, E, T, col, score_lut(ladder_letter(a.letters, ld.trunk_off[s], col), a.match, a.mismatch), ge, c0);
                if (col != next_end) continue;
                // ---- template u ends here on the trunk: sweep its suffix from the parked trunk state ----
                LongBest B = T;
                if (blen > 0) {
#pragma unroll
                    for (int r = 0; r < R; ++r) { park[(2 * r) * 64 + lane] = H[r]; park[(2 * r + 1) * 64 + lane] = E[r]; }
                    for (int j = 0; j < blen; ++j)
                        long_column<R>(J, H, E, B, col + 1 + j, score_lut(ladder_letter(a.letters, ld.branch_off[s], j), a.match, a.mismatch), ge, c0);
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

// ---- C entry points (include/tredlong.h); host side: side_unit.h ---------------------------------------------------
using namespace tredgpu;
using namespace side_unit;

namespace tredgpu {
thread_local std::string g_long_error;   // the text of tredlong_last_error(); sw_cigar_long.hip writes it as well
}

namespace {
struct State : StateBase {};
Registry<State> g_states;
}  // namespace

namespace tredgpu {
void long_classify_release(tredgpu_ctx* ctx) { release(g_states, ctx, {}); }   // tredlong_release's half (sw_cigar_long.hip)
}

extern "C" {

const char* tredlong_last_error(void) { return g_long_error.c_str(); }

int tredlong_sw_classify(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                             const char* const* suffix, const int32_t* max_units, const uint32_t* packed,
                             const int64_t* read_off, const int32_t* read_len, int64_t n_reads, const int32_t* read_ladder,
                             const tredgpu_sw_params* p, uint8_t* out_tag, int16_t* out_h, int16_t* out_score,
                             int16_t* out_dump, int32_t dump_templates) {
    std::string& err = g_long_error;
    err.clear();
    if (!ctx || !p) return fail(err, -2, "ctx or params is NULL");
    if (n_ladders <= 0 || !prefix || !repeat || !suffix || !max_units) return fail(err, -2, "bad ladder arguments");
    if (n_reads < 0) return fail(err, -2, "negative n_reads");
    if (n_reads > 0 && (!packed || !read_off || !read_len || !read_ladder || !out_tag || !out_h || !out_score))
        return fail(err, -2, "NULL array argument");
    if (out_dump && dump_templates <= 0) return fail(err, -2, "dump_templates must be > 0 with out_dump");
    if (const char* why = scoring_refusal(*p, true)) return fail(err, -2, "%s", why);
    hipStream_t st;
    int rc;
    if ((rc = select_device(err, ctx, st))) return rc;
    State& s = *g_states.state_of(ctx);
    // (the table is checked whether or not there are reads; a NULL sequence in any ladder before the limits of the first)
    if ((rc = set_ladders(err, s, st, Table{n_ladders, prefix, repeat, suffix, max_units}, TREDGPU_MAX_LONG_TEMPLATE_LEN, true)))
        return rc;
    if (n_reads == 0) return 0;
    const size_t n = (size_t)n_reads;
    for (size_t r = 0; r < n; ++r) {
        const int L = read_len[r];
        if (L < 0 || L > TREDGPU_MAX_LONG_READ_LEN)
            return fail(err, -5, "read of %d bp exceeds TREDGPU_MAX_LONG_READ_LEN=%d", L, TREDGPU_MAX_LONG_READ_LEN);
        if (read_ladder[r] < 0 || read_ladder[r] >= n_ladders) return fail(err, -2, "read %lld: ladder %d not given", (long long)r, read_ladder[r]);
        if (read_off[r + 1] - read_off[r] != ((L + 15) >> 4) + ((L + 31) >> 5))
            return fail(err, -2, "read %lld: read_off does not match read_len (tredgpu_pack_reads layout)", (long long)r);
    }
    if ((rc = reads_refusal(err, read_off, read_len, n, -1))) return rc;
    // reads by row class (up to 512 / 1024 / 2048 bp)
    std::vector<int32_t> list;
    std::vector<int64_t> first;
    bucket_order(n, 3, [&](size_t r) { return read_len[r] <= 512 ? 0 : (read_len[r] <= 1024 ? 1 : 2); }, list, first);

    LongArgs a{};
    fill_table(a, s, *p);
    a.flank = p->flank; a.clip = p->clip;
    a.dump_templates = dump_templates;
    const size_t dump_n = out_dump ? n * dump_templates * 6 : 0;
    const int32_t* d_list = nullptr;
    std::vector<Array> arrays = {
        arr_in(a.packed, packed, (size_t)read_off[n]), arr_in(a.read_off, read_off, n + 1), arr_in(a.read_len, read_len, n),
        arr_in(a.read_ladder, read_ladder, n), arr_in(d_list, list.data(), n), arr_out(a.out_tag, out_tag, n), arr_out(a.out_h, out_h, n),
        arr_out(a.out_score, out_score, n)};
    if (out_dump) arrays.push_back(arr_out(a.out_dump, out_dump, dump_n));       // (without it a.out_dump stays null)
    if ((rc = stage(err, s, st, arrays))) return rc;
    if (out_dump) SIDE_UNIT_CHK(err, hipMemsetAsync(a.out_dump, 0xFF, dump_n * sizeof(int16_t), st));
    // one wavefront per workgroup; each loops over its class's list
    auto launch = [&](int c, auto kernel) {
        a.list = d_list + first[c];
        a.n_list = (int32_t)(first[c + 1] - first[c]);
        if (a.n_list) hipLaunchKernelGGL(kernel, dim3((unsigned)std::min(a.n_list, 2048)), dim3(64), 0, st, a);
    };
    launch(0, sw_long_kernel<8>);
    launch(1, sw_long_kernel<16>);
    launch(2, sw_long_kernel<32>);
    SIDE_UNIT_CHK(err, hipGetLastError());
    return read_back(err, s, st, arrays);                          // (list is read by its copy until the stream is drained)
}

}  // extern "C"
