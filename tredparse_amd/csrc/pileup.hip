// pileup.hip -- per-allele evidence from per-read alignments (tredpileup_pileup, include/tredpileup.h): the items of a
// group -- (read, template, fields, CIGAR operations) as tredcigar_sw_cigar takes and returns them -- counted column by
// column of the group's forward template into int32 [n_groups][stride][8].  A unit of its own, outside the source hash
// the profiles are tied to (csrc/Makefile); the harness is side_unit.h's and ladder_host.h's.
//
// Two kernels per call.
//   * validate_kernel, one lane per item: every refusal of the header that an item can be given on its own (indices,
//     lengths, fields, the operations and their sums) -> pre[item] and out_status[item].  Nothing an item names is used
//     as an index before the check that bounds it, and the counting kernel only ever looks at items with pre == OK.
//   * pileup_kernel, one WORKGROUP of four wavefronts per (group, 512-column tile), the work units taken grid-stride by
//     at most MAX_BLOCKS workgroups.  The host has sorted the items by group (order / goff: a CSR in the caller's order),
//     so a workgroup reads its group's list and nobody else's.  It zeroes 8 x 512 int32 counters in LDS (16 KB), finds
//     the group's first accepted item (an LDS atomicMin over the list) and with it the group's (ladder, units) and
//     length; then its wavefronts take the group's items in turn.  A wavefront walks the
//     item's operations -- the walk is uniform over the wave -- and its lanes spread over the columns of ONE operation,
//     intersected with the tile: they hit 64 different columns, and with the counters laid out [channel][column] 64
//     different LDS banks whatever the letters are.  Adds are ds_add_u32 (atomicAdd on LDS, result unused): two wavefronts
//     may be on the same column.  At the end the tile is stored once, with plain vector stores, coalesced, zeros included
//     -- every cell of out_counts has exactly one owner, there is no global atomic, and the result is exact and order-free.
//     The workgroup of a group's tile 0 also refuses the accepted items whose (ladder, units) is not the group's.
//   * counters are 32-bit: a group may hold any number of items a call can carry (n_items < 2^31).
//
// tredpileup_pileup_anchored is the same call with the group's shape GIVEN (group_ladder, group_units = a, which may lie
// beyond the ladder) and an anchor per item: validate_anchored_kernel adds the refusals that compare an item with its
// group, so pileup_anchored_kernel needs no first-item search, and an item of h < a units is counted by the SAME walker
// (count_item) with a window of its forward columns and slots and a shift -- the flank it is anchored in and the tract
// next to it land where they lie on the group's template, what it shows of the other flank is cut.
//
// tredpileup_unit_spectrum is position-free: per group the words of the repeat units its items show whole, per item how
// many of them are the motif.  validate_spectrum_kernel adds its refusals (the group's ladder, a tract, a period of at
// most 6); spectrum_kernel, one workgroup of four wavefronts per GROUP, keeps the 4^p bins and four sums in LDS (16 400 B),
// its wavefronts take the group's items in turn, and the lanes of one spread over the units that lie whole inside ONE M
// operation and add their word for themselves (ds_add_u32).  In a real tract nearly every lane adds to the motif's bin;
// counting that word with a ballot and one add per wave instead was measured and bought nothing -- the walk waits for an
// item's loads, not for LDS (DESIGN) -- so there is one path.  The row is stored once, whole: no global atomic, exact and
// order-free.
#include <climits>
#include <cstring>

#include "side_unit.h"
#include "../../include/tredlong.h"
#include "../../include/tredpileup.h"

namespace {
using namespace side_unit;

thread_local std::string g_pileup_error;   // the text of tredpileup_last_error()

constexpr int TILE = 512;                  // columns of a work unit
constexpr int CH = TREDGPU_PILEUP_CHANNELS;
constexpr int THREADS = 256, WAVES = THREADS / 64;
// workgroups of a launch at the most.  256 CUs hold 2 048 at once (8 each by registers: 48 VGPRs, 8 waves per SIMD; by
// LDS, 16 388 B, it would be 9), but a workgroup that takes a second unit is the launch's tail: 4 567 units took 0.061 ms
// on 2 048 workgroups, 0.056 ms on 2 560 and 0.054 ms on 4 096 (DESIGN, "Per-allele pileup and consensus")
constexpr int MAX_BLOCKS = 4096;

struct PileArgs {
    const uint32_t* packed;
    const int64_t* read_off;
    const int32_t *read_len, *item_ladder, *item_template;
    const int16_t* fields;
    const uint32_t* ops;
    const int32_t *n_ops, *item_group;
    const LadderRecord* ladders;
    int32_t n_ladders, cap, n_groups, stride, ntile;
    int64_t n_items;
    const int32_t* order;      // the items with a group in range, sorted by group, the caller's order within a group
    const int64_t* goff;       // [n_groups + 1] into order
    int32_t* pre;              // [n_items]: the status of validate_kernel
    int32_t* out_counts;       // [n_groups][stride][CH]
    int32_t* out_status;
    const int32_t *item_anchor, *group_ladder, *group_units;     // the anchored entry's; NULL otherwise
    const uint8_t* letters;    // fill_table's other fields: the letters are read by spectrum_kernel alone (the motif)
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t* out_item;         // [n_items][3], the spectrum entry's; its row of a group is out_counts [n_groups][SROW]
};

__device__ int validate(const PileArgs& a, int64_t item) {
    const int g = a.item_group[item];
    if (g < 0 || g >= a.n_groups) return TREDGPU_PILEUP_BAD_ITEM;
    const int lad = a.item_ladder[item], tpl = a.item_template[item];
    if (lad < 0 || lad >= a.n_ladders) return TREDGPU_PILEUP_BAD_ITEM;
    const LadderRecord d = a.ladders[lad];                           // (a copy, and no field by strand: see template_of)
    if (tpl < 0 || tpl >= n_templates(d)) return TREDGPU_PILEUP_BAD_ITEM;
    const int tlen = template_len(d, tpl), L = a.read_len[item];
    if (L > TREDGPU_MAX_LONG_READ_LEN || tlen > TREDGPU_MAX_LONG_TEMPLATE_LEN) return TREDGPU_PILEUP_TOO_LONG;
    const int16_t* fl = a.fields + (size_t)item * 5;
    const int ref_begin = fl[1], ref_end = fl[2], read_begin = fl[3], read_end = fl[4];
    if (ref_begin < 0 || ref_end < ref_begin || ref_end >= tlen || read_begin < 0 || read_end < read_begin || read_end >= L)
        return TREDGPU_PILEUP_BAD_ITEM;
    const int n = a.n_ops[item];
    if (n < 1 || n > a.cap) return TREDGPU_PILEUP_BAD_ITEM;
    const uint32_t* ops = a.ops + (size_t)item * a.cap;
    int64_t on_ref = 0, on_read = 0;
    for (int j = 0; j < n; ++j) {
        const uint32_t op = ops[j] & 15u, len = ops[j] >> 4;
        if (op > 2u || len == 0u) return TREDGPU_PILEUP_BAD_ITEM;
        if (op != 1u) on_ref += len;
        if (op != 2u) on_read += len;
    }
    if (on_ref != ref_end - ref_begin + 1 || on_read != read_end - read_begin + 1) return TREDGPU_PILEUP_BAD_ITEM;
    return TREDGPU_PILEUP_OK;
}

__global__ __launch_bounds__(256) void validate_kernel(PileArgs a) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.n_items) return;
    const int status = validate(a, item);
    a.pre[item] = status;
    a.out_status[item] = status;
}

// validate, then what the anchored entry asks of an item against its group (whose ladder and units the host has checked):
// the group's ladder, a ladder with a tract, an anchor of 0..2, no more units than the group, and all of them when WHOLE
__device__ int validate_anchored(const PileArgs& a, int64_t item) {
    const int status = validate(a, item);
    if (status != TREDGPU_PILEUP_OK) return status;
    const int g = a.item_group[item], lad = a.item_ladder[item];   // both in range: validate has looked
    if (lad != a.group_ladder[g] || a.ladders[lad].max_units <= 0) return TREDGPU_PILEUP_BAD_ITEM;
    const int anchor = a.item_anchor[item], h = a.item_template[item] / 2 + 1, units = a.group_units[g];
    if (anchor < TREDGPU_PILEUP_ANCHOR_WHOLE || anchor > TREDGPU_PILEUP_ANCHOR_END) return TREDGPU_PILEUP_BAD_ITEM;
    if (h > units || (anchor == TREDGPU_PILEUP_ANCHOR_WHOLE && h != units)) return TREDGPU_PILEUP_BAD_ITEM;
    return TREDGPU_PILEUP_OK;
}

__global__ __launch_bounds__(256) void validate_anchored_kernel(PileArgs a) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.n_items) return;
    const int status = validate_anchored(a, item);
    a.pre[item] = status;
    a.out_status[item] = status;
}

// one operation of an item: M = 0, I = 1, D = 2 and its length
struct Op { int op, len; };
__device__ __forceinline__ Op op_of(uint32_t v) { return {(int)(v & 15u), (int)(v >> 4)}; }

// The forward columns [col_lo, col_hi) and slots [slot_lo, slot_hi) of an item's OWN template that count, and what is added
// to them on the way to the group's table.  whole(T): all of a template of T columns, where it lies.
struct Window { int col_lo, col_hi, slot_lo, slot_hi, shift; };
__device__ __forceinline__ Window whole(int T) { return {0, T, 0, T + 1, 0}; }

// One accepted item into the tile [tile0, tile0 + TILE) of cnt ([CH][TILE]); T: the length of the item's own template, w:
// what of it counts.  The whole wavefront is here with the same item.
__device__ __forceinline__ void count_item(const PileArgs& a, int64_t item, int strand, int T, const Window w, int tile0, int* cnt) {
    const int lane = threadIdx.x & 63;
    const int16_t* fl = a.fields + (size_t)item * 5;
    const int ref_begin = fl[1], ref_end = fl[2];
    // the forward columns and slots the item can touch: its columns and the slot behind the last, as far as they count
    const int lo = max(strand ? T - 1 - ref_end : ref_begin, min(w.col_lo, w.slot_lo));
    const int hi = min(strand ? T - ref_begin : ref_end + 1, max(w.col_hi, w.slot_hi) - 1);
    if (hi + w.shift < tile0 || lo + w.shift >= tile0 + TILE) return;
    // the tile in the item's own forward columns, cut to the window
    const int org = tile0 - w.shift, wlo = max(w.col_lo, org), whi = min(w.col_hi, org + TILE);
    const uint32_t* rec = a.packed + a.read_off[item];
    const int nb = (a.read_len[item] + 15) >> 4;
    const uint32_t* ops = a.ops + (size_t)item * a.cap;
    const int n = a.n_ops[item];
    int r = ref_begin, q = fl[3];
    for (int j = 0; j < n; ++j) {
        const auto [op, len] = op_of(ops[j]);
        if (op == 1) {                                             // an insertion before column r of the item's strand
            const int fwd = strand ? T - r : r, slot = fwd - org;
            if (lane == 0 && fwd >= w.slot_lo && fwd < w.slot_hi && slot >= 0 && slot < TILE) {
                atomicAdd(&cnt[6 * TILE + slot], 1);
                atomicAdd(&cnt[7 * TILE + slot], len);
            }
            q += len;
            continue;
        }
        // k in [klo, khi): the steps of the operation whose forward column r + k, or T - 1 - r - k, lies in [wlo, whi)
        const int base = strand ? T - 1 - r : r;
        const int klo = strand ? max(0, base - whi + 1) : max(0, wlo - base);
        const int khi = strand ? min(len, base - wlo + 1) : min(len, whi - base);
        for (int k = klo + lane; k < khi; k += 64) {
            const int col = (strand ? base - k : base + k) - org;
            int ch = 5;
            if (op == 0) {
                const int code = read_code(rec, nb, q + k);
                ch = (strand && code < 4) ? 3 - code : code;
            }
            atomicAdd(&cnt[ch * TILE + col], 1);
        }
        r += len;
        if (op == 0) q += len;
    }
}

// a work unit's counters: zeroed by the whole workgroup, and stored once with plain vector stores, zeros included
__device__ __forceinline__ void zero_tile(int* cnt) {
    for (int k = threadIdx.x; k < CH * TILE; k += THREADS) cnt[k] = 0;
}
__device__ __forceinline__ void store_tile(const PileArgs& a, int g, int tile0, const int* cnt) {
    int32_t* out = a.out_counts + ((size_t)g * a.stride + tile0) * CH;
    const int cols = min(TILE, a.stride - tile0);
    for (int k = threadIdx.x; k < cols * CH; k += THREADS) out[k] = cnt[(k % CH) * TILE + k / CH];
}

__global__ __launch_bounds__(THREADS) void pileup_kernel(PileArgs a) {
    __shared__ int cnt[CH * TILE];
    __shared__ int first;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_work = (int64_t)a.n_groups * a.ntile;
    for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int g = (int)(w / a.ntile), tile0 = (int)(w % a.ntile) * TILE;
        const int64_t lo = a.goff[g], hi = a.goff[g + 1];
        __syncthreads();                                           // the unit before has stored its tile
        zero_tile(cnt);
        if (threadIdx.x == 0) first = INT_MAX;
        __syncthreads();
        for (int64_t k = lo + threadIdx.x; k < hi; k += THREADS)
            if (a.pre[a.order[k]] == TREDGPU_PILEUP_OK) { atomicMin(&first, (int)(k - lo)); break; }
        __syncthreads();
        const int f = first;
        if (f != INT_MAX) {
            const int it0 = a.order[lo + f];                       // accepted: its ladder and template are in range
            const int lad0 = a.item_ladder[it0], units0 = a.item_template[it0] >> 1;
            const LadderRecord d = a.ladders[lad0];
            const int T = template_len(d, 2 * units0);
            for (int64_t k = lo + wave; k < hi; k += WAVES) {
                const int item = a.order[k];
                if (a.pre[item] != TREDGPU_PILEUP_OK) continue;
                const int tpl = a.item_template[item];
                if (a.item_ladder[item] != lad0 || (tpl >> 1) != units0) {
                    if (tile0 == 0 && lane == 0) a.out_status[item] = TREDGPU_PILEUP_BAD_ITEM;
                    continue;
                }
                if (tile0 <= T) count_item(a, item, d.max_units > 0 ? (tpl & 1) : 0, T, whole(T), tile0, cnt);
            }
        }
        __syncthreads();
        store_tile(a, g, tile0, cnt);
    }
}

// The same work units with the group's shape given: every accepted item of the list belongs to the group (validate_anchored),
// so there is nothing to search or to refuse here.  An item of the group's own units counts whole; a shorter one keeps the
// flank it is anchored in and the tract next to it -- LEFT of the forward template for BEGIN on a forward and END on a
// reverse-complement template, RIGHT otherwise, and RIGHT is shifted by the units the group has more.
__global__ __launch_bounds__(THREADS) void pileup_anchored_kernel(PileArgs a) {
    __shared__ int cnt[CH * TILE];
    const int wave = threadIdx.x >> 6;
    const int64_t n_work = (int64_t)a.n_groups * a.ntile;
    for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int g = (int)(w / a.ntile), tile0 = (int)(w % a.ntile) * TILE;
        const int64_t lo = a.goff[g], hi = a.goff[g + 1];
        __syncthreads();                                           // the unit before has stored its tile
        zero_tile(cnt);
        __syncthreads();
        const LadderRecord d = a.ladders[a.group_ladder[g]];       // (in range: the host has looked)
        const int units = a.group_units[g], P = d.alen[0], p = d.period;
        if (tile0 <= P + p * units + d.blen[0])
            for (int64_t k = lo + wave; k < hi; k += WAVES) {
                const int item = a.order[k];
                if (a.pre[item] != TREDGPU_PILEUP_OK) continue;
                const int tpl = a.item_template[item], h = tpl / 2 + 1, strand = tpl & 1, T = P + p * h + d.blen[0];
                Window win = whole(T);
                if (h != units) {
                    const bool left = (a.item_anchor[item] == TREDGPU_PILEUP_ANCHOR_BEGIN) != (strand == 1);
                    win = left ? Window{0, P + p * h, 0, P + p * h, 0} : Window{P, T, P + 1, T + 1, (units - h) * p};
                }
                count_item(a, item, strand, T, win, tile0, cnt);
            }
        __syncthreads();
        store_tile(a, g, tile0, cnt);
    }
}

// ---- the repeat-unit spectrum ------------------------------------------------------------------------------------------
constexpr int BINS = TREDGPU_SPECTRUM_BINS, SROW = TREDGPU_SPECTRUM_STRIDE, MAX_PERIOD = TREDGPU_SPECTRUM_MAX_PERIOD;
static_assert(BINS == 1 << (2 * MAX_PERIOD) && SROW == BINS + 4, "the row is 4^6 bins and four sums");

// validate, then what the spectrum entry asks of an item against its group: the group's ladder, a ladder with a tract,
// and a period the table has bins for
__device__ int validate_spectrum(const PileArgs& a, int64_t item) {
    const int status = validate(a, item);
    if (status != TREDGPU_PILEUP_OK) return status;
    const int g = a.item_group[item], lad = a.item_ladder[item];   // both in range: validate has looked
    if (lad != a.group_ladder[g] || a.ladders[lad].max_units <= 0) return TREDGPU_PILEUP_BAD_ITEM;
    if (a.ladders[lad].period > MAX_PERIOD) return TREDGPU_PILEUP_PERIOD;
    return TREDGPU_PILEUP_OK;
}

__global__ __launch_bounds__(256) void validate_spectrum_kernel(PileArgs a) {
    const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= a.n_items) return;
    const int status = validate_spectrum(a, item);
    a.pre[item] = status;
    a.out_status[item] = status;
    for (int k = 0; k < 3; ++k) a.out_item[item * 3 + k] = 0;      // (an accepted item's triple is spectrum_kernel's)
}

// what one accepted item adds: units whole inside one M operation (clean), those of them with an N, those equal to the
// motif, and the units its span touches.  All four are the same in every lane.
struct Units { int clean, with_n, motif, touched; };

// One accepted item of a ladder (P, p, S: the lengths of prefix, repeat, suffix; motif: the repeat's code, -1 with an N)
// into the group's bins.  The whole wavefront is here with the same item.
__device__ __forceinline__ Units spectrum_item(const PileArgs& a, int item, int P, int p, int S, int motif, int* spec) {
    const int lane = threadIdx.x & 63;
    const int tpl = a.item_template[item], h = tpl / 2 + 1, strand = tpl & 1, T = P + p * h + S;
    const int16_t* fl = a.fields + (size_t)item * 5;
    const int ref_begin = fl[1], ref_end = fl[2];
    Units u = {0, 0, 0, 0};
    // the span in forward columns, D columns included, cut to the tract [P, P + p h)
    const int tlo = max(strand ? T - 1 - ref_end : ref_begin, P), thi = min(strand ? T - 1 - ref_begin : ref_end, P + p * h - 1);
    if (tlo <= thi) u.touched = (thi - P) / p - (tlo - P) / p + 1;
    const uint32_t* rec = a.packed + a.read_off[item];
    const int nb = (a.read_len[item] + 15) >> 4;
    const uint32_t* ops = a.ops + (size_t)item * a.cap;
    const int n = a.n_ops[item];
    int r = ref_begin, q = fl[3];
    for (int j = 0; j < n; ++j) {
        const auto [op, len] = op_of(ops[j]);
        if (op == 0) {
            // the operation's forward columns [fa, fb) and the units [k_lo, k_hi) that lie whole inside them
            const int fa = strand ? T - r - len : r, fb = fa + len;
            const int k_lo = (max(fa, P) - P + p - 1) / p, k_hi = fb > P ? min(h, (fb - P) / p) : 0;
            for (int k0 = k_lo; k0 < k_hi; k0 += 64) {
                const int k = k0 + lane;
                const bool on = k < k_hi;
                int code = 0;
                bool has_n = false;
                if (on)
                    for (int i = 0; i < p; ++i) {                  // forward order: on strand 1 the read backwards, complemented
                        const int f = P + p * k + i, c = strand ? T - 1 - f : f;
                        const int x = read_code(rec, nb, q + (c - r));
                        has_n |= x > 3;
                        code = code * 4 + ((strand ? 3 - x : x) & 3);
                    }
                const bool word = on && !has_n;
                if (word) atomicAdd(&spec[code], 1);
                u.clean += min(64, k_hi - k0);
                u.with_n += __popcll(__ballot(on && has_n));
                u.motif += __popcll(__ballot(word && code == motif));
            }
        }
        if (op != 1) r += len;
        if (op != 2) q += len;
    }
    return u;
}

__global__ __launch_bounds__(THREADS) void spectrum_kernel(PileArgs a) {
    __shared__ int spec[SROW];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
        const int64_t lo = a.goff[g], hi = a.goff[g + 1];
        __syncthreads();                                           // the group before has stored its row
        for (int k = threadIdx.x; k < SROW; k += THREADS) spec[k] = 0;
        __syncthreads();
        const LadderRecord d = a.ladders[a.group_ladder[g]];       // (in range: the host has looked)
        const int P = d.alen[0], p = d.period, S = d.blen[0];
        if (d.max_units > 0 && p >= 1 && p <= MAX_PERIOD) {        // (otherwise validate_spectrum has accepted no item)
            int motif = 0;
            for (int i = 0; i < p; ++i) {
                const int c = a.letters[d.trunk_off[0] + P + i];
                motif = (c > 3 || motif < 0) ? -1 : motif * 4 + c;
            }
            Units sum = {0, 0, 0, 0};
            int accepted = 0;
            for (int64_t k = lo + wave; k < hi; k += WAVES) {
                const int item = __builtin_amdgcn_readfirstlane(a.order[k]);
                if (a.pre[item] != TREDGPU_PILEUP_OK) continue;
                const Units u = spectrum_item(a, item, P, p, S, motif, spec);
                if (lane == 0) {
                    int32_t* out = a.out_item + (size_t)item * 3;
                    out[0] = u.clean - u.with_n; out[1] = u.motif; out[2] = u.touched;
                }
                sum.clean += u.clean; sum.with_n += u.with_n; sum.touched += u.touched;
                accepted += 1;
            }
            if (lane == 0 && accepted) {
                atomicAdd(&spec[BINS + 0], sum.clean);
                atomicAdd(&spec[BINS + 1], sum.with_n);
                atomicAdd(&spec[BINS + 2], sum.touched);
                atomicAdd(&spec[BINS + 3], accepted);
            }
        }
        __syncthreads();
        int32_t* out = a.out_counts + (size_t)g * SROW;
        for (int k = threadIdx.x; k < SROW; k += THREADS) out[k] = spec[k];
    }
}

struct State : StateBase {};
Registry<State> g_states;

// The three entries.  anchor / group_ladder / group_units: the anchored entry's three arrays, all NULL for
// tredpileup_pileup.  The spectrum entry has group_ladder of them, out_item, and its row (SROW int32) where the others have
// stride columns of CH channels.
enum Entry { PLAIN, ANCHORED, SPECTRUM };
int run(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat, const char* const* suffix,
        const int32_t* max_units, const uint32_t* packed, const int64_t* read_off, const int32_t* read_len, int64_t n_items,
        const int32_t* item_ladder, const int32_t* item_template, const int16_t* fields, const uint32_t* ops, int32_t cap,
        const int32_t* n_ops, const int32_t* item_group, int32_t n_groups, int32_t stride, int32_t* out_counts,
        int32_t* out_status, Entry entry, const int32_t* item_anchor, const int32_t* group_ladder, const int32_t* group_units,
        int32_t* out_item) {
    const bool anchored = entry == ANCHORED, spectrum = entry == SPECTRUM;
    std::string& err = g_pileup_error;
    err.clear();
    const Table t{n_ladders, prefix, repeat, suffix, max_units};
    const tredgpu_sw_params any_scoring = {1, 5, 7, 2, 0, 0, 0, 0};     // (the scoring is not needed; the shared check wants one)
    int rc = call_refusal(err, ctx, true, t, n_items, cap, &any_scoring,
                          {packed, read_off, read_len, item_ladder, item_template, fields, ops, n_ops, item_group, out_status});
    if (rc) return rc;
    if (n_groups < 0 || (n_groups > 0 && !out_counts)) return fail(err, -2, "n_groups must not be negative, nor out_counts NULL");
    if (anchored && ((n_items > 0 && !item_anchor) || (n_groups > 0 && (!group_ladder || !group_units))))
        return fail(err, -2, "NULL array argument");
    if (spectrum && ((n_items > 0 && !out_item) || (n_groups > 0 && !group_ladder))) return fail(err, -2, "NULL array argument");
    size_t longest = 0;
    for (int i = 0; i < n_ladders; ++i) {
        if (!prefix[i] || !repeat[i] || !suffix[i]) return fail(err, -2, "ladder %d: NULL sequence", i);
        if (entry != PLAIN) continue;
        const size_t T = max_units[i] > 0 ? strlen(prefix[i]) + strlen(suffix[i]) + strlen(repeat[i]) * (size_t)max_units[i]
                                          : strlen(prefix[i]);
        longest = std::max(longest, std::min<size_t>(T, TREDGPU_MAX_LONG_TEMPLATE_LEN));
    }
    for (int g = 0; anchored && g < n_groups; ++g) {               // the shape is the group's own, wherever the ladder ends
        const int lad = group_ladder[g];
        if (lad < 0 || lad >= n_ladders) return fail(err, -2, "group %d: ladder %d out of range", g, lad);
        if (group_units[g] < 1) return fail(err, -2, "group %d: units %d must be at least 1", g, group_units[g]);
        longest = std::max(longest, strlen(prefix[lad]) + strlen(suffix[lad]) + strlen(repeat[lad]) * (size_t)group_units[g]);
    }
    for (int g = 0; spectrum && g < n_groups; ++g)
        if (group_ladder[g] < 0 || group_ladder[g] >= n_ladders) return fail(err, -2, "group %d: ladder %d out of range", g, group_ladder[g]);
    if (!spectrum && (stride <= 0 || (size_t)stride < longest + 1 || stride > TREDGPU_PILEUP_MAX_STRIDE))
        return fail(err, -2, "stride %d must be at least the largest template length + 1 = %zu and at most %d", stride,
                    longest + 1, TREDGPU_PILEUP_MAX_STRIDE);
    const size_t n = (size_t)n_items, cells = (size_t)n_groups * (spectrum ? (size_t)SROW : (size_t)stride * CH);
    if (n_items == 0 || n_groups == 0) {                           // nothing to launch: the table is written whole all the same
        if (cells) memset(out_counts, 0, cells * 4);
        if (spectrum && n) memset(out_item, 0, n * 3 * 4);
        for (size_t k = 0; k < n; ++k) out_status[k] = TREDGPU_PILEUP_BAD_ITEM;     // (no group is in range)
        return 0;
    }
    if ((rc = reads_refusal(err, read_off, read_len, n, TREDGPU_MAX_LONG_READ_LEN))) return rc;
    hipStream_t st;
    if ((rc = select_device(err, ctx, st))) return rc;
    State& s = *g_states.state_of(ctx);
    if ((rc = set_ladders(err, s, st, t, 0))) return rc;           // (a template beyond the limit is the item's TOO_LONG)

    // the items by group, in the caller's order within a group; an item whose group is out of range is in no list
    std::vector<int32_t> order;
    std::vector<int64_t> goff;
    bucket_order(n, (size_t)n_groups, [&](size_t k) { return item_group[k] < n_groups ? item_group[k] : -1; }, order, goff);

    PileArgs a{};
    fill_table(a, s, any_scoring);
    std::vector<Array> arrays = {
        arr_in(a.packed, packed, (size_t)read_off[n]), arr_in(a.read_off, read_off, n + 1), arr_in(a.read_len, read_len, n),
        arr_in(a.item_ladder, item_ladder, n), arr_in(a.item_template, item_template, n), arr_in(a.fields, fields, n * 5),
        arr_in(a.ops, ops, n * (size_t)cap), arr_in(a.n_ops, n_ops, n), arr_in(a.item_group, item_group, n),
        arr_in(a.order, order.data(), order.size()), arr_in(a.goff, goff.data(), goff.size()), arr_scratch(a.pre, n),
        arr_out(a.out_counts, out_counts, cells), arr_out(a.out_status, out_status, n)};
    if (anchored) {
        arrays.push_back(arr_in(a.item_anchor, item_anchor, n));
        arrays.push_back(arr_in(a.group_ladder, group_ladder, (size_t)n_groups));
        arrays.push_back(arr_in(a.group_units, group_units, (size_t)n_groups));
    }
    if (spectrum) {
        arrays.push_back(arr_in(a.group_ladder, group_ladder, (size_t)n_groups));
        arrays.push_back(arr_out(a.out_item, out_item, n * 3));
    }
    if ((rc = stage(err, s, st, arrays))) return rc;
    a.n_items = n_items; a.cap = cap; a.n_groups = n_groups; a.stride = stride; a.ntile = (stride + TILE - 1) / TILE;

    if ((rc = timed_begin(err, s, st))) return rc;
    const dim3 per_item((unsigned)((n + 255) / 256)), per_tile((unsigned)std::min<int64_t>((int64_t)n_groups * a.ntile, MAX_BLOCKS));
    if (spectrum) {
        hipLaunchKernelGGL(validate_spectrum_kernel, per_item, dim3(256), 0, st, a);
        hipLaunchKernelGGL(spectrum_kernel, dim3((unsigned)std::min(n_groups, MAX_BLOCKS)), dim3(THREADS), 0, st, a);
    } else if (anchored) {
        hipLaunchKernelGGL(validate_anchored_kernel, per_item, dim3(256), 0, st, a);
        hipLaunchKernelGGL(pileup_anchored_kernel, per_tile, dim3(THREADS), 0, st, a);
    } else {
        hipLaunchKernelGGL(validate_kernel, per_item, dim3(256), 0, st, a);
        hipLaunchKernelGGL(pileup_kernel, per_tile, dim3(THREADS), 0, st, a);
    }
    if ((rc = timed_end(err, s, st))) return rc;
    return read_back(err, s, st, arrays);                          // (order and goff are read by their copies until the stream is drained)
}

}  // namespace

extern "C" {

int tredpileup_pileup(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                      const char* const* suffix, const int32_t* max_units, const uint32_t* packed, const int64_t* read_off,
                      const int32_t* read_len, int64_t n_items, const int32_t* item_ladder, const int32_t* item_template,
                      const int16_t* fields, const uint32_t* ops, int32_t cap, const int32_t* n_ops, const int32_t* item_group,
                      int32_t n_groups, int32_t stride, int32_t* out_counts, int32_t* out_status) {
    return run(ctx, n_ladders, prefix, repeat, suffix, max_units, packed, read_off, read_len, n_items, item_ladder, item_template,
               fields, ops, cap, n_ops, item_group, n_groups, stride, out_counts, out_status, PLAIN, nullptr, nullptr, nullptr, nullptr);
}

int tredpileup_pileup_anchored(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                               const char* const* suffix, const int32_t* max_units, const uint32_t* packed,
                               const int64_t* read_off, const int32_t* read_len, int64_t n_items, const int32_t* item_ladder,
                               const int32_t* item_template, const int16_t* fields, const uint32_t* ops, int32_t cap,
                               const int32_t* n_ops, const int32_t* item_group, const int32_t* item_anchor, int32_t n_groups,
                               const int32_t* group_ladder, const int32_t* group_units, int32_t stride, int32_t* out_counts,
                               int32_t* out_status) {
    return run(ctx, n_ladders, prefix, repeat, suffix, max_units, packed, read_off, read_len, n_items, item_ladder, item_template,
               fields, ops, cap, n_ops, item_group, n_groups, stride, out_counts, out_status, ANCHORED, item_anchor, group_ladder,
               group_units, nullptr);
}

int tredpileup_unit_spectrum(tredgpu_ctx* ctx, int32_t n_ladders, const char* const* prefix, const char* const* repeat,
                             const char* const* suffix, const int32_t* max_units, const uint32_t* packed,
                             const int64_t* read_off, const int32_t* read_len, int64_t n_items, const int32_t* item_ladder,
                             const int32_t* item_template, const int16_t* fields, const uint32_t* ops, int32_t cap,
                             const int32_t* n_ops, const int32_t* item_group, int32_t n_groups, const int32_t* group_ladder,
                             int32_t* out_spectrum, int32_t* out_item, int32_t* out_status) {
    return run(ctx, n_ladders, prefix, repeat, suffix, max_units, packed, read_off, read_len, n_items, item_ladder, item_template,
               fields, ops, cap, n_ops, item_group, n_groups, SROW, out_spectrum, out_status, SPECTRUM, nullptr, group_ladder,
               nullptr, out_item);
}

int tredpileup_get_timing(tredgpu_ctx* ctx, int64_t* launches, double* total_ms) { return timing(g_pileup_error, g_states, ctx, launches, total_ms, false); }

int tredpileup_reset_timing(tredgpu_ctx* ctx) { return timing(g_pileup_error, g_states, ctx, nullptr, nullptr, true); }

void tredpileup_release(tredgpu_ctx* ctx) { release(g_states, ctx, {}); }

const char* tredpileup_last_error(void) { return g_pileup_error.c_str(); }

}  // extern "C"
