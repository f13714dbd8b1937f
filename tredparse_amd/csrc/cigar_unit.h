// cigar_unit.h -- what the two CIGAR units (sw_cigar.hip: one lane one item; sw_cigar_long.hip: one wavefront one item)
// share on top of side_unit.h, so that an item is decoded, refused, traced back and reported by ONE text whichever unit
// Context.sw_cigar sends it to: argument block and the list of its arrays, item decode with its refusals, direction
// byte, traceback, epilogue.  A unit keeps its pass, kernels, workspaces, limits and error string.
#pragma once
#include "side_unit.h"
#include "../../include/tredcigar.h"

namespace cigar_unit {
using namespace side_unit;

struct Args {
    const uint32_t* packed;
    const int64_t* read_off;
    const int32_t *read_len, *item_ladder, *item_template;
    const int16_t* fields;
    const LadderRecord* ladders;
    const uint8_t* letters;
    int32_t n_ladders;
    int64_t n_items;
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t cap;
    uint32_t* out_ops;
    int32_t *out_n_ops, *out_status;
    uint8_t* plane;        // the direction plane, in the unit's layout
};

// an item the decode accepted: the rectangle ref[ref_begin..ref_end] x read[read_begin..read_end] and where its letters are
struct Item {
    int score, ref_begin, ref_end, read_begin, read_end;
    int L, refLen, readLen, trunk;     // template column c is tr[c] below trunk and br[c - trunk] from there on
    const uint8_t *tr, *br;
    const uint32_t* rec;               // the read's words: nb of 2-bit codes, then the N mask
    int nb;
};

// Decodes an item and hands it to the unit's pass, whose status it returns -- or the status of an item the unit does not
// take (max_read / max_template: the unit's limits).  The pass is a callable so that each refusal is a return of its own:
// behind a status merged from them the compiler no longer knows what the checks established (1 <= refLen, readLen <= 2^16).
template <class Pass>
__device__ __forceinline__ int decode_item(const Args& a, int64_t item, int max_read, int max_template, Pass pass) {
    const int lad = a.item_ladder[item], tpl = a.item_template[item];
    const int16_t* fl = a.fields + (size_t)item * 5;
    const int score = fl[0], ref_begin = fl[1], ref_end = fl[2], read_begin = fl[3], read_end = fl[4];
    const int L = a.read_len[item];
    if (lad < 0 || lad >= a.n_ladders) return TREDGPU_CIGAR_BAD_ITEM;
    const LadderRecord d = a.ladders[lad];       // (a copy indexed by strand, not template_of: the code object stays what it was)
    if (tpl < 0 || tpl >= (d.max_units > 0 ? 2 * d.max_units : 1)) return TREDGPU_CIGAR_BAD_ITEM;
    const int strand = d.max_units > 0 ? (tpl & 1) : 0;
    const int trunk = d.alen[strand] + (d.max_units > 0 ? d.period * (tpl / 2 + 1) : 0);
    const int tlen = trunk + d.blen[strand];
    if (L > max_read || tlen > max_template) return TREDGPU_CIGAR_TOO_LONG;
    if (ref_begin < 0 || ref_end < ref_begin || ref_end >= tlen || read_begin < 0 || read_end < read_begin || read_end >= L)
        return TREDGPU_CIGAR_BAD_ITEM;
    const Item it{score, ref_begin, ref_end, read_begin, read_end, L, ref_end - ref_begin + 1, read_end - read_begin + 1, trunk,
                  a.letters + d.trunk_off[strand], a.letters + d.branch_off[strand], a.packed + a.read_off[item], (L + 15) >> 4};
    return pass(it);
}

// the three direction codes of a cell in one byte: bit 0 E's (2/3), bit 1 F's (4/5), bits 2-4 H's (1-5)
__device__ __forceinline__ uint8_t dir_pack(int de, int df, int dh) { return (uint8_t)((de - 2) | ((df - 4) << 1) | (dh << 2)); }
// the step out of a cell the traceback entered in E (which 0), F (1) or H (2)
__device__ __forceinline__ int dir_step(int c, int which) { return which == 0 ? 2 + (c & 1) : which == 1 ? 4 + ((c >> 1) & 1) : (c >> 2); }

// The traceback of ssw.c:636-726 from the rectangle's last cell to row 0 over the plane of the pass whose band was bw;
// cell(i, j) is the byte of row i, column j in the unit's addressing.  Writes the item's operations and out_n_ops and
// returns its status.
template <class Cell>
__device__ __forceinline__ int traceback(const Args& a, int64_t item, const Item& it, int bw, Cell cell) {
    uint32_t* ops = a.out_ops + (size_t)item * a.cap;
    int i = it.readLen - 1, j = it.refLen - 1, e = 0, l = 0, which = 2, op = 0, prev = 0;
    auto emit = [&](uint32_t v) { if (l < a.cap) ops[l] = v; ++l; };
    while (i > 0) {
        if (j < max(0, i - bw) || j > i + bw) return TREDGPU_CIGAR_OFF_EDGE;          // a cell this pass never wrote
        switch (dir_step(cell(i, j), which)) {
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

// entries first, first + step, ... of the item's row of out_ops (a lane alone: 0, 1; a wavefront: lane, 64)
__device__ __forceinline__ void zero_ops(const Args& a, int64_t item, const int first, const int step) {
    uint32_t* ops = a.out_ops + (size_t)item * a.cap;
    for (int k = first; k < a.cap; k += step) ops[k] = 0;
}

// the status of a finished item; n_ops is the traceback's only where it ran to its end (OK, OVERFLOW).  An item that is
// not OK gets zero_ops as well.
__device__ __forceinline__ void store_status(const Args& a, int64_t item, int status) {
    a.out_status[item] = status;
    if (status != TREDGPU_CIGAR_OK && status != TREDGPU_CIGAR_OVERFLOW) a.out_n_ops[item] = 0;
}

// ---- host side --------------------------------------------------------------------------------------------------------
// the block of a call as the caller gave it (device memory: the kernels take it as it is), with the state's ladder table
inline void fill_args(Args& a, const StateBase& s, const uint32_t* packed, const int64_t* read_off, const int32_t* read_len,
                      int64_t n_items, const int32_t* item_ladder, const int32_t* item_template, const int16_t* fields,
                      const tredgpu_sw_params& p, int32_t cap, uint32_t* out_ops, int32_t* out_n_ops, int32_t* out_status) {
    fill_table(a, s, p);
    a.packed = packed; a.read_off = read_off; a.read_len = read_len;
    a.item_ladder = item_ladder; a.item_template = item_template; a.fields = fields;
    a.out_ops = out_ops; a.out_n_ops = out_n_ops; a.out_status = out_status;
    a.n_items = n_items;
    a.cap = cap;
}

// a host-memory call: the arrays `a` points to, for stage() before the launches and read_back() after them
inline std::vector<Array> host_arrays(Args& a) {
    const size_t n = (size_t)a.n_items;
    return {arr_in(a.packed, a.packed, (size_t)a.read_off[n]), arr_in(a.read_off, a.read_off, n + 1), arr_in(a.read_len, a.read_len, n),
            arr_in(a.item_ladder, a.item_ladder, n), arr_in(a.item_template, a.item_template, n), arr_in(a.fields, a.fields, n * 5),
            arr_out(a.out_ops, a.out_ops, n * a.cap), arr_out(a.out_n_ops, a.out_n_ops, n), arr_out(a.out_status, a.out_status, n)};
}

}  // namespace cigar_unit
