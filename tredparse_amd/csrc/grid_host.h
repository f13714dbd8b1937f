// grid_host.h -- what the host and the device share about the likelihood grid's scratch, free of HIP
// (tests/grid_host_main.cpp runs it under the sanitizers): the ONE layout of a unit's slot (grid_prepare_kernel lays a unit out with
// unit_layout(), the host sizes the pool with it at the worst admissible arguments), unit_items(), and plan_grid(): a call's workspace.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

#if defined(__HIPCC__)
#define GRID_HD __host__ __device__
#else
#define GRID_HD
#endif

namespace tredgpu {

constexpr int GRID_MAX_ROWS = 1024, GRID_MAX_COLS = 1024;  // |h1range| / |h2range| the grid kernels accept (status -5 beyond)
constexpr int GRID_SPAN = 1000;      // TREDGPU_SPAN: the length of a unit's KDE
constexpr int MAXOBS = 256, MAXM = 768;  // distinct FULL / PREF sizes per unit; marginal bins (repeat units)
constexpr int TQ = 16;    // ticket queues, regions of the work-item list, and the most sub-pools (GridCounters, grid.hip)
constexpr int CB = 64, RG = 128;   // columns and rows per work item of grid_pairs_kernel: one lane owns one h2 for all the item's rows
constexpr int TC = 32;    // spanning pairs per pass over the rows (the lane's roll(h2) values stay in registers)
constexpr int RS = 16;    // short grids (up to RS rows): one item takes all the column blocks, so the unit is looked up once
// bytes of grid.hip's private records (it asserts them): a UnitDesc, a work item's unit + arg-max record, a pass' counter block
constexpr size_t GRID_DESC_BYTES = 216, GRID_ITEM_BYTES = 4 + 16, GRID_COUNTER_BYTES = 64 * (6 * TQ + 1);
struct Obs {
    int fullK[MAXOBS], fullC[MAXOBS], partK[MAXOBS], partC[MAXOBS];
    int base[MAXOBS + 1], nF, nP, nb;
};
// Where one unit's tables live in the pool (doubles from the unit's base).  T: int32_t on the device, 64 bits for the host's bound
template <class T> struct SlotLayoutT { T obs, rowoff, far1, far2, near1, near2, rept, roll1, roll2, ml, total; };
using SlotLayout = SlotLayoutT<int32_t>;
template <class T = int32_t>
GRID_HD inline SlotLayoutT<T> unit_layout(T nrow, T ncol, T nt, bool run_pe, bool haploid, T dmax, T n_near) {
    SlotLayoutT<T> L;
    T o = 0;
    L.obs = o;    o += (T)((sizeof(Obs) + 7) / 8);
    L.rowoff = o; o += (nrow + 2) / 2;
    L.far1 = o;   o += nrow;
    L.far2 = o;   o += nrow;
    L.near1 = o;  o += nrow * n_near;
    L.near2 = o;  o += nrow * n_near;
    L.rept = o;   o += dmax + 1;
    L.roll1 = o;  o += run_pe ? nrow * ((nt + 31) & ~(T)31) : 0;   // rows padded to 32 entries
    L.roll2 = o;  o += run_pe && !haploid ? ncol * nt : 0;
    L.ml = o;     o += nrow * ncol;
    L.total = (o + 15) & ~(T)15;   // slots start on 128-byte lines
    return L;
}
GRID_HD inline int unit_items(int nrow, int ncol) { return nrow <= RS ? 1 : ((ncol + CB - 1) / CB) * ((nrow + RG - 1) / RG); }

// The largest dmax = 2 * max(hmaxv - readlen, 1) grid_prepare_kernel can hand to unit_layout: it refuses a unit unless
// hmaxv / period < MAXM and 1 <= period < 18 (status -5, -7), so hmaxv <= MAXM * 17 - 1.
// Premise: readlen >= 0.  Nothing in the library enforces it -- tredgpu_unit_params.readlen is not looked at by check_unit
// (HOST memory) and cannot be by a DEVICE-memory call; the Engine fills it with the longest read of the BAM.  A unit with a
// negative readlen and axis values near the MAXM limit can ask for a longer repeat-only table than this bound holds: it
// is then deferred in every pass, and the call ends with -10 like any unit larger than its sub-pool.
constexpr int GRID_DMAX = 2 * (MAXM * 17 - 1);
// Largest slot (doubles) a unit within the caps can ask for, nt_max = most spanning pairs of any unit: the layout at the caps with every
// table present and as long as it gets (every column near, a diploid's paired-end tables) -- unit_layout grows with each argument.
inline size_t grid_slot_doubles_max(int rows_cap, int cols_cap, int nt_max) {
    return (size_t)unit_layout<int64_t>(rows_cap, cols_cap, std::max(nt_max, 0), true, false, GRID_DMAX, cols_cap).total;
}

// Every size of one call's workspace.  The scratch pool is everything the batch can ask for if that is small, else
// pool_limit_bytes (TREDGPU_GRID_POOL_MB; never less than one slot) and as many passes as it takes: units that find their
// sub-pool full are deferred to the next pass.  The kernels use the pool as n_sub sub-pools, unit g in sub-pool g % n_sub,
// and the work-item list as TQ regions, unit g in region g % TQ.
struct GridPlan {
    int n_units, max_target, cap;     // cap: most rows / columns of a unit, beyond it the unit is refused (-5)
    size_t slot_doubles, slot_room;   // grid_slot_doubles_max(cap, cap, max_target); in bytes with a line of slack
    size_t all_bytes, pool_doubles;   // bytes the batch can ask for at most
    bool may_defer;            // the pool is smaller than that: the deferred count is read back after every pass
    int n_sub;                 // a power of two, at most TQ: as many sub-pools as still hold the largest slot each
    unsigned long long sub_doubles;   // a multiple of 16: slots start on 128-byte lines
    size_t item_cap, item_best;       // entries of the work-item list (item -> unit); the arg-max records begin item_best ints in
    int item_region;           // the list is TQ regions of this many: room for the units of one queue at their most items
    size_t kde_pdf_bytes;      // the kde buffer: [n_units][GRID_SPAN] doubles, then an outcome (int32) per unit
    size_t pool_bytes, desc_bytes, items_bytes, counter_bytes, kde_bytes;   // the five buffers
};
inline GridPlan plan_grid(int n_units, int hist_stride, int max_insert, int max_target, size_t pool_limit_bytes) {
    GridPlan p;
    p.n_units = n_units; p.max_target = max_target;
    // every axis is a subset of {distinct sizes} U {max_partial} plus at most maxinsert arithmetic entries
    p.cap = std::min(std::max(hist_stride + 1 + std::max(max_insert, 0), 8), GRID_MAX_ROWS);
    p.slot_doubles = grid_slot_doubles_max(p.cap, p.cap, max_target);
    p.slot_room = (p.slot_doubles + 16) * sizeof(double);
    const size_t per_queue = ((size_t)n_units + TQ - 1) / TQ;   // units of the fullest residue class mod TQ
    p.all_bytes = TQ * per_queue * p.slot_room;
    p.pool_bytes = std::max(std::min(p.all_bytes, pool_limit_bytes), p.slot_room);
    p.may_defer = p.all_bytes > p.pool_bytes; p.pool_doubles = p.pool_bytes / sizeof(double);
    // (a unit is never too big for its sub-pool, so every pass settles at least one unit per sub-pool)
    for (p.n_sub = TQ; p.n_sub > 1 && p.pool_doubles / p.n_sub < p.slot_doubles + 16;) p.n_sub >>= 1;
    p.sub_doubles = (p.pool_doubles / p.n_sub) & ~(unsigned long long)15;
    p.item_region = (int)(per_queue * unit_items(p.cap, p.cap));   // (unit_items grows with both arguments)
    p.item_cap = (size_t)TQ * p.item_region; p.item_best = (p.item_cap + 3) & ~(size_t)3;
    p.kde_pdf_bytes = (size_t)n_units * GRID_SPAN * sizeof(double); p.kde_bytes = p.kde_pdf_bytes + (size_t)n_units * sizeof(int32_t);
    p.desc_bytes = (size_t)n_units * GRID_DESC_BYTES; p.items_bytes = p.item_cap * GRID_ITEM_BYTES + 64; p.counter_bytes = GRID_COUNTER_BYTES;
    return p;
}

}  // namespace tredgpu
