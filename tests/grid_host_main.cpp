// Stand-alone driver of tredparse_amd/csrc/grid_host.h for tests/test_grid_host.py, built with the address and
// undefined-behaviour sanitizers (plain g++: the header is free of HIP).  Records on the command line, one line of output each:
//   K                                                  the constants: MAXOBS MAXM TQ CB RG RS TC GRID_MAX_ROWS GRID_DMAX and the
//                                                      doubles an Obs takes, then the bytes of a desc / an item / the counters
//   L nrow ncol nt run_pe haploid dmax n_near          unit_layout: "obs rowoff far1 far2 near1 near2 rept roll1 roll2 ml total"
//   M rows_cap cols_cap nt_max                         grid_slot_doubles_max
//   I nrow ncol                                        unit_items
//   P n_units hist_stride max_insert max_target pool_limit_bytes
//                                                      plan_grid: "cap slot_doubles slot_room all_bytes pool_bytes may_defer
//                                                      pool_doubles n_sub sub_doubles item_cap item_region item_best |
//                                                      pool descs items counters kde kde_pdf" (the last six in bytes)
#include <cstdio>
#include <cstdlib>

#include "../tredparse_amd/csrc/grid_host.h"

int main(int argc, char** argv) {
    using namespace tredgpu;
    int i = 1;
    auto num = [&]() { return i < argc ? atoll(argv[i++]) : 0LL; };
    while (i < argc) {
        const char kind = argv[i++][0];
        if (kind == 'K') {
            printf("%d %d %d %d %d %d %d %d %d %zu %zu %zu %zu\n", MAXOBS, MAXM, TQ, CB, RG, RS, TC, GRID_MAX_ROWS, GRID_DMAX, (sizeof(Obs) + 7) / 8,
                   GRID_DESC_BYTES, GRID_ITEM_BYTES, GRID_COUNTER_BYTES);
        } else if (kind == 'L') {
            const int nrow = (int)num(), ncol = (int)num(), nt = (int)num();
            const bool run_pe = num() != 0, haploid = num() != 0;
            const int dmax = (int)num(), n_near = (int)num();
            const SlotLayout L = unit_layout(nrow, ncol, nt, run_pe, haploid, dmax, n_near);
            printf("%d %d %d %d %d %d %d %d %d %d %d\n", L.obs, L.rowoff, L.far1, L.far2, L.near1, L.near2, L.rept, L.roll1, L.roll2, L.ml, L.total);
        } else if (kind == 'M') {
            const int rows = (int)num(), cols = (int)num(), nt = (int)num();
            printf("%zu\n", grid_slot_doubles_max(rows, cols, nt));
        } else if (kind == 'I') {
            const int nrow = (int)num(), ncol = (int)num();
            printf("%d\n", unit_items(nrow, ncol));
        } else if (kind == 'P') {
            const int n_units = (int)num(), hist_stride = (int)num(), max_insert = (int)num(), max_target = (int)num();
            const size_t limit = (size_t)num();
            const GridPlan p = plan_grid(n_units, hist_stride, max_insert, max_target, limit);
            printf("%d %zu %zu %zu %zu %d %zu %d %llu %zu %d %zu | %zu %zu %zu %zu %zu %zu\n", p.cap, p.slot_doubles, p.slot_room, p.all_bytes,
                   p.pool_bytes, (int)p.may_defer, p.pool_doubles, p.n_sub, p.sub_doubles, p.item_cap, p.item_region, p.item_best, p.pool_bytes,
                   p.desc_bytes, p.items_bytes, p.counter_bytes, p.kde_bytes, p.kde_pdf_bytes);
        } else {
            fprintf(stderr, "unknown record %c\n", kind);
            return 2;
        }
    }
    return 0;
}
