// Stand-alone driver of tredparse_amd/csrc/cigar_long_plan.h for tests/test_cigar_long_plan.py, built with the address and
// undefined-behaviour sanitizers.  Records on the command line, one line of output each:
//   R rb re qb qe              rect_bytes of the fields {0, rb, re, qb, qe}
//   P k rb re qb qe [...]      plan() over k copies of each group of fields, groups in order: "slot_bytes slots total"
//   O n slots                  "slot:turn" of items 0 .. n-1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tredparse_amd/csrc/cigar_long_plan.h"

int main(int argc, char** argv) {
    using namespace cigar_long_plan;
    int i = 1;
    auto num = [&]() { return i < argc ? atol(argv[i++]) : 0L; };
    while (i < argc) {
        const char kind = argv[i++][0];
        if (kind == 'R') {
            int16_t f[5] = {0};
            for (int k = 1; k < 5; ++k) f[k] = (int16_t)num();
            printf("%zu\n", rect_bytes(f));
        } else if (kind == 'P') {
            std::vector<int16_t> fields;      // exactly n * 5 values: a read past them is the sanitizer's to report
            while (i < argc && (argv[i][0] == '-' || (argv[i][0] >= '0' && argv[i][0] <= '9'))) {
                const long k = num();
                int16_t f[5] = {0};
                for (int m = 1; m < 5; ++m) f[m] = (int16_t)num();
                for (long c = 0; c < k; ++c) fields.insert(fields.end(), f, f + 5);
            }
            const Plan p = plan(fields.data(), (int64_t)(fields.size() / 5));
            printf("%zu %d %zu\n", p.slot_bytes, p.slots, p.total());
        } else if (kind == 'O') {
            const long n = num();
            const int slots = (int)num();
            for (long k = 0; k < n; ++k) printf("%s%d:%lld", k ? " " : "", slot_of(k, slots), (long long)turn_of(k, slots));
            printf("\n");
        } else {
            fprintf(stderr, "unknown record %c\n", kind);
            return 2;
        }
    }
    return 0;
}
