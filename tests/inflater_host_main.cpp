// Stand-alone driver of tredparse_amd/csrc/inflater_host.h for tests/test_inflater_host.py, built with the address and
// undefined-behaviour sanitizers.  Records on the command line, one line of output each (every array is exactly as long as
// the record says: a read past it is the sanitizer's to report):
//   N need cap past_need past_cap                        next_cap
//   B cap_comp cap_out n coff[n + 1] ooff[n + 1]         check_blocks: its text, or "ok"
//   T n_blocks n_chunks k {chunk_first n_chunks block_first block_end} * k      check_tasks
//   C k begin_upos[k]                                    check_chunks
//   P n_blocks coff_step ooff_step k {chunk_first n_chunks block_first block_end} * k  q {begin_block end_coffset} * q
//                                                        plan_walk: "rec_base[0] .. rec_base[k] | total_recs large_table"
//   W gap n need[n] ooff[n + 1]                          wanted_runs and dense_offsets: "first-last ... | dense_off[0 .. n] | total"
//   L nb n_tasks n_chunks n_alt                          the layouts: "bclen xcrc bytes | chunks rec_base bytes | counters bytes |
//                                                        need bytes | results bytes"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tredparse_amd/csrc/inflater_host.h"

int main(int argc, char** argv) {
    using namespace inflater_host;
    int i = 1;
    auto num = [&]() { return i < argc ? atoll(argv[i++]) : 0LL; };
    auto say = [](const char* bad) { printf("%s\n", bad ? bad : "ok"); };
    auto read_tasks = [&](size_t k) {
        std::vector<tredgpu_walk_task> t(k);
        for (tredgpu_walk_task& T : t) {
            T = tredgpu_walk_task{};
            T.chunk_first = (int32_t)num(); T.n_chunks = (int32_t)num(); T.block_first = (int32_t)num(); T.block_end = (int32_t)num();
        }
        return t;
    };
    while (i < argc) {
        const char kind = argv[i++][0];
        if (kind == 'N') {
            const size_t need = (size_t)num(), cap = (size_t)num(), pn = (size_t)num(), pc = (size_t)num();
            printf("%zu\n", next_cap(need, cap, pn, pc));
        } else if (kind == 'B') {
            const size_t cap_comp = (size_t)num(), cap_out = (size_t)num();
            const int32_t n = (int32_t)num();
            std::vector<int64_t> coff((size_t)n + 1), ooff((size_t)n + 1);
            for (int64_t& v : coff) v = num();
            for (int64_t& v : ooff) v = num();
            say(check_blocks(coff.data(), ooff.data(), n, cap_comp, cap_out));
        } else if (kind == 'T') {
            const int32_t n_blocks = (int32_t)num();
            const size_t n_chunks = (size_t)num(), k = (size_t)num();
            const std::vector<tredgpu_walk_task> t = read_tasks(k);
            say(check_tasks(t.data(), k, n_chunks, n_blocks));
        } else if (kind == 'C') {
            std::vector<tredgpu_walk_chunk> c((size_t)num());
            for (tredgpu_walk_chunk& ch : c) ch = tredgpu_walk_chunk{0, (int32_t)num(), 0};
            say(check_chunks(c.data(), c.size()));
        } else if (kind == 'P') {
            const size_t nb = (size_t)num();
            const int64_t cstep = num(), ostep = num();
            std::vector<int64_t> bcoff(nb), ooff(nb + 1);
            for (size_t k = 0; k < nb; ++k) bcoff[k] = cstep * (int64_t)k;
            for (size_t k = 0; k <= nb; ++k) ooff[k] = ostep * (int64_t)k;
            const size_t k = (size_t)num();
            const std::vector<tredgpu_walk_task> t = read_tasks(k);
            std::vector<tredgpu_walk_chunk> c((size_t)num());
            for (tredgpu_walk_chunk& ch : c) { ch.begin_block = (int32_t)num(); ch.begin_upos = 0; ch.end_voffset = ((uint64_t)num() << 16) | 500; }
            std::vector<int64_t> rec_base(k + 1, -1);
            const WalkPlan p = plan_walk(t.data(), k, c.data(), bcoff.data(), ooff.data(), rec_base.data());
            for (int64_t v : rec_base) printf("%lld ", (long long)v);
            printf("| %zu %d\n", p.total_recs, (int)p.large_table);
        } else if (kind == 'W') {
            const int64_t gap = num();
            const int32_t n = (int32_t)num();
            std::vector<uint8_t> need((size_t)n);
            std::vector<int64_t> ooff((size_t)n + 1), dense((size_t)n + 1, -1);
            for (uint8_t& v : need) v = (uint8_t)num();
            for (int64_t& v : ooff) v = num();
            const std::vector<Run> runs = wanted_runs(need.data(), ooff.data(), n, gap);
            const int64_t total = dense_offsets(runs, ooff.data(), n, dense.data());
            for (const Run& r : runs) printf("%d-%d ", r.first, r.last);
            printf("|");
            for (int64_t v : dense) printf(" %lld", (long long)v);
            printf(" | %lld\n", (long long)total);
        } else if (kind == 'L') {
            const size_t nb = (size_t)num(), n_tasks = (size_t)num(), n_chunks = (size_t)num(), n_alt = (size_t)num();
            const BlockTable b{nb};
            const TaskTable t{n_tasks, n_chunks};
            const ResultTable r{n_tasks};
            const AltResultTable a{n_alt, nb};
            const SelectTable s{n_tasks};
            printf("%zu %zu %zu | %zu %zu %zu | %zu %zu | %zu %zu | %zu %zu\n", b.bclen(), b.xcrc(), b.bytes(), t.chunks(), t.rec_base(), t.bytes(),
                   r.counters(), r.bytes(), a.need(), a.bytes(), s.results(), s.bytes());
        } else {
            fprintf(stderr, "unknown record %c\n", kind);
            return 2;
        }
    }
    return 0;
}
