// Stand-alone driver of libtredbam's plan / scan family (tredparse_amd/csrc/bamread.cpp, include/tredbam.h) for the
// sanitizers: tests/test_bam_plan.py compiles it with bamread.cpp and emit.cpp under -fsanitize=address,undefined and runs
//   bam_plan_main FILE.bam contig:start:end[@contig:start:end ...] ... [+contig:start:end ...]
// one argument per locus (the '@' parts: its alternative regions), '+' arguments: extra regions.  It opens the file, plans
// with an unknown contig among the sites and with no sites at all, calls every walk planner before any plan, without room
// and with room, lists and fills the plan, inflates the blocks with zlib, preloads them, scans, hands tredbam_scan_pe a
// slice outside the declared pools, and closes.  Every step prints one line; a step that does not answer as include/tredbam.h
// says ends the program with status 1.
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tredbam.h"

static void check(bool ok, const char* what) {
    if (ok) return;
    fprintf(stderr, "failed: %s\n", what);
    exit(1);
}

static tredbam_region region(tredbam* b, const std::string& s) {      // contig:start:end
    const size_t c1 = s.find(':'), c2 = s.find(':', c1 + 1);
    check(c1 != std::string::npos && c2 != std::string::npos, "a region is contig:start:end");
    return {tredbam_tid(b, s.substr(0, c1).c_str()), atoi(s.c_str() + c1 + 1), atoi(s.c_str() + c2 + 1)};
}

int main(int argc, char** argv) {
    check(argc >= 3, "usage: bam_plan_main FILE.bam contig:start:end[@contig:start:end ...] ... [+contig:start:end ...]");
    tredbam* b = nullptr;
    check(tredbam_open(argv[1], &b) == 0 && b, "open");
    std::vector<tredbam_site> sites;
    std::vector<tredbam_region> alts, extra;
    for (int k = 2; k < argc; ++k) {
        std::string a = argv[k];
        if (a[0] == '+') { extra.push_back(region(b, a.substr(1))); continue; }
        size_t at = a.find('@');
        const tredbam_region r = region(b, a.substr(0, at));
        tredbam_site st = {r.tid, r.start, r.end, (int32_t)alts.size(), 0};
        while (at != std::string::npos) {
            const size_t next = a.find('@', at + 1);
            alts.push_back(region(b, a.substr(at + 1, next == std::string::npos ? next : next - at - 1)));
            ++st.n_alt;
            at = next;
        }
        sites.push_back(st);
    }
    sites.push_back({-1, 1000, 1100, (int32_t)alts.size(), 0});         // a locus on a contig this file does not have
    alts.push_back({-1, 0, 0});                                        // (never empty: the arrays' addresses are handed in)
    extra.push_back({-1, 0, 100});
    const int32_t n_sites = (int32_t)sites.size(), n_alts = (int32_t)alts.size() - 1, n_extra = (int32_t)extra.size();
    const tredbam_scan_opts o = {150, 1000, 9, 10000, 1000, 1, 1, 1};

    std::vector<tredbam_walk_task> tasks((size_t)std::max(std::max(n_sites, n_alts), n_extra) + 1);
    std::vector<tredbam_walk_chunk> chunks(1 << 16);
    auto plan_walks = [&](int64_t cap) { return tredbam_plan_walks(b, sites.data(), n_sites, &o, tasks.data(), cap ? chunks.data() : nullptr, cap); };
    auto plan_alt_walks = [&](int64_t cap) {
        return tredbam_plan_alt_walks(b, sites.data(), n_sites, alts.data(), n_alts, &o, tasks.data(), cap ? chunks.data() : nullptr, cap);
    };
    auto plan_region_walks = [&](int64_t cap) {
        return tredbam_plan_region_walks(b, extra.data(), n_extra, tasks.data(), cap ? chunks.data() : nullptr, cap);
    };
    auto every_planner = [&](const char* when, bool planned) {
        const char* const names[3] = {"walks", "alt_walks", "region_walks"};
        for (int which = 0; which < 3; ++which) {
            auto call = [&](int64_t cap) { return which == 0 ? plan_walks(cap) : which == 1 ? plan_alt_walks(cap) : plan_region_walks(cap); };
            const int64_t n = call((int64_t)chunks.size());
            check(n >= 0, "a planner with room");
            int64_t held = 0;
            for (int64_t c = 0; c < n; ++c) held += chunks[(size_t)c].begin_block >= 0;
            check(planned || held == 0, "before any plan no chunk starts in a planned block");
            check(call(0) == (n > 0 ? -3 : 0), "a planner without room returns -3");
            check(call(n) == n && (n == 0 || call(n - 1) == -3), "-3 exactly when the chunks do not fit");
            printf("%s %s chunks %lld in_plan %lld\n", when, names[which], (long long)n, (long long)held);
        }
    };
    every_planner("unplanned", false);

    int64_t cb = -1, ob = -1;
    check(tredbam_plan(b, sites.data(), 0, alts.data(), &o, nullptr, 0, &cb, &ob) == 0 && cb == 0 && ob == 0, "a plan of no sites is empty");
    check(tredbam_plan_blocks(b, nullptr, nullptr, nullptr, nullptr) == 0, "an empty plan lists no blocks");
    const int64_t n = tredbam_plan(b, sites.data(), n_sites, alts.data(), &o, extra.data(), n_extra, &cb, &ob);
    check(n > 0 && cb > 0 && ob > 0, "plan");
    printf("plan %lld %lld %lld\n", (long long)n, (long long)cb, (long long)ob);
    every_planner("planned", true);

    std::vector<int64_t> coffset((size_t)n), comp_off((size_t)n + 1), out_off((size_t)n + 1);
    std::vector<int32_t> clen((size_t)n), status((size_t)n, 0);
    std::vector<uint32_t> crc((size_t)n);
    std::vector<uint8_t> host((size_t)n), comp((size_t)cb), out((size_t)ob);
    check(tredbam_plan_blocks(b, coffset.data(), clen.data(), crc.data(), host.data()) == n, "plan_blocks");
    check(tredbam_plan_fill(b, comp.data(), 0, 0, comp_off.data(), out_off.data()) == 0, "plan_fill");
    check(comp_off[(size_t)n] == cb && out_off[(size_t)n] == ob, "plan_fill ends where plan said");
    for (int64_t k = 0; k < n; ++k) {
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        check(inflateInit2(&zs, -15) == Z_OK, "inflateInit2");
        zs.next_in = comp.data() + comp_off[(size_t)k];
        zs.avail_in = (uInt)(comp_off[(size_t)k + 1] - comp_off[(size_t)k]);
        zs.next_out = out.data() + out_off[(size_t)k];
        zs.avail_out = (uInt)(out_off[(size_t)k + 1] - out_off[(size_t)k]);
        const int rc = inflate(&zs, Z_FINISH);
        inflateEnd(&zs);
        check(rc == Z_STREAM_END && zs.avail_out == 0, "a planned payload inflates to its planned size");
        check(tredbam_crc32(0, out.data() + out_off[(size_t)k], out_off[(size_t)k + 1] - out_off[(size_t)k]) == crc[(size_t)k], "a planned block's CRC");
    }
    check(tredbam_preload(b, out.data(), out_off.data(), status.data()) == n, "preload takes every block");

    std::vector<tredbam_unit> units((size_t)n_sites);
    tredbam_pools pools;
    check(tredbam_scan(b, sites.data(), n_sites, alts.data(), &o, units.data()) == 0 && tredbam_scan_pools(b, &pools) == 0, "scan");
    check(units.back().status == TREDBAM_UNIT_NO_FETCH && units.back().n_reads == 0, "the unknown contig gives no reads");
    int64_t reads = 0;
    for (const tredbam_unit& u : units) reads += u.n_reads;
    check(reads == pools.n_reads && pools.word_off[pools.n_reads] == pools.n_words, "the pools hold the units' reads");
    printf("scan reads %lld global %lld target %lld\n", (long long)pools.n_reads, (long long)pools.n_global, (long long)pools.n_target);

    // pair lengths from elsewhere: a slice of site 0 that lies outside the pools as declared
    std::vector<tredbam_walk_result> pe((size_t)n_sites);
    for (auto& r : pe) { memset(&r, 0, sizeof r); r.status = 1; }
    pe[0].status = 0;
    pe[0].n_global = 5;
    const int32_t pe_global[2] = {300, 310}, pe_target[1] = {0};
    check(tredbam_pe_pool_sizes(b, 2, 0) == 0, "pe_pool_sizes");
    check(tredbam_scan_pe(b, sites.data(), n_sites, alts.data(), &o, pe.data(), pe_global, pe_target, units.data()) == -2, "a slice outside the pools is refused");
    printf("scan_pe refused: %s\n", tredbam_last_error(b));
    pe[0].n_global = 2;
    check(tredbam_scan_pe(b, sites.data(), n_sites, alts.data(), &o, pe.data(), pe_global, pe_target, units.data()) == 0, "a slice inside them is taken");
    check(units[0].n_global == 2 && units[0].n_target == 0, "site 0 has the two lengths handed in");

    int64_t hits = -1, misses = -1;
    tredbam_preload_clear(b, &hits, &misses);
    check(hits > 0 && misses == 0, "every block load of the scans was served from the preloaded set");
    printf("preload hits %lld misses %lld\n", (long long)hits, (long long)misses);
    every_planner("cleared", false);                                   // (the plan went with the preloaded blocks)
    tredbam_close(b);
    printf("closed\n");
    return 0;
}
