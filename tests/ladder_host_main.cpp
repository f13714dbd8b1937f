// Stand-alone driver of tredparse_amd/csrc/ladder_host.h for tests/test_ladder_host.py (built there with the address and
// undefined-behaviour sanitizers).  Arguments, any number of groups:
//   L PREFIX REPEAT SUFFIX MAX_UNITS              -> "strands N period P max_units M" and per strand "ALEN BLEN TRUNK BRANCH"
//                                                    (tab-separated, letters ACGTN), or "refused RC TEXT"
//   S MATCH MISMATCH GAP_OPEN GAP_EXTEND FLANK 0|1 -> "scoring ok" or "scoring TEXT" (last argument: the flank switch)
// and of what the units' entry points take from it (a sequence given as NULL is a null pointer):
//   K N {PREFIX REPEAT SUFFIX MAX_UNITS} x N       -> "key TEXT", or "refused RC TEXT"
//   P MAX_TEMPLATE N {PREFIX REPEAT SUFFIX MAX_UNITS} x N
//                                                  -> "pool LETTERS" (the whole pool, padding included) and per ladder "PERIOD
//                                                     MAX_UNITS" and per strand "ALEN BLEN TRUNK_OFF BRANCH_OFF" (tab-separated;
//                                                     two strands always, as stored), or "refused RC TEXT"
//   Q MAX_TEMPLATE N {...} x N                     -> as P, with the limits of a plain reference on (1 .. MAX_TEMPLATE letters)
//   B N_BUCKETS N KEY x N                          -> "order ITEM ..." and "off OFFSET ..." of bucket_order (a negative key: the
//                                                     item is in no bucket)
//   C CTX MEM_OK N_ITEMS N_LADDERS CAP NULL_TABLE PARAMS NULL_ARRAY
//                                                  -> "call RC TEXT".  CTX, MEM_OK: 0|1; NULL_TABLE: which of prefix, repeat,
//                                                     suffix, max_units is null (1..4, 0 none); PARAMS: NULL or MATCH,MISMATCH,
//                                                     GAP_OPEN,GAP_EXTEND; NULL_ARRAY: which of the nine arrays is null (-1 none)
//   R MAX_READ N READ_OFF x (N + 1) READ_LEN x N   -> "reads RC TEXT"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tredparse_amd/csrc/ladder_host.h"

static std::string letters(const ladder_host::Codes& v) {
    std::string s;
    for (uint8_t c : v) s += "ACGTN"[c];
    return s;
}

static const char* seq(const char* s) { return strcmp(s, "NULL") ? s : nullptr; }

// the table of N ladders that begins at argv[k]; the arrays live in the caller's vectors
static ladder_host::Table table(char** argv, int k, int n, std::vector<const char*> (&cols)[3], std::vector<int32_t>& mu) {
    for (int i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) cols[c].push_back(seq(argv[k + 4 * i + c]));
        mu.push_back(atoi(argv[k + 4 * i + 3]));
    }
    return ladder_host::Table{n, cols[0].data(), cols[1].data(), cols[2].data(), mu.data()};
}

int main(int argc, char** argv) {
    int ladder = 0;
    for (int k = 1; k < argc;) {
        if (!strcmp(argv[k], "L") && k + 4 < argc) {
            ladder_host::Strands st;
            std::string err;
            const char* why = ladder_host::build_strands(argv[k + 1], argv[k + 2], argv[k + 3], atoi(argv[k + 4]), st);
            if (why) {
                const int rc = ladder_host::fail(err, -2, "ladder %d: %s", ladder, why);
                printf("refused %d %s\n", rc, err.c_str());
            } else {
                printf("strands %d period %d max_units %d\n", st.n_strands, st.period, st.max_units);
                for (int s = 0; s < st.n_strands; ++s)
                    printf("%d\t%d\t%s\t%s\n", st.alen[s], st.blen[s], letters(st.trunk[s]).c_str(), letters(st.branch[s]).c_str());
            }
            ++ladder;
            k += 5;
        } else if (!strcmp(argv[k], "S") && k + 6 < argc) {
            tredgpu_sw_params p;
            memset(&p, 0, sizeof p);
            p.match = atoi(argv[k + 1]);
            p.mismatch = atoi(argv[k + 2]);
            p.gap_open = atoi(argv[k + 3]);
            p.gap_extend = atoi(argv[k + 4]);
            p.flank = atoi(argv[k + 5]);
            const char* why = ladder_host::scoring_refusal(p, atoi(argv[k + 6]) != 0);
            printf("scoring %s\n", why ? why : "ok");
            k += 7;
        } else if ((!strcmp(argv[k], "K") && k + 1 < argc && k + 1 + 4 * atoi(argv[k + 1]) < argc) ||
                   ((!strcmp(argv[k], "P") || !strcmp(argv[k], "Q")) && k + 2 < argc && k + 2 + 4 * atoi(argv[k + 2]) < argc)) {
            const bool pack = argv[k][0] != 'K', plain_limits = argv[k][0] == 'Q';
            const int at = k + (pack ? 3 : 2), n = atoi(argv[at - 1]);
            std::vector<const char*> cols[3];
            std::vector<int32_t> mu;
            const ladder_host::Table t = table(argv, at, n, cols, mu);
            std::string err, key;
            std::vector<ladder_host::LadderRecord> lad;
            ladder_host::Codes pool;
            const int rc = pack ? ladder_host::pack_ladders(err, t, atoi(argv[k + 1]), lad, pool, plain_limits) : ladder_host::ladder_key(err, t, key);
            if (rc) printf("refused %d %s\n", rc, err.c_str());
            else if (!pack) printf("key %s\n", key.c_str());
            else {
                printf("pool %s\n", letters(pool).c_str());
                for (const ladder_host::LadderRecord& d : lad) {
                    printf("%d\t%d\n", d.period, d.max_units);
                    for (int s = 0; s < 2; ++s) printf("%d\t%d\t%d\t%d\n", d.alen[s], d.blen[s], d.trunk_off[s], d.branch_off[s]);
                }
            }
            k = at + 4 * n;
        } else if (!strcmp(argv[k], "B") && k + 2 < argc && k + 2 + atoi(argv[k + 2]) < argc) {
            const int n = atoi(argv[k + 2]);
            std::vector<long long> keys;               // exactly n entries: a read past them is the sanitizer's
            for (int i = 0; i < n; ++i) keys.push_back(atoll(argv[k + 3 + i]));
            std::vector<int32_t> order;
            std::vector<int64_t> off;
            ladder_host::bucket_order((size_t)n, (size_t)atoi(argv[k + 1]), [&](size_t i) { return keys[i]; }, order, off);
            printf("order");
            for (int32_t v : order) printf(" %d", v);
            printf("\noff");
            for (int64_t v : off) printf(" %lld", (long long)v);
            printf("\n");
            k += 3 + n;
        } else if (!strcmp(argv[k], "C") && k + 8 < argc) {
            const char* col[1] = {"A"};
            const int32_t mu[1] = {0};
            const int null_table = atoi(argv[k + 6]), null_array = atoi(argv[k + 8]);
            const ladder_host::Table t{atoi(argv[k + 4]), null_table == 1 ? nullptr : col, null_table == 2 ? nullptr : col,
                                       null_table == 3 ? nullptr : col, null_table == 4 ? nullptr : mu};
            tredgpu_sw_params p;
            memset(&p, 0, sizeof p);
            const bool have_p = sscanf(argv[k + 7], "%d,%d,%d,%d", &p.match, &p.mismatch, &p.gap_open, &p.gap_extend) == 4;
            const void* arr[9];
            for (int i = 0; i < 9; ++i) arr[i] = i == null_array ? nullptr : &p;
            std::string err;
            const int rc = ladder_host::call_refusal(err, atoi(argv[k + 1]) ? &p : nullptr, atoi(argv[k + 2]) != 0, t, atoll(argv[k + 3]),
                                                     atoi(argv[k + 5]), have_p ? &p : nullptr,
                                                     {arr[0], arr[1], arr[2], arr[3], arr[4], arr[5], arr[6], arr[7], arr[8]});
            printf("call %d %s\n", rc, err.c_str());
            k += 9;
        } else if (!strcmp(argv[k], "R") && k + 2 < argc && k + 3 + 2 * atoi(argv[k + 2]) < argc) {
            const int n = atoi(argv[k + 2]);
            std::vector<int64_t> off;                  // exactly n + 1 and n entries: a read past them is the sanitizer's
            std::vector<int32_t> len;
            for (int i = 0; i <= n; ++i) off.push_back(atoll(argv[k + 3 + i]));
            for (int i = 0; i < n; ++i) len.push_back(atoi(argv[k + 4 + n + i]));
            std::string err;
            const int rc = ladder_host::reads_refusal(err, off.data(), len.data(), (size_t)n, atoi(argv[k + 1]));
            printf("reads %d %s\n", rc, err.c_str());
            k += 4 + 2 * n;
        } else {
            fprintf(stderr, "bad arguments at %d\n", k);
            return 2;
        }
    }
    return 0;
}
