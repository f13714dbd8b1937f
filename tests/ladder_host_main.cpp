// Stand-alone driver of tredparse_amd/csrc/ladder_host.h for tests/test_ladder_host.py (built there with the address and
// undefined-behaviour sanitizers).  Arguments, any number of groups:
//   L PREFIX REPEAT SUFFIX MAX_UNITS              -> "strands N period P max_units M" and per strand "ALEN BLEN TRUNK BRANCH"
//                                                    (tab-separated, letters ACGTN), or "refused RC TEXT"
//   S MATCH MISMATCH GAP_OPEN GAP_EXTEND FLANK 0|1 -> "scoring ok" or "scoring TEXT" (last argument: the flank switch)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tredparse_amd/csrc/ladder_host.h"

static std::string letters(const ladder_host::Codes& v) {
    std::string s;
    for (uint8_t c : v) s += "ACGTN"[c];
    return s;
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
        } else {
            fprintf(stderr, "bad arguments at %d\n", k);
            return 2;
        }
    }
    return 0;
}
