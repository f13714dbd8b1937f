// Stand-alone driver of the tail counts in tredparse_amd/csrc/kmer_host.h (tail_entry, tail_count, tail_pack) for
// tests/test_sw_tail_host.py (built with ASan + UBSan).
// usage: sw_tail_main prefix repeat suffix max_units R  < lines
// A line of read letters (ACGTN; an empty line is a read of length 0): per strand one output line "s c0 c1 ... c15", the
// read's tail counts for R rows per lane.  The per-word masks are made as read_class_kernel makes them: bit j of word w =
// the window that ENDS at base 16 w + j lies in the read and is present in the strand's bitmap or holds an N.
// A line "=m0 m1 ..." (hex): the masks of the words themselves, for counts no read can reach; one output line "= c0 ... c15".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../tredparse_amd/csrc/kmer_host.h"
#include "../tredparse_amd/csrc/ladder_host.h"

static void emit(const char* head, const std::vector<uint32_t>& masks, int R) {
    std::vector<uint32_t> entries(masks.size());
    int total = 0;
    for (size_t w = 0; w < masks.size(); ++w) {
        entries[w] = kmer_host::tail_entry(masks[w], total);
        total += __builtin_popcount(masks[w] & 0xffffu);
    }
    uint32_t out[4];
    kmer_host::tail_pack(entries.data(), 1, (int)entries.size(), total, R, out);
    printf("%s", head);
    for (int l = 0; l < kmer_host::TAIL_LANES; ++l) printf(" %u", (out[l >> 2] >> (8 * (l & 3))) & 0xffu);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: sw_tail_main prefix repeat suffix max_units R\n"); return 2; }
    const ladder_host::Codes P = ladder_host::encode(argv[1]), Rp = ladder_host::encode(argv[2]), S = ladder_host::encode(argv[3]);
    const int mu = atoi(argv[4]), R = atoi(argv[5]);
    const ladder_host::Codes A[2] = {P, ladder_host::revcomp(S)}, Rep[2] = {Rp, ladder_host::revcomp(Rp)}, B[2] = {S, ladder_host::revcomp(P)};
    std::vector<uint32_t> bits[2], cls;
    for (int s = 0; s < 2; ++s) kmer_host::build_tables(A[s], Rep[s], B[s], mu, bits[s], cls);
    std::string line;
    while (std::getline(std::cin, line)) {
        if (!line.empty() && line[0] == '=') {
            std::istringstream in(line.substr(1));
            std::vector<uint32_t> masks;
            std::string tok;
            while (in >> tok) masks.push_back((uint32_t)strtoul(tok.c_str(), nullptr, 16));
            emit("=", masks, R);
            continue;
        }
        const ladder_host::Codes rd = ladder_host::encode(line.c_str());
        const int L = (int)rd.size();
        for (int s = 0; s < 2; ++s) {
            std::vector<uint32_t> masks((size_t)(L + 15) >> 4, 0u);
            for (int j = 5; j < L; ++j) {
                uint32_t idx = 0;
                bool has_n = false;
                for (int k = 0; k < 6; ++k) {
                    const int c = rd[(size_t)(j - 5 + k)];
                    has_n = has_n || c > 3;
                    idx |= (uint32_t)(c & 3) << (2 * k);
                }
                if (has_n || ((bits[s][idx >> 5] >> (idx & 31)) & 1u)) masks[(size_t)j >> 4] |= 1u << (j & 15);
            }
            emit(s ? "1" : "0", masks, R);
        }
    }
    return 0;
}
