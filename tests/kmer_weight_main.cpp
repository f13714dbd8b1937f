// Stand-alone driver of tredparse_amd/csrc/kmer_host.h for tests/test_kmer_weight_host.py (built with ASan + UBSan).
// usage: kmer_weight_main (prefix repeat suffix max_units)...
// Per ladder: "flag F", then per strand "bits <the 4096 presence bits, 6-mer 0 first>" and "cls <one hex digit per 6-mer>"
// ("cls -" when the builder left no class table).  The strands are those of tredgpu_set_ladders: prefix / repeat / suffix
// and rc(suffix) / rc(repeat) / rc(prefix).
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../tredparse_amd/csrc/kmer_host.h"
#include "../tredparse_amd/csrc/ladder_host.h"

int main(int argc, char** argv) {
    for (int a = 1; a + 3 < argc; a += 4) {
        const ladder_host::Codes P = ladder_host::encode(argv[a]), R = ladder_host::encode(argv[a + 1]), S = ladder_host::encode(argv[a + 2]);
        const int mu = atoi(argv[a + 3]);
        const ladder_host::Codes A[2] = {P, ladder_host::revcomp(S)}, Rep[2] = {R, ladder_host::revcomp(R)}, B[2] = {S, ladder_host::revcomp(P)};
        std::string text;
        int flag = 0;
        for (int s = 0; s < 2; ++s) {
            std::vector<uint32_t> bits, cls;
            const bool with_n = kmer_host::build_tables(A[s], Rep[s], B[s], mu, bits, cls);
            if (bits.size() != (size_t)kmer_host::BITS_WORDS || (with_n ? cls.size() != (size_t)kmer_host::CLS_WORDS : !cls.empty())) {
                fprintf(stderr, "table sizes %zu %zu\n", bits.size(), cls.size());
                return 2;
            }
            flag |= (with_n ? 1 : 0) << s;
            text += "bits ";
            for (int w = 0; w < 4096; ++w) text += (bits[w >> 5] >> (w & 31)) & 1u ? '1' : '0';
            text += "\ncls ";
            if (cls.empty()) text += "-";
            else for (int w = 0; w < 4096; ++w) text += "0123456789abcdef"[(cls[w >> 3] >> (4 * (w & 7))) & 15u];
            text += "\n";
        }
        printf("flag %d\n%s", flag, text.c_str());
    }
    return 0;
}
