// kmer_host.h -- the 6-mer tables of one ladder strand, built on the host (tredgpu_set_ladders) for the exact strand
// filter of sw_cont_kernel / read_class_kernel, and the arithmetic of the per-lane tail counts (below; host and device).
// Plain C++17, no HIP needed (tests/kmer_weight_main.cpp and tests/sw_tail_main.cpp run it under ASan).
//
// Templates of a strand: head + repeat * u + branch, u = 1 .. max_units, as base codes 0..3 and 4 = N.  A template N
// scores 0 against every base, so it neither breaks nor feeds a run of matches: a template window with N positions
// stands for all its fillings.
//   bits   4096-bit presence map (128 words): 6-mer w (2 bits per base, first base in the low bits) occurs in some
//          template window of the strand, under some filling
//   cls    only for a strand whose templates hold an N: 4 bits per 6-mer (512 words, entry w in bits 4 * (w & 7) of
//          word w >> 3) = j(w), the fewest N positions of any template window that produces w; 0 for an absent 6-mer.
//          A run of matches through k read windows crosses at least ceil(sum j / 6) template N columns (every column
//          lies in at most six of the windows), each worth 0 instead of a match: see DESIGN.md 4.1.
#pragma once
#include <cstdint>
#include <vector>

namespace kmer_host {

constexpr int BITS_WORDS = 128;
constexpr int CLS_WORDS = 512;

template <class Vec>
inline bool holds_n(const Vec& v) {
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i] > 3) return true;
    return false;
}

// Returns whether some template of the strand holds an N; cls is left empty when none does.
template <class Vec>
inline bool build_tables(const Vec& head, const Vec& repeat, const Vec& branch, int max_units, std::vector<uint32_t>& bits,
                         std::vector<uint32_t>& cls) {
    bits.assign(BITS_WORDS, 0u);
    cls.clear();
    const bool with_n = max_units > 0 && (holds_n(head) || holds_n(repeat) || holds_n(branch));
    std::vector<uint8_t> fewest(4096, 15);          // 15: absent
    std::vector<bool> seen((size_t)1 << 18, false);  // window = 12 bits of codes | 6 bits of N positions: expanded once
    Vec t;
    for (int u = 1; u <= max_units; ++u) {
        t.assign(head.begin(), head.end());
        for (int k = 0; k < u; ++k) t.insert(t.end(), repeat.begin(), repeat.end());
        t.insert(t.end(), branch.begin(), branch.end());
        for (size_t i = 0; i + 6 <= t.size(); ++i) {
            uint32_t code = 0, mask = 0;
            int wild[6], nw = 0;
            for (int k = 0; k < 6; ++k) {
                if (t[i + k] > 3) { wild[nw++] = k; mask |= 1u << k; }
                else code |= (uint32_t)(t[i + k] & 3) << (2 * k);
            }
            const uint32_t key = code | mask << 12;
            if (seen[key]) continue;
            seen[key] = true;
            for (uint32_t f = 0; f < (1u << (2 * nw)); ++f) {
                uint32_t cf = code;
                for (int j = 0; j < nw; ++j) cf |= ((f >> (2 * j)) & 3u) << (2 * wild[j]);
                bits[cf >> 5] |= 1u << (cf & 31);
                if (nw < fewest[cf]) fewest[cf] = (uint8_t)nw;
            }
        }
    }
    if (with_n) {
        cls.assign(CLS_WORDS, 0u);
        for (uint32_t w = 0; w < 4096; ++w)
            if (fewest[w] != 15) cls[w >> 3] |= (uint32_t)fewest[w] << (4 * (w & 7));
    }
    return with_n;
}

// ---- per-lane tail counts (read_class_kernel -> SwArgs::read_tail -> the second tier of sw_cont_kernel's bounded-gain exit)
// Wtail[lane] = the read's 6-mer windows that start at or after row lane * R and are present in the strand's templates (a
// window with a read N counts as present), R = rows per lane; one byte per lane, saturated at TAIL_SAT; TAIL_NONE = no bound.
// read_class_kernel's count loop has, per 16-base word of the read, the mask of the present windows by END position (a
// window that starts at row w ends at w + 5); it leaves one entry per word, and the 16 counts are taken from the entries
// once the loop is over.  Host and device: the same function is checked by tests/sw_tail_main.cpp under ASan.
#if defined(__HIPCC__)
#define KMER_HD __host__ __device__
#else
#define KMER_HD
#endif
constexpr int TAIL_LANES = 16;
constexpr int TAIL_SAT = 254;
constexpr int TAIL_NONE = 255;

// One word's entry: the mask of its 16 end positions | the windows counted in the words before it << 16.
KMER_HD inline uint32_t tail_entry(uint32_t end_mask, int before) { return (end_mask & 0xffffu) | (uint32_t)before << 16; }

// entries[w * stride], w = 0 .. nb - 1; total = the windows counted in all words.  The lane's count = total - the windows
// that end before position lane * R + 5.
KMER_HD inline int tail_count(const uint32_t* entries, int stride, int nb, int total, int R, int lane) {
    const int e = lane * R + 5;
    const int w = e >> 4;
    if (w >= nb) return 0;
    const uint32_t en = entries[w * stride];
    const int t = total - (int)(en >> 16) - __builtin_popcount(en & ((1u << (e & 15)) - 1u));
    return t > TAIL_SAT ? TAIL_SAT : t;
}

// The 16 bytes of one read and strand, lane 0 in the low byte of out[0].
KMER_HD inline void tail_pack(const uint32_t* entries, int stride, int nb, int total, int R, uint32_t out[4]) {
    for (int k = 0; k < 4; ++k) {
        uint32_t v = 0;
        for (int b = 0; b < 4; ++b) v |= (uint32_t)tail_count(entries, stride, nb, total, R, 4 * k + b) << (8 * b);
        out[k] = v;
    }
}

}  // namespace kmer_host
