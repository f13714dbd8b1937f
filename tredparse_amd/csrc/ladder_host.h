// ladder_host.h -- the host code the two opt-in units (sw_long.hip, sw_cigar.hip) share: base codes, the strand templates
// of a ladder, the error-text helper and the scoring-range check.  Plain C++17, nothing from HIP.
//
// capi.hip keeps its own copy of these functions (base_code / encode / revcomp and the construction in
// tredgpu_set_ladders) on purpose: it belongs to the sources whose hash the records under profiles/ carry (SRC_HASH in
// the Makefile), so it cannot change without a new profiling round.  This header is outside that hash.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/tredgpu.h"

namespace ladder_host {

using Codes = std::vector<uint8_t>;   // one base code per letter: A C G T = 0..3, anything else 4 (N)

inline int base_code(char ch) {
    switch (ch) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}

inline Codes encode(const char* s) {
    Codes o;
    for (; *s; ++s) o.push_back((uint8_t)base_code(*s));
    return o;
}

// reverse complement on codes (N stays N): bam_parser.py:448-450
inline Codes revcomp(const Codes& v) {
    Codes o(v.size());
    for (size_t i = 0; i < v.size(); ++i) {
        const int c = v[v.size() - 1 - i];
        o[i] = (uint8_t)(c == 4 ? 4 : 3 - c);
    }
    return o;
}

// The templates of one ladder, per strand: template u (1..max_units) of strand s is trunk[s][0 .. alen[s] + period * u)
// followed by branch[s].  max_units == 0 is a plain reference: one strand, trunk = prefix, no branch.
struct Strands {
    int n_strands = 0, period = 0, max_units = 0;   // period = |repeat|, for a plain reference too
    int alen[2] = {0, 0}, blen[2] = {0, 0};
    Codes trunk[2], branch[2];
};

// The layout of tredgpu_set_ladders: trunk = prefix + repeat * max_units / rc(suffix) + rc(repeat) * max_units,
// branch = suffix / rc(prefix).  Returns null, or why the ladder is refused (the text after "ladder %d: ").
// Length limits are the caller's.
inline const char* build_strands(const char* prefix, const char* repeat, const char* suffix, int max_units, Strands& out) {
    out = Strands();
    if (max_units < 0) return "negative max_units";
    const Codes P = encode(prefix), R = encode(repeat), S = encode(suffix);
    out.period = (int)R.size();
    out.max_units = max_units;
    if (max_units == 0) {
        out.n_strands = 1;
        out.alen[0] = (int)P.size();
        out.trunk[0] = P;
        return nullptr;
    }
    if (R.empty()) return "empty repeat";
    const Codes A[2] = {P, revcomp(S)}, Rep[2] = {R, revcomp(R)}, B[2] = {S, revcomp(P)};
    out.n_strands = 2;
    for (int s = 0; s < 2; ++s) {
        out.alen[s] = (int)A[s].size();
        out.blen[s] = (int)B[s].size();
        out.trunk[s] = A[s];
        for (int u = 0; u < max_units; ++u) out.trunk[s].insert(out.trunk[s].end(), Rep[s].begin(), Rep[s].end());
        out.branch[s] = B[s];
    }
    return nullptr;
}

// formats the message into the caller's (thread_local) error string and returns the code
inline int fail(std::string& err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// null, or the message of a scoring the kernels do not take; with_flank: flank is checked (and named) as well
inline const char* scoring_refusal(const tredgpu_sw_params& p, bool with_flank) {
    const bool ok = p.match >= 1 && p.match <= 8 && p.mismatch >= 0 && p.mismatch <= 16 && p.gap_extend >= 1 &&
                    p.gap_extend <= p.gap_open && p.gap_open <= 16 && (!with_flank || (p.flank >= 0 && p.flank <= 255));
    if (ok) return nullptr;
    return with_flank ? "scoring out of the supported range (match 1..8, mismatch 0..16, "
                        "1 <= gap_extend <= gap_open <= 16, flank 0..255)"
                      : "scoring out of the supported range (match 1..8, mismatch 0..16, 1 <= gap_extend <= gap_open <= 16)";
}

}  // namespace ladder_host
