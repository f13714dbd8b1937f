// ladder_host.h -- the HIP-free half of what the five opt-in units (sw_long.hip, sw_cigar.hip, sw_cigar_long.hip,
// sw_second.hip, pileup.hip) share; side_unit.h, which includes it, is the half that needs HIP.  Base codes, the strand
// templates of a ladder, the error-text helper and the scoring-range check; the key of a ladder table and its packing
// into records and a letter pool; the argument checks of the entry points; the stable counting sort of a call's items
// into buckets.  Plain C++17 (tests/ladder_host_main.cpp runs it under ASan).
//
// capi.hip keeps its own copy of these functions (base_code / encode / revcomp and the construction in
// tredgpu_set_ladders) on purpose: it belongs to the sources whose hash the records under profiles/ carry (SRC_HASH in
// the Makefile), so it cannot change without a new profiling round.  This header is outside that hash.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
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

// ---- the ladder table and the argument checks ------------------------------------------------------------------------------

// a ladder table as the entry points take it
struct Table { int32_t n; const char* const *prefix, *const *repeat, *const *suffix; const int32_t* max_units; };

// one ladder of a packed table: strand s has its trunk at letters[trunk_off[s]] and its branch at letters[branch_off[s]]
struct LadderRecord {
    int32_t alen[2], blen[2];
    int32_t trunk_off[2], branch_off[2];   // byte offsets into the letter pool (one code 0..4 per byte)
    int32_t period, max_units;
};

// the text two tables share only when they are the same table; refuses a NULL sequence
inline int ladder_key(std::string& err, const Table& t, std::string& key) {
    key.clear();
    for (int i = 0; i < t.n; ++i) {
        if (!t.prefix[i] || !t.repeat[i] || !t.suffix[i]) return fail(err, -2, "ladder %d: NULL sequence", i);
        key += t.prefix[i]; key += '|'; key += t.repeat[i]; key += '|'; key += t.suffix[i]; key += '|';
        key += std::to_string(t.max_units[i]); key += ';';
    }
    return 0;
}

// the table as records and one pool of letters: per ladder and strand the trunk, then the branch, and 16 bytes of N behind
// the last.  max_template: the longest template a ladder may have (0: the items are checked on the device instead).
// plain_limits: a plain reference (max_units == 0) must have 1 .. max_template letters and is refused in words of its own
inline int pack_ladders(std::string& err, const Table& t, int max_template, std::vector<LadderRecord>& lad, Codes& pool,
                        bool plain_limits = false) {
    lad.assign((size_t)t.n, LadderRecord());
    pool.clear();
    auto append = [&pool](const Codes& v) {
        const int off = (int)pool.size();
        pool.insert(pool.end(), v.begin(), v.end());
        return off;
    };
    Strands S;
    for (int i = 0; i < t.n; ++i) {
        LadderRecord& d = lad[i];
        if (const char* why = build_strands(t.prefix[i], t.repeat[i], t.suffix[i], t.max_units[i], S))
            return fail(err, -2, "ladder %d: %s", i, why);
        const size_t T = (size_t)S.alen[0] + S.blen[0] + (size_t)S.period * S.max_units;
        if (plain_limits && S.max_units == 0 && (T < 1 || T > (size_t)max_template))
            return fail(err, -2, "ladder %d: reference length %zu not in [1,%d]", i, T, max_template);
        if (max_template > 0 && T > (size_t)max_template)
            return fail(err, -2, "ladder %d: longest template %zu exceeds TREDGPU_MAX_LONG_TEMPLATE_LEN=%d", i, T, max_template);
        d.period = S.period; d.max_units = S.max_units;
        for (int k = 0; k < S.n_strands; ++k) {
            d.alen[k] = S.alen[k];
            d.blen[k] = S.blen[k];
            d.trunk_off[k] = append(S.trunk[k]);
            d.branch_off[k] = append(S.branch[k]);
        }
    }
    pool.resize(pool.size() + 16, 4);
    return 0;
}

// what an entry point refuses before it reads an array.  mem_ok: the unit's own check of its memory switch; arrays: the
// nine of the items, looked at only when there are items
inline int call_refusal(std::string& err, const void* ctx, bool mem_ok, const Table& t, int64_t n_items, int32_t cap,
                        const tredgpu_sw_params* p, std::initializer_list<const void*> arrays) {
    if (!ctx) return fail(err, -2, "ctx is NULL");
    if (!mem_ok) return fail(err, -2, "mem must be TREDGPU_MEM_HOST or TREDGPU_MEM_DEVICE");
    if (n_items < 0 || n_items > 0x7fffffff || t.n <= 0 || cap <= 0) return fail(err, -2, "n_items, n_ladders and cap must be positive");
    if (!t.prefix || !t.repeat || !t.suffix || !t.max_units) return fail(err, -2, "NULL ladder argument");
    if (!p) return fail(err, -2, "params is NULL");
    if (const char* why = scoring_refusal(*p, false)) return fail(err, -2, "%s", why);
    for (const void* a : arrays)
        if (n_items > 0 && !a) return fail(err, -2, "NULL array argument");
    return 0;
}

// host memory: packed[0 .. read_off[n]) is what a call copies to the device.  With max_read >= 0 the words of every read
// the kernel accepts (0 <= L <= max_read) must be among them, since it reads them
inline int reads_refusal(std::string& err, const int64_t* read_off, const int32_t* read_len, size_t n, int max_read) {
    if (read_off[0] < 0 || read_off[n] < read_off[0]) return fail(err, -2, "read_off must be monotone");
    for (size_t k = 0; k < n && max_read >= 0; ++k) {
        const int L = read_len[k];
        if (L < 0 || L > max_read) continue;
        if (read_off[k] < 0 || read_off[k] + ((L + 15) >> 4) + ((L + 31) >> 5) > read_off[n])
            return fail(err, -2, "item %zu: its read does not lie inside packed[0 .. read_off[n_items])", k);
    }
    return 0;
}

// The stable counting sort of n items into n_buckets buckets: key(k) is item k's bucket, or negative for an item that is
// in none.  order: the items bucket after bucket, in the caller's order within one; off: the n_buckets + 1 offsets into it.
template <class Key>
void bucket_order(size_t n, size_t n_buckets, Key key, std::vector<int32_t>& order, std::vector<int64_t>& off) {
    off.assign(n_buckets + 1, 0);
    for (size_t k = 0; k < n; ++k)
        if (key(k) >= 0) off[(size_t)key(k) + 1] += 1;
    for (size_t b = 0; b < n_buckets; ++b) off[b + 1] += off[b];
    order.resize((size_t)off[n_buckets]);
    std::vector<int64_t> fill(off.begin(), off.end() - 1);
    for (size_t k = 0; k < n; ++k)
        if (key(k) >= 0) order[(size_t)fill[(size_t)key(k)]++] = (int32_t)k;
}

}  // namespace ladder_host
