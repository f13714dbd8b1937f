// side_unit.h -- the harness of the five opt-in units outside the hashed sources (sw_long.hip, sw_cigar.hip,
// sw_cigar_long.hip, sw_second.hip, pileup.hip).  Device side: the fields every unit's argument block has for the ladder
// table and the scoring, the template of an item, a read's letter, the score table of a template letter, the wave-wide max
// scan.  Host side: the state a context keeps (grow-only buffers, the cached ladder table, the event pool), staging and
// read-back of a host-memory call from a list the unit writes once, timing, release.  A unit keeps its kernels, its own
// argument fields, its limits and its error string (every host function here takes that string).  The HIP-free part --
// ladder key and packing, argument checks, bucket_order -- is in ladder_host.h.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

#include <hip/hip_runtime.h>
#include "ladder_host.h"

namespace side_unit {
using namespace ladder_host;

// ---- device side ------------------------------------------------------------------------------------------------------
// The fields of an argument block that fill_table writes and template_of reads, under these names in every unit's block
// (each unit keeps them where its block always had them: a kernel's code object depends on the layout):
//     const LadderRecord* ladders;  const uint8_t* letters;  int32_t n_ladders;  int32_t match, mismatch, gap_open, gap_extend;

// template tpl (db order) of ladder lad: column c is tr[c] below trunk and br[c - trunk] from there on
struct Template {
    int trunk, tlen;
    const uint8_t *tr, *br;
};

// how many templates a ladder has (db order: unit by unit, the forward strand first), and the length of template tpl,
// which is the same on both strands
__device__ __forceinline__ int n_templates(const LadderRecord& d) { return d.max_units > 0 ? 2 * d.max_units : 1; }
__device__ __forceinline__ int template_len(const LadderRecord& d, int tpl) {
    return d.alen[0] + (d.max_units > 0 ? d.period * (tpl / 2 + 1) : 0) + d.blen[0];
}

// false where (lad, tpl) names no template of the table.  The record is read in place, the strand's fields alone: each
// load waits for the strand, which a wavefront that decodes one item does not notice.  The kernels whose lanes decode an
// item each (pileup.hip's validate, cigar_unit.h's decode_item) copy the record instead, as they always did.
template <class Block>
__device__ __forceinline__ bool template_of(const Block& a, int lad, int tpl, Template& t) {
    if (lad < 0 || lad >= a.n_ladders) return false;
    const LadderRecord& d = a.ladders[lad];
    const int max_units = d.max_units;
    if (tpl < 0 || tpl >= n_templates(d)) return false;
    const int strand = max_units > 0 ? (tpl & 1) : 0;
    t.trunk = d.alen[strand] + (max_units > 0 ? d.period * (tpl / 2 + 1) : 0);
    t.tlen = t.trunk + d.blen[strand];
    t.tr = a.letters + d.trunk_off[strand];
    t.br = a.letters + d.branch_off[strand];
    return true;
}

// letter ri of a packed read (nb words of 2-bit codes, then the N mask): 0..3, or 4 where the mask is set
__device__ __forceinline__ int read_code(const uint32_t* rec, int nb, int ri) {
    return ((rec[nb + (ri >> 5)] >> (ri & 31)) & 1u) ? 4 : (int)((rec[ri >> 4] >> ((ri & 15) * 2)) & 3u);
}

// 5-bit fields, field k = 16 + score of read code k (0..3, 4 = N) against template letter `let`; field 5 is 0, the -16
// of sw_long.hip's padding rows
__device__ __forceinline__ uint32_t score_lut(int let, int match, int mismatch) {
    uint32_t lut = 0;
    for (int k = 0; k < 5; ++k) {
        const int s = (k == 4 || let > 3) ? 0 : k == let ? match : -mismatch;   // N on either side scores 0
        lut |= (uint32_t)(s + 16) << (5 * k);
    }
    return lut;
}

// inclusive max scan over the 64 lanes (int or long long)
template <class T>
__device__ __forceinline__ T wave_incl_max(T x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, (unsigned)d, 64);
        if (lane >= d) x = x > y ? x : y;
    }
    return x;
}

// exclusive: the maximum of the lanes below this one, `none` in lane 0
template <class T>
__device__ __forceinline__ T wave_excl_max(T x, int lane, T none) {
    const T up = __shfl_up(wave_incl_max(x, lane), 1u, 64);
    return lane == 0 ? none : up;
}

// ---- host side --------------------------------------------------------------------------------------------------------
#define SIDE_UNIT_CHK(err, expr)                                                                 \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) return fail(err, -10, "%s: %s", #expr, hipGetErrorString(e_));     \
    } while (0)

struct Dev { void* p = nullptr; size_t cap = 0; };

// slack: a buffer grows by a quarter more than asked; without it the size is exact (its cap is a promise)
inline int ensure(std::string& err, Dev& b, size_t bytes, hipStream_t st, bool slack = true) {
    bytes = std::max<size_t>(bytes, 16);
    if (b.cap >= bytes) return 0;
    if (b.p) {
        SIDE_UNIT_CHK(err, hipStreamSynchronize(st));        // the buffer may still be in use by enqueued work
        SIDE_UNIT_CHK(err, hipFree(b.p));
        b = Dev();
    }
    const size_t want = slack ? bytes + bytes / 4 : bytes;
    SIDE_UNIT_CHK(err, hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

// what the calls on one context hold (grow-only, reused across calls); a unit adds its workspaces
struct StateBase {
    std::string ladder_key;
    int n_ladders = 0;
    Dev ladders, letters;
    std::vector<Dev> st;               // the arrays of a host-memory call, in the order of the unit's list
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t used = 0;
    int64_t launches = 0;
    double total_ms = 0;
};

// a unit's states, one per context
template <class State>
struct Registry {
    std::mutex mu;
    std::map<tredgpu_ctx*, State*> states;
    State* state_of(tredgpu_ctx* ctx) {
        std::lock_guard<std::mutex> lock(mu);
        State*& s = states[ctx];
        if (!s) s = new State();
        return s;
    }
    State* take(tredgpu_ctx* ctx) {      // null when the context has none
        std::lock_guard<std::mutex> lock(mu);
        auto it = states.find(ctx);
        State* s = it == states.end() ? nullptr : it->second;
        if (s) states.erase(it);
        return s;
    }
};

inline hipStream_t stream_of(tredgpu_ctx* ctx) { return (hipStream_t)tredgpu_get_stream(ctx); }

// the context's stream, with its device made current
inline int select_device(std::string& err, tredgpu_ctx* ctx, hipStream_t& st) {
    st = stream_of(ctx);
    int dev = 0;
    SIDE_UNIT_CHK(err, hipStreamGetDevice(st, &dev));
    SIDE_UNIT_CHK(err, hipSetDevice(dev));
    return 0;
}

// the ladder table of the call (ladder_host::pack_ladders), uploaded only when it differs from the previous call's; a
// refused table leaves the previous one in place
inline int set_ladders(std::string& err, StateBase& s, hipStream_t st, const Table& t, int max_template, bool plain_limits = false) {
    std::string key;
    std::vector<LadderRecord> lad;
    Codes pool;
    int rc;
    if ((rc = ladder_key(err, t, key))) return rc;
    if (s.n_ladders == t.n && key == s.ladder_key) return 0;
    if ((rc = pack_ladders(err, t, max_template, lad, pool, plain_limits))) return rc;
    if ((rc = ensure(err, s.ladders, lad.size() * sizeof(LadderRecord), st))) return rc;
    if ((rc = ensure(err, s.letters, pool.size(), st))) return rc;
    SIDE_UNIT_CHK(err, hipStreamSynchronize(st));
    if (t.n) SIDE_UNIT_CHK(err, hipMemcpy(s.ladders.p, lad.data(), lad.size() * sizeof(LadderRecord), hipMemcpyHostToDevice));
    SIDE_UNIT_CHK(err, hipMemcpy(s.letters.p, pool.data(), pool.size(), hipMemcpyHostToDevice));
    s.ladder_key.swap(key);
    s.n_ladders = t.n;
    return 0;
}

// the table and scoring fields of a unit's argument block: the state's ladder table and the call's scoring
template <class Block>
void fill_table(Block& a, const StateBase& s, const tredgpu_sw_params& p) {
    a.ladders = (const LadderRecord*)s.ladders.p;
    a.letters = (const uint8_t*)s.letters.p;
    a.n_ladders = s.n_ladders;
    a.match = p.match; a.mismatch = p.mismatch; a.gap_open = p.gap_open; a.gap_extend = p.gap_extend;
}

// One array of a host-memory call, as a unit's list names it: the pointer of the argument block that stage() points at
// the device's copy, the caller's array and its size.  arr_in: copied to the device by stage(); arr_out: copied back by
// read_back(); arr_scratch: on the device only.
struct Array {
    void* slot;
    const void* src;
    void* dst;
    size_t bytes;
};
template <class T>
Array arr_in(const T*& dev, const T* host, size_t count) { return Array{&dev, host, nullptr, count * sizeof(T)}; }
template <class T>
Array arr_out(T*& dev, T* host, size_t count) { return Array{&dev, nullptr, host, count * sizeof(T)}; }
template <class T>
Array arr_scratch(T*& dev, size_t count) { return Array{&dev, nullptr, nullptr, count * sizeof(T)}; }

// sizes the state's buffers for the list, enqueues the copies of its inputs and points the block at the device's arrays
inline int stage(std::string& err, StateBase& s, hipStream_t st, const std::vector<Array>& arrays) {
    int rc;
    if (s.st.size() < arrays.size()) s.st.resize(arrays.size());
    for (size_t k = 0; k < arrays.size(); ++k)
        if ((rc = ensure(err, s.st[k], arrays[k].bytes, st))) return rc;
    for (size_t k = 0; k < arrays.size(); ++k) {
        const Array& a = arrays[k];
        if (a.src && a.bytes) SIDE_UNIT_CHK(err, hipMemcpyAsync(s.st[k].p, a.src, a.bytes, hipMemcpyHostToDevice, st));
        memcpy(a.slot, &s.st[k].p, sizeof(void*));
    }
    return 0;
}

// the end of a host-memory call: the list's outputs to the caller's arrays, and the stream drained (whatever of the
// caller's an enqueued copy reads is free from here on)
inline int read_back(std::string& err, const StateBase& s, hipStream_t st, const std::vector<Array>& arrays) {
    for (size_t k = 0; k < arrays.size(); ++k)
        if (arrays[k].dst && arrays[k].bytes)
            SIDE_UNIT_CHK(err, hipMemcpyAsync(arrays[k].dst, s.st[k].p, arrays[k].bytes, hipMemcpyDeviceToHost, st));
    SIDE_UNIT_CHK(err, hipStreamSynchronize(st));
    return 0;
}

// the finished event pairs into the totals (the stream is drained)
inline void fold(StateBase& s) {
    for (size_t i = 0; i < s.used; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.events[i].first, s.events[i].second) == hipSuccess) { s.total_ms += ms; s.launches += 1; }
    }
    s.used = 0;
}

// one event pair per call around the unit's launches: timed_begin, the launches, timed_end
inline int timed_begin(std::string& err, StateBase& s, hipStream_t st) {
    if (s.used == s.events.size()) {
        if (s.used >= 256) {                    // bounded pool: fold what is already finished
            SIDE_UNIT_CHK(err, hipStreamSynchronize(st));
            fold(s);
        } else {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            SIDE_UNIT_CHK(err, hipEventCreate(&e0));
            SIDE_UNIT_CHK(err, hipEventCreate(&e1));
            s.events.emplace_back(e0, e1);
        }
    }
    SIDE_UNIT_CHK(err, hipEventRecord(s.events[s.used].first, st));
    return 0;
}

inline int timed_end(std::string& err, StateBase& s, hipStream_t st) {
    SIDE_UNIT_CHK(err, hipGetLastError());
    SIDE_UNIT_CHK(err, hipEventRecord(s.events[s.used].second, st));
    s.used += 1;
    return 0;
}

// *_get_timing / *_timing, and with reset *_reset_timing
template <class State>
int timing(std::string& err, Registry<State>& reg, tredgpu_ctx* ctx, int64_t* launches, double* total_ms, bool reset) {
    if (!ctx) return fail(err, -2, "ctx is NULL");
    StateBase& s = *reg.state_of(ctx);
    SIDE_UNIT_CHK(err, hipStreamSynchronize(stream_of(ctx)));
    fold(s);
    if (reset) { s.launches = 0; s.total_ms = 0; }
    if (launches) *launches = s.launches;
    if (total_ms) *total_ms = s.total_ms;
    return 0;
}

// *_release: per context, idempotent; extra: the unit's own workspaces
template <class State>
void release(Registry<State>& reg, tredgpu_ctx* ctx, std::initializer_list<Dev State::*> extra) {
    State* s = reg.take(ctx);
    if (!s) return;
    (void)hipStreamSynchronize(stream_of(ctx));
    for (Dev State::*b : extra) (void)hipFree((s->*b).p);            // (a null pointer is no error)
    for (Dev* b : {&s->ladders, &s->letters}) (void)hipFree(b->p);
    for (Dev& b : s->st) (void)hipFree(b.p);
    for (auto& ev : s->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    delete s;
}

}  // namespace side_unit
