// cigar_unit.h -- what the two CIGAR units (sw_cigar.hip: one lane one item; sw_cigar_long.hip: one wavefront one item)
// share, so that an item is decoded, refused, traced back and reported by ONE text whichever unit Context.sw_cigar sends
// it to.  Device side: argument block, item decode with its refusals, read letter, direction byte, traceback, epilogue.
// Host side: the state a context keeps, ladder upload, staging of a host-memory call, event pool and timing, release.  A
// unit keeps its pass, kernels, workspaces, limits and error string (every host function here takes that string).  The
// HIP-free part -- ladder key and packing, argument checks -- is in ladder_host.h.
#pragma once
#include <algorithm>
#include <map>
#include <mutex>

#include <hip/hip_runtime.h>
#include "ladder_host.h"
#include "../../include/tredcigar.h"

namespace cigar_unit {
using namespace ladder_host;

// ---- device side ------------------------------------------------------------------------------------------------------
struct Args {
    const uint32_t* packed;
    const int64_t* read_off;
    const int32_t *read_len, *item_ladder, *item_template;
    const int16_t* fields;
    const LadderRecord* ladders;
    const uint8_t* letters;
    int32_t n_ladders;
    int64_t n_items;
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t cap;
    uint32_t* out_ops;
    int32_t *out_n_ops, *out_status;
    uint8_t* plane;        // the direction plane, in the unit's layout
};

// an item the decode accepted: the rectangle ref[ref_begin..ref_end] x read[read_begin..read_end] and where its letters are
struct Item {
    int score, ref_begin, ref_end, read_begin, read_end;
    int L, refLen, readLen, trunk;     // template column c is tr[c] below trunk and br[c - trunk] from there on
    const uint8_t *tr, *br;
    const uint32_t* rec;               // the read's words: nb of 2-bit codes, then the N mask
    int nb;
};

// Decodes an item and hands it to the unit's pass, whose status it returns -- or the status of an item the unit does not
// take (max_read / max_template: the unit's limits).  The pass is a callable so that each refusal is a return of its own:
// behind a status merged from them the compiler no longer knows what the checks established (1 <= refLen, readLen <= 2^16).
template <class Pass>
__device__ __forceinline__ int decode_item(const Args& a, int64_t item, int max_read, int max_template, Pass pass) {
    const int lad = a.item_ladder[item], tpl = a.item_template[item];
    const int16_t* fl = a.fields + (size_t)item * 5;
    const int score = fl[0], ref_begin = fl[1], ref_end = fl[2], read_begin = fl[3], read_end = fl[4];
    const int L = a.read_len[item];
    if (lad < 0 || lad >= a.n_ladders) return TREDGPU_CIGAR_BAD_ITEM;
    const LadderRecord d = a.ladders[lad];
    if (tpl < 0 || tpl >= (d.max_units > 0 ? 2 * d.max_units : 1)) return TREDGPU_CIGAR_BAD_ITEM;
    const int strand = d.max_units > 0 ? (tpl & 1) : 0;
    const int trunk = d.alen[strand] + (d.max_units > 0 ? d.period * (tpl / 2 + 1) : 0);
    const int tlen = trunk + d.blen[strand];
    if (L > max_read || tlen > max_template) return TREDGPU_CIGAR_TOO_LONG;
    if (ref_begin < 0 || ref_end < ref_begin || ref_end >= tlen || read_begin < 0 || read_end < read_begin || read_end >= L)
        return TREDGPU_CIGAR_BAD_ITEM;
    const Item it{score, ref_begin, ref_end, read_begin, read_end, L, ref_end - ref_begin + 1, read_end - read_begin + 1, trunk,
                  a.letters + d.trunk_off[strand], a.letters + d.branch_off[strand], a.packed + a.read_off[item], (L + 15) >> 4};
    return pass(it);
}

// letter ri of a packed read: 0..3, or 4 where the N mask is set
__device__ __forceinline__ int read_code(const uint32_t* rec, int nb, int ri) {
    return ((rec[nb + (ri >> 5)] >> (ri & 31)) & 1u) ? 4 : (int)((rec[ri >> 4] >> ((ri & 15) * 2)) & 3u);
}

// the three direction codes of a cell in one byte: bit 0 E's (2/3), bit 1 F's (4/5), bits 2-4 H's (1-5)
__device__ __forceinline__ uint8_t dir_pack(int de, int df, int dh) { return (uint8_t)((de - 2) | ((df - 4) << 1) | (dh << 2)); }
// the step out of a cell the traceback entered in E (which 0), F (1) or H (2)
__device__ __forceinline__ int dir_step(int c, int which) { return which == 0 ? 2 + (c & 1) : which == 1 ? 4 + ((c >> 1) & 1) : (c >> 2); }

// The traceback of ssw.c:636-726 from the rectangle's last cell to row 0 over the plane of the pass whose band was bw;
// cell(i, j) is the byte of row i, column j in the unit's addressing.  Writes the item's operations and out_n_ops and
// returns its status.
template <class Cell>
__device__ __forceinline__ int traceback(const Args& a, int64_t item, const Item& it, int bw, Cell cell) {
    uint32_t* ops = a.out_ops + (size_t)item * a.cap;
    int i = it.readLen - 1, j = it.refLen - 1, e = 0, l = 0, which = 2, op = 0, prev = 0;
    auto emit = [&](uint32_t v) { if (l < a.cap) ops[l] = v; ++l; };
    while (i > 0) {
        if (j < max(0, i - bw) || j > i + bw) return TREDGPU_CIGAR_OFF_EDGE;          // a cell this pass never wrote
        switch (dir_step(cell(i, j), which)) {
            case 1: --i; --j; which = 2; op = 0; break;
            case 2: --i; which = 0; op = 1; break;
            case 3: --i; which = 2; op = 1; break;
            case 4: --j; which = 1; op = 2; break;
            default: --j; which = 2; op = 2; break;
        }
        if (op == prev) ++e;
        else { emit((uint32_t)e << 4 | prev); prev = op; e = 1; }
    }
    if (op == 0) emit((uint32_t)(e + 1) << 4);
    else { emit((uint32_t)e << 4 | op); emit(1u << 4); }
    a.out_n_ops[item] = l;
    if (l > a.cap) return TREDGPU_CIGAR_OVERFLOW;
    for (int s = 0, t = l - 1; s < t; ++s, --t) { const uint32_t v = ops[s]; ops[s] = ops[t]; ops[t] = v; }   // :717-726
    return TREDGPU_CIGAR_OK;
}

// entries first, first + step, ... of the item's row of out_ops (a lane alone: 0, 1; a wavefront: lane, 64)
__device__ __forceinline__ void zero_ops(const Args& a, int64_t item, const int first, const int step) {
    uint32_t* ops = a.out_ops + (size_t)item * a.cap;
    for (int k = first; k < a.cap; k += step) ops[k] = 0;
}

// the status of a finished item; n_ops is the traceback's only where it ran to its end (OK, OVERFLOW).  An item that is
// not OK gets zero_ops as well.
__device__ __forceinline__ void store_status(const Args& a, int64_t item, int status) {
    a.out_status[item] = status;
    if (status != TREDGPU_CIGAR_OK && status != TREDGPU_CIGAR_OVERFLOW) a.out_n_ops[item] = 0;
}

// ---- host side --------------------------------------------------------------------------------------------------------
#define CIGAR_UNIT_CHK(err, expr)                                                                \
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
        CIGAR_UNIT_CHK(err, hipStreamSynchronize(st));       // the buffer may still be in use by enqueued work
        CIGAR_UNIT_CHK(err, hipFree(b.p));
        b = Dev();
    }
    const size_t want = slack ? bytes + bytes / 4 : bytes;
    CIGAR_UNIT_CHK(err, hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

// what the calls on one context hold (grow-only, reused across calls); a unit adds its workspaces
struct StateBase {
    std::string ladder_key;
    int n_ladders = 0;
    Dev ladders, letters, st[9];       // st: the six inputs and three outputs of a host-memory call
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
    CIGAR_UNIT_CHK(err, hipStreamGetDevice(st, &dev));
    CIGAR_UNIT_CHK(err, hipSetDevice(dev));
    return 0;
}

// the ladder table of the call (ladder_host::pack_ladders), uploaded only when it differs from the previous call's; a
// refused table leaves the previous one in place
inline int set_ladders(std::string& err, StateBase& s, hipStream_t st, const Table& t, int max_template) {
    std::string key;
    std::vector<LadderRecord> lad;
    Codes pool;
    int rc;
    if ((rc = ladder_key(err, t, key))) return rc;
    if (s.n_ladders == t.n && key == s.ladder_key) return 0;
    if ((rc = pack_ladders(err, t, max_template, lad, pool))) return rc;
    if ((rc = ensure(err, s.ladders, lad.size() * sizeof(LadderRecord), st))) return rc;
    if ((rc = ensure(err, s.letters, pool.size(), st))) return rc;
    CIGAR_UNIT_CHK(err, hipStreamSynchronize(st));
    if (t.n) CIGAR_UNIT_CHK(err, hipMemcpy(s.ladders.p, lad.data(), lad.size() * sizeof(LadderRecord), hipMemcpyHostToDevice));
    CIGAR_UNIT_CHK(err, hipMemcpy(s.letters.p, pool.data(), pool.size(), hipMemcpyHostToDevice));
    s.ladder_key.swap(key);
    s.n_ladders = t.n;
    return 0;
}

// the arguments of a call as the caller gave them, with the state's ladder table
inline void fill_args(Args& a, const StateBase& s, const uint32_t* packed, const int64_t* read_off, const int32_t* read_len,
                      int64_t n_items, const int32_t* item_ladder, const int32_t* item_template, const int16_t* fields,
                      const tredgpu_sw_params& p, int32_t cap, uint32_t* out_ops, int32_t* out_n_ops, int32_t* out_status) {
    a.packed = packed; a.read_off = read_off; a.read_len = read_len;
    a.item_ladder = item_ladder; a.item_template = item_template; a.fields = fields;
    a.out_ops = out_ops; a.out_n_ops = out_n_ops; a.out_status = out_status;
    a.ladders = (const LadderRecord*)s.ladders.p;
    a.letters = (const uint8_t*)s.letters.p;
    a.n_ladders = s.n_ladders;
    a.n_items = n_items;
    a.match = p.match; a.mismatch = p.mismatch; a.gap_open = p.gap_open; a.gap_extend = p.gap_extend;
    a.cap = cap;
}

// a host-memory call: copies the six inputs `a` points to into the state's staging buffers, sizes the three outputs and
// points `a` at the device's arrays
inline int stage(std::string& err, StateBase& s, hipStream_t st, Args& a) {
    const size_t n = (size_t)a.n_items;
    const size_t sizes[9] = {(size_t)a.read_off[n] * 4, (n + 1) * 8, n * 4, n * 4, n * 4, n * 10,
                             n * a.cap * sizeof(uint32_t), n * 4, n * 4};
    const void* src[6] = {a.packed, a.read_off, a.read_len, a.item_ladder, a.item_template, a.fields};
    int rc;
    for (int k = 0; k < 9; ++k)
        if ((rc = ensure(err, s.st[k], sizes[k], st))) return rc;
    for (int k = 0; k < 6; ++k)
        if (sizes[k]) CIGAR_UNIT_CHK(err, hipMemcpyAsync(s.st[k].p, src[k], sizes[k], hipMemcpyHostToDevice, st));
    auto at = [&s](auto& ptr, int k) { ptr = static_cast<std::remove_reference_t<decltype(ptr)>>(s.st[k].p); };
    at(a.packed, 0); at(a.read_off, 1); at(a.read_len, 2); at(a.item_ladder, 3); at(a.item_template, 4); at(a.fields, 5);
    at(a.out_ops, 6); at(a.out_n_ops, 7); at(a.out_status, 8);
    return 0;
}

// the end of a host-memory call: the three outputs of `a` to the caller's arrays, and the stream drained
inline int read_back(std::string& err, hipStream_t st, const Args& a, uint32_t* out_ops, int32_t* out_n_ops, int32_t* out_status) {
    const size_t n = (size_t)a.n_items;
    CIGAR_UNIT_CHK(err, hipMemcpyAsync(out_ops, a.out_ops, n * a.cap * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CIGAR_UNIT_CHK(err, hipMemcpyAsync(out_n_ops, a.out_n_ops, n * 4, hipMemcpyDeviceToHost, st));
    CIGAR_UNIT_CHK(err, hipMemcpyAsync(out_status, a.out_status, n * 4, hipMemcpyDeviceToHost, st));
    CIGAR_UNIT_CHK(err, hipStreamSynchronize(st));
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
            CIGAR_UNIT_CHK(err, hipStreamSynchronize(st));
            fold(s);
        } else {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            CIGAR_UNIT_CHK(err, hipEventCreate(&e0));
            CIGAR_UNIT_CHK(err, hipEventCreate(&e1));
            s.events.emplace_back(e0, e1);
        }
    }
    CIGAR_UNIT_CHK(err, hipEventRecord(s.events[s.used].first, st));
    return 0;
}

inline int timed_end(std::string& err, StateBase& s, hipStream_t st) {
    CIGAR_UNIT_CHK(err, hipGetLastError());
    CIGAR_UNIT_CHK(err, hipEventRecord(s.events[s.used].second, st));
    s.used += 1;
    return 0;
}

// *_get_timing / *_timing, and with reset *_reset_timing
template <class State>
int timing(std::string& err, Registry<State>& reg, tredgpu_ctx* ctx, int64_t* launches, double* total_ms, bool reset) {
    if (!ctx) return fail(err, -2, "ctx is NULL");
    StateBase& s = *reg.state_of(ctx);
    CIGAR_UNIT_CHK(err, hipStreamSynchronize(stream_of(ctx)));
    fold(s);
    if (reset) { s.launches = 0; s.total_ms = 0; }
    if (launches) *launches = s.launches;
    if (total_ms) *total_ms = s.total_ms;
    return 0;
}

// *_release: per context, idempotent; extra: the unit's own buffers
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

}  // namespace cigar_unit
