// inflater_api.hip -- the C ABI of the front end on the device (include/tredgpu.h section 4: tredgpu_inflater_*,
// tredgpu_inflate_blocks[_crc], tredgpu_inflate_walk, tredgpu_inflater_fetch[_dense]): buffers, streams, the order of the
// launches.  The kernels are inflate_decode.hip's and walk.hip's (inflater_internal.h).
#include <hip/hip_runtime.h>
#include <cstring>
#include <ctime>
#include <cstdlib>
#include <cstdio>
#include <stdint.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "inflater_internal.h"
#include "inflater_host.h"

using namespace tredgpu_front;
using namespace inflater_host;

// ---- C ABI (include/tredgpu.h) ------------------------------------------------------------------------------------
// A call is cut into slices of blocks that alternate between two streams: the copy-in and the decoding of slice k + 1
// run beside the copy-out of slice k (the copy-out is the long pole: four bytes leave for every byte that arrives).
constexpr int MAX_SLICES = 8;
constexpr int SLICE_BLOCKS = 4096;      // >= 4 096 wavefronts per launch: 16 per CU, and two launches run side by side

// ---- owned buffers: each knows its kind and its room, and enters itself in one of the inflater's two sets -- release() and
// tredgpu_inflater_pinned_bytes walk the sets, so a buffer declared in the struct cannot be missing from either.
// cap counts entries of `unit` bytes (growth was always rounded in entries: the allocation sizes depend on it).
struct Buf {
    enum Kind { DEVICE = 1, PINNED = 2, PAIR = 3 };
    const Kind kind; const size_t unit; size_t cap = 0;
    Buf(std::vector<Buf*>& set, Kind k, size_t u) : kind(k), unit(u) { set.push_back(this); }
    Buf(const Buf&) = delete;
    size_t pinned_bytes() const { return (kind & PINNED) ? cap * unit : 0; }
    void free() { if (host) (void)hipHostFree(host); if (dev) (void)hipFree(dev); host = dev = nullptr; cap = 0; }
    hipError_t alloc(size_t c) {                     // exactly c entries; {nullptr, 0} when that fails
        free();
        hipError_t e = (kind & PINNED) ? hipHostMalloc(&host, c * unit, hipHostMallocDefault) : hipSuccess;
        if (e == hipSuccess && (kind & DEVICE)) e = hipMalloc(&dev, c * unit);
        if (e == hipSuccess) cap = c; else free();
        return e;
    }
    hipError_t grow(size_t need, Slack s) { return need <= cap ? hipSuccess : alloc(next_cap(need, cap, s)); }
protected:
    void *host = nullptr, *dev = nullptr;
};
template <Buf::Kind K> struct BufOf : Buf {          // h(): the pinned side, d(): the device side -- of a kind that has one
    BufOf(std::vector<Buf*>& set, size_t u = 1) : Buf(set, K, u) {}
    template <class T = uint8_t> T* h() const { static_assert(K & PINNED, "no pinned side"); return (T*)host; }
    template <class T = uint8_t> T* d() const { static_assert(K & DEVICE, "no device side"); return (T*)dev; }
};
using DeviceBuf = BufOf<Buf::DEVICE>; using PinnedBuf = BufOf<Buf::PINNED>; using PairBuf = BufOf<Buf::PAIR>;   // (a pair: the same layout on both sides)

struct tredgpu_inflater {
    int device = 0;
    hipStream_t stream[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};   // waited for asleep (polled): see tredgpu_inflate_blocks
    hipEvent_t t0[2] = {}, t1[2] = {}, k0[MAX_SLICES] = {}, k1[MAX_SLICES] = {};   // timing (tredgpu_inflater_timing)
    int last_slices = 0, last_streams = 0;
    std::vector<Buf*> decode_bufs, walk_bufs;         // (tredgpu_inflater_reserve and _host_out release the first set alone)
    // the staging: the caller fills comp and off and reads out in place; all of it grows together (tredgpu_inflater_reserve)
    PairBuf comp{decode_bufs};
    PinnedBuf h_out{decode_bufs}; DeviceBuf d_out{decode_bufs};
    bool host_out = true;                             // false (tredgpu_inflater_host_out): no pinned room for the whole output --
                                                      // the blocks the host wants come through tredgpu_inflater_fetch_dense
    PairBuf off{decode_bufs, 2 * sizeof(int64_t)};    // per block: comp_off[cap] then out_off[cap]
    PairBuf status{decode_bufs, 2 * sizeof(int32_t)}; //            status[cap] then crc[cap]
    PinnedBuf dense{decode_bufs};                     // the fetched blocks, one after the other
    PairBuf pieces{decode_bufs, sizeof(FetchPiece)};  // the fetch kernel's copy table
    size_t cap_blocks() const { return off.cap; }
    int64_t* h_ooff() const { return off.h<int64_t>() + off.cap; }
    // the pair walk (tredgpu_inflate_walk): a stream of its own, the file's view of the blocks, tasks, per-task tables, pools
    hipStream_t wstream = nullptr, astream = nullptr;          // (astream: the alternative loci's walks, beside the pair walks)
    hipEvent_t adone = nullptr;
    hipEvent_t wdone = nullptr, w0 = nullptr, w1 = nullptr, decoded[2] = {nullptr, nullptr};
    bool walk_timed = false, big_lds_allowed = false;
    int walk_table_cap = 0;
    size_t last_walk_tasks = 0;                       // regions of the last walk call (tredgpu_inflater_walk_serial_regions)
    PairBuf wblk{walk_bufs}, wtask{walk_bufs}, wres{walk_bufs};   // the packed arrays BlockTable, TaskTable, ResultTable (inflater_host.h)
    PairBuf atask{walk_bufs}, ares{walk_bufs};                    // the alternative loci's TaskTable and AltResultTable
    DeviceBuf wpairs{walk_bufs, WALK_PAIR_CAP * sizeof(WalkPair)}, wchained{walk_bufs, sizeof(WalkChained)};               // per task
    DeviceBuf wrecs{walk_bufs, sizeof(WalkRec)}, wfields{walk_bufs, sizeof(WalkFields)};   // per record: the chain's list, the parsed fields
    // the read selection (tredgpu.h section 5): per task its parameters and result, and TREDGPU_SELECT_CAP record places
    PairBuf sel{walk_bufs};                                                        // SelectTable
    DeviceBuf sel_list{walk_bufs, TREDGPU_SELECT_CAP * sizeof(int64_t)};           // per task
    int sel_tasks = 0;                                                             // tasks of the last walk with a selection (0: none)
    hipEvent_t aready = nullptr;                                                   // the alternative loci's walk has run (the selection reads its hits)
    DeviceBuf gpool{walk_bufs}, tpool{walk_bufs};     // (device pools: the call's bound)
    PinnedBuf h_gpool{walk_bufs}, h_tpool{walk_bufs}; // (pinned host pools: what the walks really produced, an eighth more)
    std::string err;
};

namespace {
thread_local std::string g_inflate_error;

// TREDGPU_TRACE=1: host-side timestamps of a call's phases on stderr (milliseconds since the call began)
struct CallTrace {
    bool on; const char* what; double t0; std::string line;
    static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
    explicit CallTrace(const char* w) : on(getenv("TREDGPU_TRACE") != nullptr), what(w), t0(on ? now() : 0) {}
    void mark(const char* k) { if (on) { char b[64]; snprintf(b, sizeof b, " %s=%.2f", k, now() - t0); line += b; } }
    ~CallTrace() { if (on) fprintf(stderr, "[tredgpu %d] %s:%s\n", (int)getpid(), what, line.c_str()); }
};

int ifail(tredgpu_inflater* f, int code, const char* what, hipError_t e = hipSuccess) {
    std::string m = what;
    if (e != hipSuccess) { m += ": "; m += hipGetErrorString(e); }
    if (f) f->err = m; else g_inflate_error = m;
    return code;
}

#define ICHK(f, expr)                                             \
    do {                                                          \
        hipError_t e_ = (expr);                                   \
        if (e_ != hipSuccess) return ifail((f), -10, #expr, e_);  \
    } while (0)

void release(std::vector<Buf*>& set) { for (Buf* b : set) b->free(); }

void destroy_handles(tredgpu_inflater* f) {
    for (hipEvent_t e : {f->done[0], f->done[1], f->t0[0], f->t0[1], f->t1[0], f->t1[1]}) if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < MAX_SLICES; ++k) { if (f->k0[k]) (void)hipEventDestroy(f->k0[k]); if (f->k1[k]) (void)hipEventDestroy(f->k1[k]); }
    for (hipEvent_t e : {f->wdone, f->w0, f->w1, f->decoded[0], f->decoded[1], f->adone, f->aready}) if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : {f->stream[0], f->stream[1], f->wstream, f->astream}) if (st) (void)hipStreamDestroy(st);
}
}  // namespace

extern "C" {

int tredgpu_inflater_create(int device_id, tredgpu_inflater** out) {
    if (!out) return ifail(nullptr, -2, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return ifail(nullptr, -3, "no HIP device available; libtredgpu has no CPU fallback", e);
    if (device_id < 0 || device_id >= n) return ifail(nullptr, -2, "device out of range");
    tredgpu_inflater* f = new tredgpu_inflater();
    f->device = device_id;
    // the lowest stream priority: a genotyping launch of the same or another driver process should not queue up behind
    // several of these
    int lo_prio = 0, hi_prio = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
    e = hipSetDevice(device_id);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = create_partitioned_stream(&f->stream[k], hipStreamNonBlocking, lo_prio, 0, device_id);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f->done[k], hipEventBlockingSync | hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreate(&f->t0[k]);
        if (e == hipSuccess) e = hipEventCreate(&f->t1[k]);
    }
    for (int k = 0; k < MAX_SLICES && e == hipSuccess; ++k) {
        e = hipEventCreate(&f->k0[k]);
        if (e == hipSuccess) e = hipEventCreate(&f->k1[k]);
    }
    if (e == hipSuccess) e = create_partitioned_stream(&f->wstream, hipStreamNonBlocking, lo_prio, 0, device_id);
    if (e == hipSuccess) e = create_partitioned_stream(&f->astream, hipStreamNonBlocking, lo_prio, 0, device_id);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->adone, hipEventBlockingSync | hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->aready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->wdone, hipEventBlockingSync | hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&f->w0);
    if (e == hipSuccess) e = hipEventCreate(&f->w1);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&f->decoded[k], hipEventDisableTiming);
    if (e != hipSuccess) {
        destroy_handles(f);
        delete f;
        return ifail(nullptr, -10, "stream / event creation", e);
    }
    *out = f;
    return 0;
}

void tredgpu_inflater_destroy(tredgpu_inflater* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    for (hipStream_t st : f->stream) (void)hipStreamSynchronize(st);
    (void)hipStreamSynchronize(f->wstream);
    if (f->astream) (void)hipStreamSynchronize(f->astream);
    release(f->decode_bufs); release(f->walk_bufs);
    destroy_handles(f);
    delete f;
}

const char* tredgpu_inflater_last_error(const tredgpu_inflater* f) { return f ? f->err.c_str() : g_inflate_error.c_str(); }

int tredgpu_inflater_reserve(tredgpu_inflater* f, int64_t comp_bytes, int64_t out_bytes, int32_t n_blocks, uint8_t** comp_host,
                             uint8_t** out_host, int64_t** comp_off_host, int64_t** out_off_host) {
    if (!f) return -2;
    if (comp_bytes < 0 || out_bytes < 0 || n_blocks < 0 || !comp_host || !out_host || !comp_off_host || !out_off_host)
        return ifail(f, -2, "bad arguments");
    ICHK(f, hipSetDevice(f->device));
    const size_t need_c = (size_t)comp_bytes + 64, need_o = (size_t)out_bytes + 64, need_b = (size_t)n_blocks + 1;
    if (need_c > f->comp.cap || need_o > f->d_out.cap || need_b > f->cap_blocks()) {
        // one decision for all of the staging: every buffer of the set is let go, then each is given its new room
        for (hipStream_t st : f->stream) ICHK(f, hipStreamSynchronize(st));
        const size_t cc = next_cap(need_c, f->comp.cap, GROW_STAGING), co = next_cap(need_o, f->d_out.cap, GROW_STAGING), cb = next_cap(need_b, f->cap_blocks(), GROW_BLOCKS);
        release(f->decode_bufs);
        hipError_t e = f->comp.alloc(cc);
        if (e == hipSuccess && f->host_out) e = f->h_out.alloc(co);
        if (e == hipSuccess) e = f->d_out.alloc(co);
        if (e == hipSuccess) e = f->off.alloc(cb);
        if (e == hipSuccess) e = f->status.alloc(cb);
        if (e != hipSuccess) { release(f->decode_bufs); return ifail(f, -10, "staging allocation", e); }
    }
    *comp_host = f->comp.h(); *out_host = f->h_out.h();
    *comp_off_host = f->off.h<int64_t>(); *out_off_host = f->h_ooff();
    return 0;
}

}  // extern "C"

namespace {
int wait_asleep(tredgpu_inflater* f, hipEvent_t ev) {
    // hipEventSynchronize spins even on a hipEventBlockingSync event here (measured: CPU time = wall time, and calls of
    // other threads on other streams queue up behind the spinning one); the host threads that wait are the ones whose
    // cores the path is short of
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) return ifail(f, -10, "hipEventQuery", q);
        usleep(100);
    }
}

// ---- one call (run_inflate below): what its steps share -------------------------------------------------------------------
struct Call {
    tredgpu_inflater* f; int32_t n_blocks; int32_t* status; uint32_t* crc; bool copy_out; tredgpu_walk_args* w;
    const int64_t *coff = f->off.h<int64_t>(), *ooff = f->h_ooff();          // the caller's offsets, in the pinned staging
    int64_t *d_coff = f->off.d<int64_t>(), *d_ooff = d_coff + f->cap_blocks(); int32_t* d_crc = f->status.d<int32_t>() + f->cap_blocks();
    bool want_crc = crc != nullptr || w != nullptr;
    int slices = std::min(MAX_SLICES, std::max(1, n_blocks / SLICE_BLOCKS)), nstreams = slices > 1 ? 2 : 1;
    // the walk's sizes (select: a selection over at least one task), its plan and where the parts of its packed arrays lie
    size_t n_tasks = 0, n_alt = 0; bool select = false; WalkPlan plan = {0, false};
    BlockTable blk = {0}; TaskTable task = {0, 0}, atask = {0, 0}; ResultTable res = {0}; AltResultTable ares = {0, 0}; SelectTable sel = {0};
    int check(), grow_walk(), stage_walk(), enqueue_decode(), enqueue_walk(), collect(CallTrace& tr);     // the steps, in this order
};

// 1. the blocks, then the walk's arguments: a refusal comes before anything is allocated or enqueued
int Call::check() {
    const char* bad = check_blocks(coff, ooff, n_blocks, f->comp.cap, f->d_out.cap);
    if (bad) return ifail(f, -2, bad);
    if (!w) return 0;
    if (w->n_tasks < 0 || w->n_chunks < 0 || !w->blk_coffset || !w->blk_clen || !w->blk_crc || (w->n_tasks > 0 && (!w->tasks || !w->results)) ||
        (w->n_chunks > 0 && !w->chunks) || w->cap_global < 0 || w->cap_target < 0 || (w->cap_global > 0 && !w->global_pool) ||
        (w->cap_target > 0 && !w->target_pool))
        return ifail(f, -2, "bad walk arguments");
    const size_t nb = (size_t)n_blocks, n_chunks = (size_t)w->n_chunks, n_alt_chunks = (size_t)std::max(w->n_alt_chunks, 0);
    n_tasks = (size_t)w->n_tasks;
    if ((bad = check_tasks(w->tasks, n_tasks, n_chunks, n_blocks)) || (bad = check_chunks(w->chunks, n_chunks))) return ifail(f, -2, bad);
    n_alt = (size_t)std::max(w->n_alt_tasks, 0);
    if (w->n_alt_tasks < 0 || w->n_alt_chunks < 0 || (n_alt > 0 && (!w->alt_tasks || !w->alt_results || !w->need)) || (n_alt_chunks > 0 && !w->alt_chunks))
        return ifail(f, -2, "bad walk arguments (alternative loci)");
    if ((bad = check_tasks(w->alt_tasks, n_alt, n_alt_chunks, n_blocks)) || (bad = check_chunks(w->alt_chunks, n_alt_chunks))) return ifail(f, -2, bad);
    if ((w->select != nullptr) != (w->selected != nullptr)) return ifail(f, -2, "select and selected go together");
    for (size_t t = 0; w->select && t < n_tasks; ++t) {
        const tredgpu_select_task& S = w->select[t];
        if (S.n_alt > 0 && (S.alt_first < 0 || (size_t)S.alt_first + (size_t)S.n_alt > n_alt)) return ifail(f, -2, "select task outside the alternative loci's tasks");
    }
    select = w->select && n_tasks > 0;
    blk = {nb}; task = {n_tasks, n_chunks}; atask = {n_alt, n_alt_chunks}; res = {n_tasks}; ares = {n_alt, nb}; sel = {n_tasks};
    return 0;
}

// 2. all the walk's buffers; the plan (the record room, the name table) is written where the tasks are staged
int Call::grow_walk() {
    f->sel_tasks = 0;
    if (w->select) {
        ICHK(f, f->sel.grow(sel.bytes() + PAD, GROW_WALK));
        ICHK(f, f->sel_list.grow(n_tasks, GROW_LISTS));
    }
    if (n_alt > 0) {
        ICHK(f, f->atask.grow(atask.rec_base() + PAD, GROW_WALK));
        ICHK(f, f->ares.grow(ares.bytes() + PAD, GROW_WALK));
    }
    ICHK(f, f->wblk.grow(blk.bytes() + PAD, GROW_WALK));
    ICHK(f, f->wtask.grow(task.bytes() + PAD, GROW_WALK));
    plan = plan_walk(w->tasks, n_tasks, w->chunks, w->blk_coffset, ooff, part<int64_t>(f->wtask.h(), task.rec_base()));
    ICHK(f, f->wrecs.grow(plan.total_recs, GROW_WALK));
    ICHK(f, f->wfields.grow(plan.total_recs, GROW_WALK));
    ICHK(f, f->wchained.grow(n_tasks, GROW_WALK));
    ICHK(f, f->wres.grow(res.counters() + PAD, GROW_WALK));          // (the counters lie in the pad)
    ICHK(f, f->wpairs.grow(n_tasks, GROW_WALK));
    // (the pools on the device hold the call's BOUND -- a tenth of it is used at 30x --, their pinned host copies are
    //  sized behind the walks, from what was really produced)
    ICHK(f, f->gpool.grow(((size_t)w->cap_global + 16) * 4, GROW_WALK));
    ICHK(f, f->tpool.grow(((size_t)w->cap_target + 16) * 4, GROW_WALK));
    return 0;
}

// 3. the walk's inputs go first, on its own streams (nothing there depends on the decoding yet)
int Call::stage_walk() {
    const size_t nb = blk.nb;
    if (w->select) memcpy(f->sel.h(), w->select, sel.results());
    if (n_alt > 0) {
        memcpy(f->atask.h(), w->alt_tasks, atask.chunks());
        memcpy(f->atask.h() + atask.chunks(), w->alt_chunks, atask.rec_base() - atask.chunks());
        ICHK(f, hipMemcpyAsync(f->atask.d(), f->atask.h(), atask.rec_base(), hipMemcpyHostToDevice, f->astream));
        ICHK(f, hipMemsetAsync(f->ares.d() + ares.need(), 0, nb, f->astream));
    }
    memcpy(f->wblk.h(), w->blk_coffset, nb * 8);
    memcpy(f->wblk.h() + blk.bclen(), w->blk_clen, nb * 4);
    memcpy(f->wblk.h() + blk.xcrc(), w->blk_crc, nb * 4);
    memcpy(f->wtask.h(), w->tasks, task.chunks());
    memcpy(f->wtask.h() + task.chunks(), w->chunks, task.rec_base() - task.chunks());
    ICHK(f, hipMemcpyAsync(f->wblk.d(), f->wblk.h(), blk.bytes(), hipMemcpyHostToDevice, f->wstream));
    ICHK(f, hipMemcpyAsync(f->wtask.d(), f->wtask.h(), task.bytes(), hipMemcpyHostToDevice, f->wstream));
    ICHK(f, hipMemsetAsync(f->wres.d() + res.counters(), 0, 16, f->wstream));
    if (select) ICHK(f, hipMemcpyAsync(f->sel.d(), f->sel.h(), sel.results(), hipMemcpyHostToDevice, f->wstream));
    return 0;
}

// 4. copy in, decode (in slices on two streams); copy_out: every slice's blocks go back as soon as they are decoded
int Call::enqueue_decode() {
    int32_t *h_status = f->status.h<int32_t>(), *d_status = f->status.d<int32_t>();
    // the two streams never wait for each other: each copies the offsets in for itself (both write the same values)
    for (int s = 0; s < nstreams; ++s) {
        ICHK(f, hipEventRecord(f->t0[s], f->stream[s]));
        ICHK(f, hipMemcpyAsync(d_coff, coff, ((size_t)n_blocks + 1) * sizeof(int64_t), hipMemcpyHostToDevice, f->stream[s]));
        ICHK(f, hipMemcpyAsync(d_ooff, ooff, ((size_t)n_blocks + 1) * sizeof(int64_t), hipMemcpyHostToDevice, f->stream[s]));
    }
    for (int k = 0; k < slices; ++k) {
        hipStream_t st = f->stream[k % nstreams];
        const int32_t b0 = (int32_t)((int64_t)n_blocks * k / slices), b1 = (int32_t)((int64_t)n_blocks * (k + 1) / slices);
        const size_t c_from = (size_t)coff[b0], c_to = std::min(((size_t)coff[b1] + 3) & ~(size_t)3, f->comp.cap);
        ICHK(f, hipMemcpyAsync(f->comp.d() + c_from, f->comp.h() + c_from, c_to - c_from, hipMemcpyHostToDevice, st));
        ICHK(f, hipEventRecord(f->k0[k], st));
        ICHK(f, launch_inflate(f->comp.d<const uint32_t>(), d_coff, f->d_out.d(), d_ooff, b0, b1 - b0, d_status, want_crc ? (uint32_t*)d_crc : nullptr, st));
        ICHK(f, hipEventRecord(f->k1[k], st));
        if (copy_out) ICHK(f, hipMemcpyAsync(f->h_out.h() + ooff[b0], f->d_out.d() + ooff[b0], (size_t)(ooff[b1] - ooff[b0]), hipMemcpyDeviceToHost, st));
        ICHK(f, hipMemcpyAsync(h_status + b0, d_status + b0, (size_t)(b1 - b0) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (want_crc) ICHK(f, hipMemcpyAsync(h_status + f->cap_blocks() + b0, d_crc + b0, (size_t)(b1 - b0) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    f->last_slices = slices; f->last_streams = nstreams;
    return 0;
}

// 5. the walks follow the last slice on streams of their own, and their results come back
int Call::enqueue_walk() {
    // the walk reads every slice's blocks: its stream waits for the last launch of both decode streams
    for (int s = 0; s < nstreams; ++s) {
        ICHK(f, hipEventRecord(f->decoded[s], f->stream[s]));
        ICHK(f, hipStreamWaitEvent(f->wstream, f->decoded[s], 0));
        ICHK(f, hipStreamWaitEvent(f->astream, f->decoded[s], 0));
    }
    WalkView v;
    v.out = f->d_out.d(); v.ooff = d_ooff; v.bstatus = f->status.d<int32_t>(); v.bcrc = (const uint32_t*)d_crc;
    v.bcoff = f->wblk.d<const int64_t>(); v.bclen = part<const int32_t>(f->wblk.d(), blk.bclen()); v.xcrc = part<const uint32_t>(f->wblk.d(), blk.xcrc());
    v.out_end = ooff[n_blocks] + 48;                   // (the buffers hold 64 bytes more than reserved)
    const tredgpu_walk_task* d_tasks = f->wtask.d<const tredgpu_walk_task>();
    const tredgpu_walk_chunk* d_chunks = part<const tredgpu_walk_chunk>(f->wtask.d(), task.chunks());
    const int64_t* d_rec_base = part<const int64_t>(f->wtask.d(), task.rec_base());
    WalkRec* recs = f->wrecs.d<WalkRec>(); WalkFields* fields = f->wfields.d<WalkFields>(); WalkChained* chained = f->wchained.d<WalkChained>();
    ICHK(f, hipEventRecord(f->w0, f->wstream));
    if (n_tasks > 0) {
        // the small table when every region is short (plan_walk)
        const int table_cap = plan.large_table ? WALK_PAIR_CAP : WALK_PAIR_CAP_SMALL;
        if (!f->big_lds_allowed) {                 // (per inflater: each lives on one device, and a process may use several)
            ICHK(f, allow_pair_walk_lds());
            f->big_lds_allowed = true;
        }
        f->walk_table_cap = table_cap; f->last_walk_tasks = n_tasks;
        ICHK(f, launch_walk_chain_par(v, d_tasks, d_chunks, d_rec_base, recs, chained, (int)n_tasks, f->wstream));
        if (getenv("TREDGPU_WALK_SERIAL") != nullptr)       // (A/B and tests: every region through the serial chain)
            ICHK(f, hipMemsetAsync(chained, 0, n_tasks * sizeof(WalkChained), f->wstream));
        ICHK(f, launch_walk_chain(v, d_tasks, d_chunks, d_rec_base, recs, chained, (int)n_tasks, f->wstream));
        ICHK(f, launch_walk_parse(v, (int)n_tasks, d_rec_base, recs, chained, fields, plan.total_recs, f->wstream));
        ICHK(f, launch_pair_walk(v, d_tasks, d_rec_base, recs, fields, chained, f->wres.d<tredgpu_walk_result>(), f->wpairs.d<WalkPair>(),
                                 f->gpool.d<int32_t>(), w->cap_global, f->tpool.d<int32_t>(), w->cap_target,
                                 part<unsigned long long>(f->wres.d(), res.counters()), table_cap, (int)n_tasks, f->wstream));
    }
    if (!select) ICHK(f, hipEventRecord(f->w1, f->wstream));
    f->walk_timed = true;
    ICHK(f, hipMemcpyAsync(f->wres.h(), f->wres.d(), res.bytes(), hipMemcpyDeviceToHost, f->wstream));
    // the alternative loci's walks on a stream of their own, beside the pair walks: 480 pair-walk wavefronts leave half
    // of the SIMDs without one, and one after the other the two launches were 4.1 + 1.9 ms of every call
    // (also wblk / the walk view they read: copied in on wstream -- astream waits for that copy below)
    if (n_alt > 0) {
        ICHK(f, hipStreamWaitEvent(f->astream, f->w0, 0));
        ICHK(f, launch_alt_walk(v, f->atask.d<const tredgpu_walk_task>(), part<const tredgpu_walk_chunk>(f->atask.d(), atask.chunks()),
                                f->ares.d<tredgpu_alt_result>(), f->ares.d() + ares.need(), (int)n_alt, f->astream));
        ICHK(f, hipEventRecord(f->aready, f->astream));
        ICHK(f, hipMemcpyAsync(f->ares.h(), f->ares.d(), ares.bytes(), hipMemcpyDeviceToHost, f->astream));
    }
    ICHK(f, hipEventRecord(f->adone, f->astream));
    if (select) {
        // the selection reads the pair walk's record lists (this stream) and the alternative loci's hits (the other one)
        if (n_alt > 0) ICHK(f, hipStreamWaitEvent(f->wstream, f->aready, 0));
        tredgpu_select_result* d_selres = part<tredgpu_select_result>(f->sel.d(), sel.results());
        ICHK(f, launch_select(v, d_tasks, f->sel.d<const tredgpu_select_task>(), d_rec_base, recs, fields, chained, f->wres.d<const tredgpu_walk_result>(),
                              f->atask.d<const tredgpu_walk_task>(), f->ares.d<const tredgpu_alt_result>(), (int)n_alt, f->sel_list.d<int64_t>(), d_selres,
                              (int)n_tasks, f->wstream));
        ICHK(f, hipEventRecord(f->w1, f->wstream));
        ICHK(f, hipMemcpyAsync(f->sel.h() + sel.results(), d_selres, sel.bytes() - sel.results(), hipMemcpyDeviceToHost, f->wstream));
    }
    ICHK(f, hipEventRecord(f->wdone, f->wstream));
    return 0;
}

// 6. the waits; status / crc, the walks' results, and a second trip for the pools (sized from what was really produced)
int Call::collect(CallTrace& tr) {
    for (int s = 0; s < nstreams; ++s)
        if (wait_asleep(f, f->done[s])) return -10;
    tr.mark("decoded");
    const int32_t* h_status = f->status.h<int32_t>();
    int bad = 0;
    for (int32_t k = 0; k < n_blocks; ++k) { status[k] = h_status[k]; bad += status[k] != 0; }
    if (crc) for (int32_t k = 0; k < n_blocks; ++k) crc[k] = (uint32_t)h_status[f->cap_blocks() + k];
    if (!w) return bad;
    if (wait_asleep(f, f->wdone)) return -10;
    tr.mark("pair_walk");
    if (wait_asleep(f, f->adone)) return -10;
    tr.mark("alt_walk");
    unsigned long long used[2];
    memcpy(used, f->wres.h() + res.counters(), 16);
    memcpy(w->results, f->wres.h(), res.counters());
    if (select) {
        memcpy(w->selected, f->sel.h() + sel.results(), sel.bytes() - sel.results());
        f->sel_tasks = (int)n_tasks;
    }
    if (n_alt > 0) {
        memcpy(w->alt_results, f->ares.h(), ares.need());
        memcpy(w->need, f->ares.h() + ares.need(), ares.nb);
    }
    // (a task that found its pool full took its room all the same: the counters can exceed the capacities)
    const size_t ng = (size_t)std::min<unsigned long long>(used[0], (unsigned long long)w->cap_global),
                 nt = (size_t)std::min<unsigned long long>(used[1], (unsigned long long)w->cap_target);
    ICHK(f, f->h_gpool.grow((ng + 16) * 4, GROW_HOST_POOLS));
    ICHK(f, f->h_tpool.grow((nt + 16) * 4, GROW_HOST_POOLS));
    if (ng) ICHK(f, hipMemcpyAsync(f->h_gpool.h(), f->gpool.d(), ng * 4, hipMemcpyDeviceToHost, f->wstream));
    if (nt) ICHK(f, hipMemcpyAsync(f->h_tpool.h(), f->tpool.d(), nt * 4, hipMemcpyDeviceToHost, f->wstream));
    ICHK(f, hipEventRecord(f->wdone, f->wstream));
    if (wait_asleep(f, f->wdone)) return -10;
    if (ng) memcpy(w->global_pool, f->h_gpool.h(), ng * 4);
    if (nt) memcpy(w->target_pool, f->h_tpool.h(), nt * 4);
    w->n_global = (int64_t)ng; w->n_target = (int64_t)nt;
    tr.mark("pools");
    return bad;
}

// the copy engines: every run from its place in the decoder's output to host + host_off[its first block], on the two streams in turn
int copy_runs(tredgpu_inflater* f, const std::vector<Run>& runs, const int64_t* ooff, uint8_t* host, const int64_t* host_off, CallTrace* tr) {
    int copies = 0;
    for (const Run& r : runs) {
        ICHK(f, hipMemcpyAsync(host + host_off[r.first], f->d_out.d() + ooff[r.first], (size_t)(ooff[r.last + 1] - ooff[r.first]), hipMemcpyDeviceToHost, f->stream[copies & 1]));
        ++copies;
    }
    if (tr) tr->mark("enqueued");
    for (int s = 0; s < 2; ++s) {
        ICHK(f, hipEventRecord(f->done[s], f->stream[s]));
        if (wait_asleep(f, f->done[s])) return -10;
    }
    return copies;
}

// w != nullptr: tredgpu_inflate_walk
int run_inflate(tredgpu_inflater* f, int32_t n_blocks, int32_t* status, uint32_t* crc, bool copy_out, tredgpu_walk_args* w) {
    if (!f) return -2;
    if (n_blocks < 0 || (size_t)n_blocks + 1 > f->cap_blocks() || (n_blocks > 0 && !status)) return ifail(f, -2, "bad arguments (reserve first)");
    if (n_blocks == 0) return 0;
    if (copy_out && !f->h_out.h()) return ifail(f, -2, "this inflater keeps no host copy of the output (tredgpu_inflater_host_out): walk and fetch");
    CallTrace tr(w ? "inflate_walk" : "inflate");
    Call c{f, n_blocks, status, crc, copy_out, w};
    int rc = c.check();
    if (rc) return rc;
    ICHK(f, hipSetDevice(f->device));
    if (w && ((rc = c.grow_walk()) || (rc = c.stage_walk()))) return rc;
    tr.mark("walk_inputs");
    if ((rc = c.enqueue_decode())) return rc;
    f->walk_timed = false;
    if (!w) f->sel_tasks = 0;                      // (the output a selection pointed into is being overwritten)
    if (w && (rc = c.enqueue_walk())) return rc;
    for (int s = 0; s < c.nstreams; ++s) {
        ICHK(f, hipEventRecord(f->t1[s], f->stream[s]));
        ICHK(f, hipEventRecord(f->done[s], f->stream[s]));
    }
    tr.mark("enqueued");
    return c.collect(tr);
}
}  // namespace

extern "C" {

int tredgpu_inflate_blocks_crc(tredgpu_inflater* f, int32_t n_blocks, int32_t* status, uint32_t* crc) {
    return run_inflate(f, n_blocks, status, crc, true, nullptr);
}

int tredgpu_inflate_walk(tredgpu_inflater* f, int32_t n_blocks, int32_t* status, uint32_t* crc, tredgpu_walk_args* walk) {
    if (!walk) return f ? ifail(f, -2, "walk is NULL") : -2;
    return run_inflate(f, n_blocks, status, crc, false, walk);
}

// The blocks with need[k] != 0 of the last tredgpu_inflate_walk, copied to their places in the pinned output (runs of
// wanted blocks, and the unwanted ones between two runs when they are few, go in one copy).
int tredgpu_inflater_fetch(tredgpu_inflater* f, int32_t n_blocks, const uint8_t* need) {
    if (!f) return -2;
    if (n_blocks < 0 || (size_t)n_blocks + 1 > f->cap_blocks() || (n_blocks > 0 && !need)) return ifail(f, -2, "bad arguments");
    if (n_blocks == 0) return 0;
    if (!f->h_out.h()) return ifail(f, -2, "this inflater keeps no host copy of the output: tredgpu_inflater_fetch_dense");
    const int64_t* ooff = f->h_ooff();
    ICHK(f, hipSetDevice(f->device));
    return copy_runs(f, wanted_runs(need, ooff, n_blocks, FETCH_GAP), ooff, f->h_out.h(), ooff, nullptr);
}

int tredgpu_inflate_blocks(tredgpu_inflater* f, int32_t n_blocks, int32_t* status) { return tredgpu_inflate_blocks_crc(f, n_blocks, status, nullptr); }

int tredgpu_inflater_timing(tredgpu_inflater* f, double* total_ms, double* kernel_ms) {
    if (!f || !total_ms || !kernel_ms) return -2;
    *total_ms = *kernel_ms = 0.0;
    if (f->last_slices == 0) return 0;
    ICHK(f, hipSetDevice(f->device));
    float ms = 0.f;
    for (int s = 0; s < f->last_streams; ++s) {
        ICHK(f, hipEventElapsedTime(&ms, f->t0[0], f->t1[s]));
        *total_ms = std::max(*total_ms, (double)ms);
    }
    for (int k = 0; k < f->last_slices; ++k) {
        if (hipEventElapsedTime(&ms, f->k0[k], f->k1[k]) == hipSuccess) *kernel_ms += ms;
    }
    return 0;
}

int tredgpu_inflater_host_out(tredgpu_inflater* f, int enabled) {
    if (!f) return -2;
    if ((enabled != 0) != f->host_out) {
        ICHK(f, hipSetDevice(f->device));
        for (hipStream_t st : f->stream) ICHK(f, hipStreamSynchronize(st));
        release(f->decode_bufs);                       // (the next reserve allocates what the new mode needs)
        f->host_out = enabled != 0;
    }
    return 0;
}

int tredgpu_inflater_fetch_dense(tredgpu_inflater* f, int32_t n_blocks, const uint8_t* need, uint8_t** host, int64_t* dense_off) {
    if (!f) return -2;
    if (n_blocks < 0 || (size_t)n_blocks + 1 > f->cap_blocks() || !host || !dense_off || (n_blocks > 0 && !need)) return ifail(f, -2, "bad arguments");
    CallTrace tr("fetch_dense");
    const int64_t* ooff = f->h_ooff();
    const std::vector<Run> runs = wanted_runs(need, ooff, n_blocks, FETCH_GAP);
    const int64_t total = dense_offsets(runs, ooff, n_blocks, dense_off);
    ICHK(f, hipSetDevice(f->device));
    ICHK(f, f->dense.grow((size_t)total + PAD, GROW_DENSE));
    tr.mark("room");
    *host = f->dense.h();
    int copies = 0;
    static const bool by_dma = getenv("TREDGPU_FETCH_DMA") != nullptr;     // (A/B: the copy engines, one copy per run)
    if (by_dma) {
        if ((copies = copy_runs(f, runs, ooff, f->dense.h(), dense_off, &tr)) < 0) return copies;
    } else if (!runs.empty()) {
        constexpr int64_t PIECE = 32 * 1024;       // bytes per workgroup: ~3 300 workgroups for a 16-sample call
        size_t n_pieces = 0;
        for (const Run& r : runs) n_pieces += (size_t)((ooff[r.last + 1] - ooff[r.first] + PIECE - 1) / PIECE);
        ICHK(f, f->pieces.grow(n_pieces, GROW_LISTS));
        FetchPiece* P = f->pieces.h<FetchPiece>();
        size_t p = 0;
        for (const Run& r : runs) {
            const int64_t bytes = ooff[r.last + 1] - ooff[r.first];
            for (int64_t o = 0; o < bytes; o += PIECE) P[p++] = FetchPiece{ooff[r.first] + o, dense_off[r.first] + o, (int32_t)std::min(PIECE, bytes - o), 0};
        }
        ICHK(f, hipMemcpyAsync(f->pieces.d(), P, n_pieces * sizeof(FetchPiece), hipMemcpyHostToDevice, f->stream[0]));
        ICHK(f, launch_fetch_gather(f->d_out.d(), f->dense.h(), f->pieces.d<const FetchPiece>(), n_pieces, f->stream[0]));
        copies = (int)n_pieces;
        tr.mark("enqueued");
        ICHK(f, hipEventRecord(f->done[0], f->stream[0]));
        if (wait_asleep(f, f->done[0])) return -10;
    }
    tr.mark("copied");
    if (tr.on) { char b[64]; snprintf(b, sizeof b, " copies=%d MB=%.1f", copies, total / 1e6); tr.line += b; }
    return copies;
}

int64_t tredgpu_inflater_pinned_bytes(const tredgpu_inflater* f) {
    if (!f) return -2;
    size_t n = 0;
    for (const std::vector<Buf*>* set : {&f->decode_bufs, &f->walk_bufs}) for (const Buf* b : *set) n += b->pinned_bytes();
    return (int64_t)n;
}

int64_t tredgpu_inflater_walk_serial_regions(tredgpu_inflater* f) {
    if (!f) return -2;
    if (f->last_walk_tasks == 0 || !f->wchained.d()) return 0;
    ICHK(f, hipSetDevice(f->device));
    std::vector<WalkChained> c(f->last_walk_tasks);
    ICHK(f, hipMemcpy(c.data(), f->wchained.d(), c.size() * sizeof(WalkChained), hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (const WalkChained& w : c) n += w.mode == 0;
    if (getenv("TREDGPU_TRACE") != nullptr)
        for (size_t t = 0; t < c.size(); ++t)
            if (c[t].mode == 0) fprintf(stderr, "tredgpu: region %zu chained serially (reason %d), %d records, status %d\n", t, c[t].pad, c[t].n, c[t].status);
    return n;
}

int tredgpu_inflater_walk_ms(tredgpu_inflater* f, double* walk_ms) {
    if (!f || !walk_ms) return -2;
    *walk_ms = 0.0;
    if (!f->walk_timed) return 0;
    ICHK(f, hipSetDevice(f->device));
    float ms = 0.f;
    ICHK(f, hipEventElapsedTime(&ms, f->w0, f->w1));
    *walk_ms = ms;
    return 0;
}

}  // extern "C"

// what tredgpu_genotype_selected (capi.hip) reads of an inflater: the decoder's output, the selected records' places and the
// host copy of the select results of its last walk
int tredgpu_front::inflater_selected(tredgpu_inflater* f, SelectedView* view) {
    if (!f || !view) return -2;
    if (f->sel_tasks <= 0 || !f->sel_list.d() || !f->d_out.d()) return ifail(f, -2, "the inflater's last call carried no read selection");
    view->device = f->device;
    view->out = f->d_out.d();
    view->sel_list = f->sel_list.d<int64_t>();
    view->n_tasks = f->sel_tasks;
    view->results = part<const tredgpu_select_result>(f->sel.h(), SelectTable{(size_t)f->sel_tasks}.results());
    return 0;
}
