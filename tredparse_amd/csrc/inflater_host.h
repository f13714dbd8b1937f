// inflater_host.h -- the host arithmetic of inflater_api.hip, free of HIP (tests/inflater_host_main.cpp runs it under the
// sanitizers): how buffers grow, what a call's offsets / tasks / chunks must satisfy, the record room and the name table
// of a walk, the runs a fetch copies, and where the parts of the packed arrays lie.
#ifndef TREDGPU_INFLATER_HOST_H
#define TREDGPU_INFLATER_HOST_H

#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/tredgpu.h"

namespace inflater_host {

// ---- growth: a buffer that is too small becomes need + need / past_need or cap + cap / past_cap, whichever is more (0: no slack) --
struct Slack { size_t past_need, past_cap; };
inline size_t next_cap(size_t need, size_t cap, size_t past_need, size_t past_cap) {
    return std::max(need + (past_need ? need / past_need : 0), cap + (past_cap ? cap / past_cap : 0));
}
inline size_t next_cap(size_t need, size_t cap, Slack s) { return next_cap(need, cap, s.past_need, s.past_cap); }
// (page-locked staging grows by an eighth past the largest call seen, and a sixteenth past the call that makes it grow:
//  a chunk's size varies by a few per cent -- sized exactly, the second and the third chunk of a driver each freed and
//  page-locked 0.3 GB again, 0.3-0.4 s of a cohort's first two seconds --, and every spare byte here is pinned three times
//  per driver process)
constexpr Slack GROW_STAGING = {16, 8};     // comp, out
constexpr Slack GROW_BLOCKS = {16, 2};      // the offsets and the status / crc per block
constexpr Slack GROW_WALK = {8, 2};         // the walk's tables and lists, the pools on the device (the call's BOUND)
constexpr Slack GROW_LISTS = {0, 2};        // the selection's record places, the fetch kernel's pieces
constexpr Slack GROW_HOST_POOLS = {8, 8};   // the pinned pools: what the walks really produced, an eighth more
constexpr Slack GROW_DENSE = {0, 8};        // the fetched blocks
constexpr size_t PAD = 64;                  // bytes every packed array is given beyond its parts

// ---- what a call must satisfy (nullptr, or the refusal's text) ----------------------------------------------------------
inline const char* check_blocks(const int64_t* coff, const int64_t* ooff, int32_t n_blocks, size_t cap_comp, size_t cap_out) {
    for (int32_t k = 0; k < n_blocks; ++k)
        if (coff[k] < 0 || (coff[k] & 3) != 0 || coff[k + 1] < coff[k] || ooff[k] < 0 || ooff[k + 1] < ooff[k] || ooff[k + 1] - ooff[k] > 65536)
            return "block offsets: payloads start on 4-byte boundaries, ascend, and inflate to at most 64 KiB each";
    if ((size_t)coff[n_blocks] + 64 > cap_comp || (size_t)ooff[n_blocks] + 64 > cap_out) return "offsets beyond the reserved buffers";
    return nullptr;
}
inline const char* check_tasks(const tredgpu_walk_task* tasks, size_t n_tasks, size_t n_chunks, int32_t n_blocks) {
    for (size_t t = 0; t < n_tasks; ++t) {
        const tredgpu_walk_task& T = tasks[t];         // (n_chunks < 0: not planned, nothing of it is read)
        if (T.n_chunks >= 0 && (T.chunk_first < 0 || (size_t)T.chunk_first + (size_t)T.n_chunks > n_chunks || T.block_first < 0 ||
                                T.block_end > n_blocks || T.block_first > T.block_end))
            return "walk task outside its chunks / blocks";
    }
    return nullptr;
}
inline const char* check_chunks(const tredgpu_walk_chunk* chunks, size_t n_chunks) {
    for (size_t q = 0; q < n_chunks; ++q)
        if (chunks[q].begin_upos < 0 || chunks[q].begin_upos > 65536) return "walk chunk starts outside a block";
    return nullptr;
}

// ---- the walk's plan ------------------------------------------------------------------------------------------------------
// the blocks a task's chunks span (a task's block_first .. block_end is its whole FILE), and their inflated bytes
struct Span { int64_t blocks, bytes; };
inline Span chunk_span(const tredgpu_walk_task& T, const tredgpu_walk_chunk* chunks, const int64_t* blk_coffset, const int64_t* ooff) {
    Span s = {0, 0};
    for (int32_t q = 0; q < T.n_chunks; ++q) {
        const tredgpu_walk_chunk& ch = chunks[T.chunk_first + q];
        if (ch.begin_block < T.block_first || ch.begin_block >= T.block_end) continue;
        const int64_t* lo = blk_coffset + ch.begin_block;
        const int64_t* hi = std::upper_bound(lo, blk_coffset + T.block_end, (int64_t)(ch.end_voffset >> 16));
        s.blocks += hi - lo;
        s.bytes += ooff[ch.begin_block + (hi - lo)] - ooff[ch.begin_block];
    }
    return s;
}
// rec_base[n_tasks + 1]: room for every region's record list, at no less than 64 bytes per record (36 fixed bytes, a name,
// 36 bases and their qualities: 100 and more) -- a region that has more records than that is the host's (status 4).
// large_table: some region spans more than 40 blocks; up to there (2.6 MB of records, ~8 000 of them) a region has at most
// ~4 000 names, and one that has more after all is handed back to the host (status 4)
struct WalkPlan { size_t total_recs; bool large_table; };
inline WalkPlan plan_walk(const tredgpu_walk_task* tasks, size_t n_tasks, const tredgpu_walk_chunk* chunks, const int64_t* blk_coffset,
                          const int64_t* ooff, int64_t* rec_base) {
    WalkPlan p = {0, false};
    rec_base[0] = 0;
    for (size_t t = 0; t < n_tasks; ++t) {
        const Span s = chunk_span(tasks[t], chunks, blk_coffset, ooff);
        rec_base[t + 1] = rec_base[t] + (tasks[t].n_chunks > 0 ? s.bytes / 64 + 64 : 0);
        p.large_table |= s.blocks > 40;
    }
    p.total_recs = (size_t)rec_base[n_tasks];
    return p;
}

// ---- the runs a fetch copies: a wanted block, and on to the next wanted one while the blocks in between are no more than gap bytes --
constexpr int64_t FETCH_GAP = 128 * 1024;        // a copy costs the host ~5 us: less than these bytes cost the bus
struct Run { int32_t first, last; };             // blocks [first, last]
inline std::vector<Run> wanted_runs(const uint8_t* need, const int64_t* ooff, int32_t n_blocks, int64_t gap) {
    std::vector<Run> runs;
    for (int32_t k = 0; k < n_blocks;) {
        if (!need[k]) { ++k; continue; }
        int32_t last = k;
        for (int32_t j = k + 1; j < n_blocks && ooff[j] - ooff[last + 1] <= gap; ++j)
            if (need[j]) last = j;
        runs.push_back(Run{k, last});
        k = last + 1;
    }
    return runs;
}
// dense_off[n_blocks + 1]: the runs' blocks one after the other (a block outside every run is empty); returns their bytes
inline int64_t dense_offsets(const std::vector<Run>& runs, const int64_t* ooff, int32_t n_blocks, int64_t* dense_off) {
    int64_t total = 0;
    int32_t k = 0;
    dense_off[0] = 0;
    for (const Run& r : runs) {
        for (; k < r.first; ++k) dense_off[k + 1] = total;
        for (; k <= r.last; ++k) { total += ooff[k + 1] - ooff[k]; dense_off[k + 1] = total; }
    }
    for (; k < n_blocks; ++k) dense_off[k + 1] = total;
    return total;
}

// ---- the packed arrays: byte offsets of their parts, the same from the pinned base and from the device base -------------------
template <class T> T* part(uint8_t* base, size_t at) { return (T*)(base + at); }
struct BlockTable { size_t nb; size_t bclen() const { return nb * 8; } size_t xcrc() const { return nb * 12; } size_t bytes() const { return nb * 16; } };   // bcoff[nb] int64 | bclen[nb] int32 | xcrc[nb] uint32
struct TaskTable {                               // tasks | chunks | rec_base[n_tasks + 1] (the alternative loci's: tasks | chunks)
    size_t n_tasks, n_chunks;
    size_t chunks() const { return n_tasks * sizeof(tredgpu_walk_task); }
    size_t rec_base() const { return chunks() + n_chunks * sizeof(tredgpu_walk_chunk); }
    size_t bytes() const { return rec_base() + (n_tasks + 1) * sizeof(int64_t); }
};
struct ResultTable { size_t n_tasks; size_t counters() const { return n_tasks * sizeof(tredgpu_walk_result); } size_t bytes() const { return counters() + 16; } };   // results | the two pools' counters
struct AltResultTable { size_t n_alt, nb; size_t need() const { return n_alt * sizeof(tredgpu_alt_result); } size_t bytes() const { return need() + nb; } };       // the alternative loci's results | the blocks' need flags
struct SelectTable { size_t n_tasks; size_t results() const { return n_tasks * sizeof(tredgpu_select_task); } size_t bytes() const { return results() + n_tasks * sizeof(tredgpu_select_result); } };   // select tasks | their results
static_assert(sizeof(tredgpu_walk_task) % 8 == 0 && sizeof(tredgpu_walk_chunk) % 8 == 0 && sizeof(tredgpu_walk_result) % 8 == 0 && sizeof(tredgpu_select_task) % 8 == 0,
              "rec_base, the counters and the select results stay 8-byte aligned");

}  // namespace inflater_host
#endif
