// cigar_long_plan.h -- the host-side planning of sw_cigar_long.hip: how many wavefront slots a call gets, how much
// direction plane each of them owns and which items a slot takes.  Plain C++17, nothing from HIP, so that a stand-alone
// program can run it under the sanitizers (tests/cigar_long_plan_main.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace cigar_long_plan {

constexpr int SLOTS = 256;                              // wavefronts of a launch at the most (one per CU of an MI355X)
constexpr size_t WORKSPACE_CAP = (size_t)1 << 30;       // bytes of direction plane a context holds at the most
constexpr int MAX_READ = 2048, MAX_TEMPLATE = 4095;     // TREDGPU_MAX_LONG_READ_LEN / TREDGPU_MAX_LONG_TEMPLATE_LEN
constexpr size_t ALIGN = 256;

// Bytes of direction plane the rectangle of fields {score, ref_begin, ref_end, read_begin, read_end} needs: one byte per
// cell of a row's band, and a band never holds more than refLen cells, so refLen * readLen whatever the band doubles to.
// 0 for fields the kernel refuses before its first pass (a negative begin, end < begin, a rectangle beyond the limits).
inline size_t rect_bytes(const int16_t* f) {
    const long ref_begin = f[1], ref_end = f[2], read_begin = f[3], read_end = f[4];
    if (ref_begin < 0 || ref_end < ref_begin || read_begin < 0 || read_end < read_begin) return 0;
    if (ref_end >= MAX_TEMPLATE || read_end >= MAX_READ) return 0;
    return (size_t)(ref_end - ref_begin + 1) * (size_t)(read_end - read_begin + 1);
}

struct Plan {
    size_t slot_bytes = ALIGN;   // direction plane of one slot: the call's largest rectangle, rounded up to ALIGN
    int slots = 0;               // wavefronts to launch: slots * slot_bytes <= WORKSPACE_CAP
    size_t total() const { return slot_bytes * (size_t)slots; }
};

// fields: int16 [n_items][5]
inline Plan plan(const int16_t* fields, int64_t n_items) {
    Plan p;
    size_t largest = 0;
    for (int64_t k = 0; k < n_items; ++k) largest = std::max(largest, rect_bytes(fields + 5 * k));
    p.slot_bytes = std::max(ALIGN, (largest + ALIGN - 1) / ALIGN * ALIGN);
    const int64_t room = (int64_t)(WORKSPACE_CAP / p.slot_bytes);
    p.slots = (int)std::max<int64_t>(0, std::min<int64_t>({n_items, (int64_t)SLOTS, room}));
    return p;
}

// Items are taken grid-stride: slot s does items s, s + slots, s + 2 * slots, ... in that order.
inline int slot_of(int64_t item, int slots) { return (int)(item % slots); }
inline int64_t turn_of(int64_t item, int slots) { return item / slots; }

}  // namespace cigar_long_plan
