// What a batch's slice lengths decide before anything is laid out (csrc/avr_layout.h takes these as its inputs): the arrays of an
// avr_chunk_plan, the slices' output regions, the tiles, and whether the batch goes through the intra-slice parallel kernels.  Each rule is
// written ONCE here; the kernels index chunk_slice[], res_off[] and dig_off[] unchecked, so these rules keep them inside their
// buffers.  Python twin: chunk_plan_arrays() in avrecode-ms_amd/device.py; tests/test_plan.py holds the two to each other and to
// recorded numbers.  Plain C++17, no HIP header: tests/plan_check.cpp compiles it alone.  The per-slice rules are `__host__ __device__`
// under hipcc, in the way avr_div.h is: the device planner (avr_plan_dev.hip) applies the very functions fill_plan applies.
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>

#include "avr_layout.h"

#if defined(__HIPCC__)
#define AVR_PLAN_HD __host__ __device__ inline
#else
#define AVR_PLAN_HD inline
#endif

namespace avr {

// ------------------------------------------------------------------ per slice of nb bins
AVR_PLAN_HD uint32_t slice_chunks(uint64_t nb) { return nb ? uint32_t((nb + kChunk - 1) / kChunk) : 1u; }            // an empty slice has one
AVR_PLAN_HD uint32_t slice_blocks(uint64_t nb) { return nb ? uint32_t((nb + kSortBlock - 1) / kSortBlock) : 1u; }    // census blocks
AVR_PLAN_HD uint64_t slice_work_bytes(uint64_t nb) { return ((nb + 15) & ~uint64_t(15)) + 16; }   // per-bin work arrays: whole 16-byte groups and one more
AVR_PLAN_HD uint64_t slice_digit_sums(uint64_t nb) { return nb / 2 + 8; }
AVR_PLAN_HD uint64_t slice_out_bytes(uint64_t nb) { return (nb + 16 + 7) & ~uint64_t(7); }        // worst case 8 bits per bin for either coder ("output sizing") + stop bytes

// Which arrays a path reads; each level needs those of the levels before it.
//   Serial   one lane per slice: out_off
//   Chunks   K2p, the estimator resolver: + chunk_base, chunk_slice
//   Codes    K1p from resolved codes: + dig_off
//   K1p      the whole of K1p: + res_off, blk_base, blk_slice
enum class PlanFor { Serial, Chunks, Codes, K1p };

// Exclusive prefix sums over the slices with the total appended (n + 1 entries), and per chunk / block the slice it belongs to.
// An array the path does not read is left empty.
struct HostPlan {
    std::vector<uint64_t> out_off, res_off, dig_off;
    std::vector<uint32_t> chunk_base, chunk_slice, blk_base, blk_slice;
    // bytes of the arrays a caller copies to the device as a plan (out_off goes its own way)
    size_t staged_bytes() const { return 8 * (res_off.size() + dig_off.size()) + 4 * (chunk_base.size() + chunk_slice.size() + blk_base.size() + blk_slice.size()); }
};
// the total a prefix-sum array ends in; 0 for an array the path left empty
template <class T>
inline T plan_total(const std::vector<T> &off) { return off.empty() ? 0 : off.back(); }

inline void fill_plan(HostPlan &p, const uint32_t *n_bins, size_t n, PlanFor path) {
    p.out_off.assign(n + 1, 0);
    p.chunk_base.assign(path >= PlanFor::Chunks ? n + 1 : 0, 0);
    p.dig_off.assign(path >= PlanFor::Codes ? n + 1 : 0, 0);
    p.res_off.assign(path >= PlanFor::K1p ? n + 1 : 0, 0);
    p.blk_base.assign(path >= PlanFor::K1p ? n + 1 : 0, 0);
    p.chunk_slice.clear();
    p.blk_slice.clear();
    for (size_t i = 0; i < n; i++) {
        const uint64_t nb = n_bins[i];
        p.out_off[i + 1] = p.out_off[i] + slice_out_bytes(nb);
        if (p.chunk_base.empty()) continue;
        const uint32_t nc = slice_chunks(nb);
        p.chunk_base[i + 1] = p.chunk_base[i] + nc;
        p.chunk_slice.insert(p.chunk_slice.end(), nc, uint32_t(i));
        if (p.dig_off.empty()) continue;
        p.dig_off[i + 1] = p.dig_off[i] + slice_digit_sums(nb);
        if (p.res_off.empty()) continue;
        const uint32_t nk = slice_blocks(nb);
        p.res_off[i + 1] = p.res_off[i] + slice_work_bytes(nb);
        p.blk_base[i + 1] = p.blk_base[i] + nk;
        p.blk_slice.insert(p.blk_slice.end(), nk, uint32_t(i));
    }
}

// The tiles of the one-lane-per-slice paths: slices are processed longest first (stable: equal lengths keep the caller's order), 64 to
// a tile, and a tile is as long as its first -- its longest -- slice.  tile_off: n_tiles + 1 offsets in 16-byte chunks.
// records_per_chunk: 8 for two-byte records, 16 for one-byte tiles (k_pack_tiles8_narrow).  Python twin: plan_tiles() in
// avrecode-ms_amd/device.py; tests/test_plan.py holds the two to each other.  (static: the sort's instantiations stay out of the
// library's exported symbols.)
static inline void plan_tiles(const std::vector<uint32_t> &n_bins, std::vector<uint32_t> &order, std::vector<uint64_t> &tile_off,
                              uint32_t records_per_chunk = 8) {
    const size_t n = n_bins.size();
    order.resize(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return n_bins[a] > n_bins[b]; });
    const size_t n_tiles = (n + 63) / 64;
    tile_off.assign(n_tiles + 1, 0);
    for (size_t t = 0; t < n_tiles; t++) {
        const uint64_t chunks = (uint64_t(n_bins[order[t * 64]]) + records_per_chunk - 1) / records_per_chunk;   // sorted: first lane is the longest
        tile_off[t + 1] = tile_off[t] + chunks * 64;
    }
}

// One lane per slice needs tens of thousands of slices to fill the chip; a batch of few, long slices (a clip with one slice per
// frame) goes through the intra-slice parallel kernels.  (The AVR_K1_PATH override is the caller's.)
inline bool want_chunked(size_t n_slices, uint64_t total_bins) { return n_slices > 0 && n_slices <= 32768 && total_bins / n_slices >= 8192; }

// a workspace pointer as the launchers want it: callers allocate 256 bytes more than a layout's total
template <class T>
inline T *align256(T *p) { return reinterpret_cast<T *>(uintptr_t(align256(uint64_t(reinterpret_cast<uintptr_t>(p))))); }

}  // namespace avr
