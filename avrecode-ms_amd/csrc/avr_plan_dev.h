// The plan of a device-resident batch made ON the device (avr_plan_dev.hip): what fill_plan and plan_tiles of avr_plan.h make on the
// host from lengths in host memory, from lengths that lie in HBM -- and the way back, a batch's coded bytes compacted from their
// worst-case regions without the lengths leaving the device.  The per-slice rules are avr_plan.h's own functions.
//
// This header holds what the host needs without a device: the bounds, and where everything lies in the one workspace the three calls
// share (avr_plan_workspace_bytes quotes the largest of the three layouts; the launchers carve by the same structs, as avr_layout.h
// does it).  Plain C++17 up to the launchers' declarations, which need hipStream_t.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "avr_layout.h"

namespace avr {
namespace plan_dev {

constexpr uint32_t kScanTile = 1024;                             // entries a workgroup of the scan takes: 256 threads, four each
constexpr uint32_t kSortTile = 256;                              // keys a workgroup of the sort ranks at a time: one per thread
constexpr uint32_t kSortBlocks = 1024;                           // workgroups of the sort at most; each takes a run of whole tiles
constexpr uint32_t kSortDigits = 256;                            // eight bits a pass, four passes

// The scan is reduce per workgroup, scan of the workgroups' sums, apply: level j holds one sum per workgroup of level j - 1 (level 0:
// of the entries themselves), and the last level fits one workgroup.  No entries above one workgroup's: no level.  2^31 entries: 3.
struct ScanLevels {
    uint32_t count = 0;
    uint64_t n[4] = {0, 0, 0, 0};                                // sums at level j
    uint64_t off[4] = {0, 0, 0, 0};                              // bytes from the region's start
    uint64_t bytes = 0;
};
inline ScanLevels scan_levels(uint64_t n_entries, uint32_t sum_bytes) {
    ScanLevels L;
    Cursor c;
    uint64_t m = (n_entries + kScanTile - 1) / kScanTile;
    while (m > 1 && L.count < 4) {
        L.n[L.count] = m;
        L.off[L.count] = c.take(m * sum_bytes);
        L.count++;
        if (m <= kScanTile) break;
        m = (m + kScanTile - 1) / kScanTile;
    }
    L.bytes = c.at;
    return L;
}

constexpr uint32_t kPlanSums = 7;                                // out, records, chunks, digit sums, work bytes, blocks, bins: 64 bits each

// avr_plan_chunks_device: a copy of the totals for the expansion kernels (the caller's may be host memory), then the scan's sums
struct ChunksLayout { uint64_t totals, sums, total; };
inline ChunksLayout chunks_layout(size_t n_slices) {
    ChunksLayout L;
    Cursor c;
    L.totals = c.take(sizeof(avr_plan_totals));
    L.sums = c.take(scan_levels(n_slices, kPlanSums * 8).bytes);
    L.total = c.at;
    return L;
}

// How the sort deals its keys out: `blocks` workgroups, each `per_block` consecutive keys (whole tiles) in tile order.
struct SortShape { uint32_t blocks, per_block; };
inline SortShape sort_shape(size_t n_slices) {
    const uint64_t tiles = (uint64_t(n_slices) + kSortTile - 1) / kSortTile;
    SortShape s;
    s.blocks = uint32_t(tiles < kSortBlocks ? (tiles ? tiles : 1) : kSortBlocks);
    s.per_block = uint32_t((tiles + s.blocks - 1) / s.blocks * kSortTile);
    return s;
}

// avr_plan_tiles_device: two (key, index) buffers the passes go to and fro between, a pass's histograms [digit][workgroup] and their
// sums per 1024, the sums of the scan over the tiles
struct TilesLayout { uint64_t keys[2], vals[2], hist, hist_sums, sums, total; };
inline TilesLayout tiles_layout(size_t n_slices) {
    TilesLayout L;
    Cursor c;
    for (int i = 0; i < 2; i++) {
        L.keys[i] = c.take(uint64_t(n_slices) * 4);
        L.vals[i] = c.take(uint64_t(n_slices) * 4);
    }
    L.hist = c.take(uint64_t(kSortDigits) * sort_shape(n_slices).blocks * 4);
    L.hist_sums = c.take(uint64_t(kSortDigits) * kSortBlocks / kScanTile * 4);
    L.sums = c.take(scan_levels((uint64_t(n_slices) + 63) / 64, 8).bytes);
    L.total = c.at;
    return L;
}

// avr_compact_device: the sums of the scan over the slices' lengths
struct CompactLayout { uint64_t sums, total; };
inline CompactLayout compact_layout(size_t n_slices) {
    CompactLayout L;
    Cursor c;
    L.sums = c.take(scan_levels(n_slices, 8).bytes);
    L.total = c.at;
    return L;
}

// avr_finish_device: the slices' final lengths (64 bits each, pass 1 writes them, the scan reads them), then the scan's sums.  A quote
// of its own (avr_finish_workspace_bytes): avr_plan_workspace_bytes stays what it was.
struct FinishLayout { uint64_t lens, sums, total; };
inline FinishLayout finish_layout(size_t n_slices) {
    FinishLayout L;
    Cursor c;
    L.lens = c.take(uint64_t(n_slices) * 8);
    L.sums = c.take(scan_levels(n_slices, 8).bytes);
    L.total = std::max<uint64_t>(c.at, 256);
    return L;
}

inline uint64_t workspace_bytes(size_t n_slices) {
    return std::max(std::max(chunks_layout(n_slices).total, tiles_layout(n_slices).total), std::max<uint64_t>(compact_layout(n_slices).total, 256));
}

inline void bounds(size_t n_slices, uint64_t max_total_bins, uint64_t *cap_chunks, uint64_t *cap_blocks) {
    if (cap_chunks) *cap_chunks = max_total_bins / kChunk + n_slices;               // a slice has at most n_bins / kChunk + 1 chunks, an empty one has one
    if (cap_blocks) *cap_blocks = max_total_bins / kSortBlock + n_slices;
}

}  // namespace plan_dev

#if defined(__HIPCC__)
// Everything is enqueued on `s`; nothing waits, allocates or runs on another stream.  `ws`: workspace_bytes(n_slices), 256-byte aligned.
hipError_t launch_plan_chunks(hipStream_t s, const uint32_t *n_bins, uint32_t n_slices, int level, const avr_plan_arrays &arrays, void *ws,
                              avr_plan_totals *totals);
hipError_t launch_plan_tiles(hipStream_t s, const uint32_t *n_bins, uint32_t n_slices, uint32_t records_per_chunk, uint32_t *order,
                             uint64_t *tile_off, void *ws, avr_plan_totals *totals);
hipError_t launch_compact_wide(hipStream_t s, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, uint32_t n_slices,
                               uint8_t *dense, uint64_t dense_capacity, uint64_t *dense_off, void *ws);
// `ws`: finish_layout(n_slices).total bytes; status: null or n_slices words; finish: n_slices words (AVR_FINISH_WORD)
hipError_t launch_finish(hipStream_t s, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, const int32_t *status,
                         uint32_t n_slices, const uint32_t *finish, uint8_t *dense, uint64_t dense_capacity, uint64_t *dense_off, void *ws);
#endif

}  // namespace avr
