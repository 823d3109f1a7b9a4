// The chunk geometry, once: every path that cuts a slice (K1p, K2p, the estimator resolver and its checker, the planners) cuts it in
// chunks of kChunk bins, and every number that follows from that length is named here.  What the kernels ASSUME about the length is
// the list of static_asserts at the end; the ones that belong to a constant of one file (K2p's ring, the checker's span) stand next
// to that constant and say so.  Plain C++17, no HIP header: `__host__ __device__` under hipcc, in the way avr_plan.h is.
#pragma once
#include <stdint.h>

#include "../../include/avrecode_ms_amd.h"

#if defined(__HIPCC__)
#define AVR_CHUNK_HD __host__ __device__ inline
#else
#define AVR_CHUNK_HD inline
#endif

namespace avr {

// Host-only test builds may state another length (tests/test_k1p_emul.py builds the CPU emulation at 256 and 4096): nothing that
// holds device code can, the chunk plan of the C ABI and every workspace size being made for AVR_CHUNK_BINS.
#if defined(AVR_TEST_CHUNK_BINS)
#if defined(__HIPCC__)
#error "AVR_TEST_CHUNK_BINS is for host-only test builds: the kernels and the C ABI's chunk plan are made for AVR_CHUNK_BINS"
#endif
constexpr uint32_t kChunk = AVR_TEST_CHUNK_BINS;
#else
constexpr uint32_t kChunk = AVR_CHUNK_BINS;                      // bins per chunk: one lane of K1p's sort, replay, B1 and C
#endif
constexpr uint32_t kSortBlock = AVR_SORT_BLOCK_BINS;             // bins per block of K1p's census

constexpr uint32_t floor_log2(uint32_t x) { return x > 1 ? 1 + floor_log2(x >> 1) : 0; }
constexpr uint32_t kChunkLog2 = floor_log2(kChunk);

// ---- what a chunk takes, per form of its bins
constexpr uint32_t kChunkCodeBytes = kChunk;                     // resolved codes: a byte a bin
constexpr uint32_t kChunkCodeGroups = kChunk / 16;               // ... in 16-byte groups (the rows of a tile of TileCodes)
constexpr uint32_t kChunkRecGroups = kChunk / 8;                 // two-byte records in 16-byte groups
constexpr uint32_t kChunkBitDwords = kChunk / 32;                // the bit string of k_k1p_local: a bit a bin (lbits' stride, rows of `bits`)
constexpr uint32_t kChunkBitBytes = kChunk / 8;
constexpr uint32_t kChunkSpareRow = kChunkBitDwords;             // row of `bits` behind the string: positions from kChunk on land there
constexpr uint32_t kChunkPosMask = 2 * kChunk - 1;               // a position of k_k1p_local (one 16-bit half of a counter dword): below kChunk a place in the string, from kChunk on the spare row

// ---- which chunk holds bin i of its slice, and where in it (a length that is no power of two changes these and nothing else)
AVR_CHUNK_HD uint32_t chunk_of(uint32_t i) { return i >> kChunkLog2; }
AVR_CHUNK_HD uint32_t bin_in_chunk(uint32_t i) { return i & (kChunk - 1); }
AVR_CHUNK_HD uint32_t chunk_start(uint32_t c) { return c * kChunk; }            // the first bin of chunk c
// the same for an index u that counts units of PER bins (K2p: a 16-byte group of 8 records, a ring batch)
template <uint32_t PER>
AVR_CHUNK_HD uint32_t chunk_of_unit(uint32_t u) {
    static_assert(PER && (PER & (PER - 1)) == 0 && kChunk % PER == 0, "a chunk is a power of two of whole units");
    return u >> (kChunkLog2 - floor_log2(PER));
}
template <uint32_t PER>
AVR_CHUNK_HD uint32_t unit_in_chunk(uint32_t u) { return u & (kChunk / PER - 1); }
AVR_CHUNK_HD uint32_t chunks_of(uint32_t n_bins) { return (n_bins + kChunk - 1) / kChunk; }   // chunks that hold bins: 0 for an empty slice (the plan, slice_chunks, gives it one)

// ---- the bins [i0, i1) of chunk c of a slice of n bins, and how many they are: chunk_bins == i1 - i0 for every chunk that starts
// inside the slice.  One that starts at or past its end (the one chunk of an empty slice; an index nobody has checked) has no bins
// and i1 == n <= i0: a caller that walks [i0, i1) clamps i0 (k_k1p_local), a caller that counts asks chunk_bins (the estimator kernels).
struct ChunkSpan { uint32_t i0, i1; };
AVR_CHUNK_HD ChunkSpan chunk_span(uint32_t c, uint32_t n) {
    const uint32_t i0 = chunk_start(c);
    return ChunkSpan{i0, i0 + kChunk < n ? i0 + kChunk : n};
}
AVR_CHUNK_HD uint32_t chunk_bins(uint32_t c, uint32_t n) {
    const uint32_t i0 = chunk_start(c);
    return n > i0 ? (n - i0 < kChunk ? n - i0 : kChunk) : 0u;
}

// ---- what the kernels assume about the length
static_assert((kChunk & (kChunk - 1)) == 0 && (1u << kChunkLog2) == kChunk, "chunk_of / bin_in_chunk / chunk_of_unit / unit_in_chunk are a shift and a mask, and kChunkPosMask is a mask");
static_assert(kChunk % 32 == 0, "a chunk's bit string is whole dwords (lbits, the rows of k_k1p_local's `bits`)");
static_assert(kChunk % 16 == 0, "a chunk's codes and records are whole 16-byte groups: chunk starts stay 16-byte aligned in every record width");
static_assert(2 * kChunk <= 65536, "k_k1p_local: two 16-bit counters a dword with no carry between them, 16-bit lend entries, and the spare row counts on from kChunk");
static_assert(kChunkBitDwords >= 4 && (kChunkBitDwords & (kChunkBitDwords - 1)) == 0, "the chains read a 128-bit window from dword (pos / 32) mod kChunkBitDwords of a string");

}  // namespace avr
