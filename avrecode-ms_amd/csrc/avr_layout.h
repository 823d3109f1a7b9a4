// Where everything lies in the device workspaces a caller hands in: one struct of byte offsets (and `total`) per workspace, each made
// by ONE function through one cursor.  The *_workspace_bytes functions quote `total`, the launchers take their pointers from the same
// struct, so a quote and its carving cannot drift apart (callers allocate exactly the quote: tests/test_gpu_workspace.py holds them
// to it, tests/test_layouts.py holds the numbers).  Host only, plain C++17, no HIP header: tests/layout_check.cpp compiles it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/avrecode_ms_amd.h"
#include "avr_k1p.h"

namespace avr {

inline uint64_t align256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

// regions one behind the other, every start a multiple of 256 unless a layout says otherwise
struct Cursor {
    uint64_t at = 0;
    uint64_t take(uint64_t bytes) { const uint64_t o = at; at += align256(bytes); return o; }
    uint64_t take_unrounded(uint64_t bytes) { const uint64_t o = at; at += bytes; return o; }
};

// ------------------------------------------------------------------ K1p (avr_k1p.hip)

// k_k1p_tn's table: tn[(128 << n) - 128 + (st << n | bits)], bits < 2^n, n = 0 .. 8
constexpr uint32_t kTnBytes = 128 * 511;
constexpr uint32_t kMaxChainSegs = 16;                           // segments a context chain is cut in, at most
constexpr uint32_t kSegBits = 128;                               // bins a segment's bit string holds
struct alignas(16) SegSummary {
    uint64_t bits[2];         // the segment's bins of this context, first bin in bit 0 of bits[0] (valid when n_bins <= kSegBits)
    uint32_t n_bins;          // (of a segment whose walks did not meet: one that met is left with more than kSegBits whatever it had)
    uint8_t exit_state;       // state after the segment when the walks met
    uint8_t met;              // 1: the walks met (exit_state valid, chunks from met_chunk on are noted)
    uint16_t met_chunk;       // first chunk of the segment (relative to its start) whose entry state is noted; segment length if none
};

// resolved codes, wave-interleaved in tiles of kTileChunks chunks, a row a 16-byte group of each (TileCodes in avr_k1p.hip): whole tiles
constexpr uint32_t kTileChunks = 64, kTileRowBytes = kTileChunks * 16;
inline uint64_t tile_codes_bytes(uint32_t total_chunks) { return (uint64_t(total_chunks) + kTileChunks - 1) / kTileChunks * kTileChunks * kChunkCodeBytes; }

// Phase A (launch_resolve): per-chunk bit strings, end positions and entry states, tables; laid out for the caller's context count
// `ns` -- the kernels index it by the dense count, which is known only after the census.
struct ResolveLayout { uint64_t lbits, lend, est, stretch, meta, summ, total; };
inline ResolveLayout resolve_layout(size_t n_slices, uint32_t ns, const avr_chunk_plan *pl) {
    ResolveLayout L;
    Cursor c;
    L.lbits = c.take(uint64_t(pl->total_chunks + 64) * kChunkBitBytes);   // + 64 chunks: the chains read a few chunks ahead, unconditionally
    L.lend = c.take(uint64_t(pl->total_chunks + 64) * ns * 2 + 256) + 128;   // 128 bytes into its region: k_k1p_ctxchain reads lend[-1]
    L.est = c.take(uint64_t(pl->total_chunks) * ((ns + 3) / 4) * 4 + 16);    // + 16: slack behind the last row; callers allocate exactly the quote, so it stays
    L.stretch = c.take(uint64_t(pl->total_chunks) * sizeof(k1p::Stretch));
    L.meta = c.take(256 + 2 * AVR_MAX_STATES + 2 * AVR_MAX_STATES + kTnBytes);   // used[32] + n_dense, table[AVR_MAX_STATES], index[AVR_MAX_STATES], tn
    L.summ = c.take(uint64_t(n_slices) * ns * kMaxChainSegs * sizeof(SegSummary));    // the segmented chains' summaries
    L.total = c.at;
    return L;
}

// Phases B-D (launch_code): stretch summaries, entries, per-slice totals, digit sums, and B1's wave-interleaved copy of the codes
struct CodeLayout { uint64_t stretch, entry, totals, sums, tile, total; };
inline CodeLayout code_layout(size_t n_slices, const avr_chunk_plan *pl) {
    CodeLayout L;
    Cursor c;
    L.stretch = c.take(uint64_t(pl->total_chunks) * sizeof(k1p::Stretch));
    L.entry = c.take(uint64_t(pl->total_chunks) * sizeof(k1p::Entry));
    L.totals = c.take(uint64_t(n_slices) * sizeof(k1p::SliceTotals));
    L.sums = c.take(pl->dig_total * 4 + 16);                     // + 16: slack behind the last slice's digits; stays for the same reason
    L.tile = c.take(tile_codes_bytes(pl->total_chunks));
    L.total = c.at;
    return L;
}

// The whole path (launch_k1p, launch_k1p_retry, launch_k1p8): the code buffer between the two stages, then the two workspaces above
struct K1pLayout { uint64_t codes, resolve, code, total; };   // resolve / code: where a ResolveLayout / a CodeLayout starts
inline K1pLayout k1p_layout(size_t n_slices, uint32_t ns, const avr_chunk_plan *pl) {
    K1pLayout L;
    Cursor c;
    // the larger of the tiled size (what the path itself writes) and the linear one: + 32 as the header asks of a caller's code buffer
    const uint64_t tiled = tile_codes_bytes(pl->total_chunks), linear = pl->res_total + 32;
    L.codes = c.take(tiled > linear ? tiled : linear);
    L.resolve = c.take(resolve_layout(n_slices, ns, pl).total);
    L.code = c.take(code_layout(n_slices, pl).total);            // begins at resolve.total behind `resolve`: both totals are multiples of 256
    L.total = c.at;
    return L;
}

// ------------------------------------------------------------------ K2p (avr_k2p.hip)

// ck_range, ck_pos per chunk; fin_range, fin_pos per slice; the hybrid pass 1's list of long slices; 32-bit sums per output byte position
struct K2pLayout { uint64_t ck_range, ck_pos, fin_range, fin_pos, long_chunks, sums, total; };
inline K2pLayout k2p_layout(size_t n_slices, uint32_t total_chunks, uint64_t out_total) {
    K2pLayout L;
    Cursor c;
    L.ck_range = c.take(uint64_t(total_chunks) * 8);
    L.ck_pos = c.take(uint64_t(total_chunks) * 4);
    L.fin_range = c.take(uint64_t(n_slices) * 8);
    L.fin_pos = c.take(uint64_t(n_slices) * 4);
    // threshold, count and the long slices, 1 024 words: at most 1 007 slices where launch_k2p takes the hybrid by the batch's shape
    // (1 025 .. 61 440 slices); under the test hook k2p_wave = 3 at most 1 022 from 65 slices on, and no more than there are slices
    // below (tests/test_k2p_ragged.py).  A multiple of 256 as it is
    L.long_chunks = c.take_unrounded(4096);
    L.sums = c.take(out_total * 4 + 64);                         // + 64: slack behind the last slice's sums; the quote has always had it
    L.total = c.at;
    return L;
}

// ------------------------------------------------------------------ the estimator resolver (avr_est.hip)

namespace est {
constexpr uint32_t kKeysPad = 1028;                    // a table's stride in the workspace
constexpr uint32_t kKeysPad8 = 128;                    // ... of one-byte key records (AVR_KIND_RANGE_KEYS8): the 128 dense ids, nothing to pad
constexpr uint32_t kWindow = 16;                       // chunks per window
inline uint64_t n_rows(uint64_t total_chunks, uint32_t W) { return 2 * ((total_chunks + W - 1) / W); }
}  // namespace est

// slice -> group, first bad slice per group, per row a 32-bit table (counts, then functions) and a 16-bit one (totals, then
// {pos, neg} at the row's start); rows exist whether a group spans windows or not.  keys_pad: the tables' stride, kKeysPad for two-byte
// key records, kKeysPad8 for one-byte ones (768 bytes a row)
struct EstLayout { uint64_t slice_group, group_bad, row32, row16, total; };
inline EstLayout est_layout(uint64_t n_slices, uint64_t n_groups, uint64_t total_chunks, uint32_t keys_pad = est::kKeysPad) {
    EstLayout L;
    Cursor c;
    const uint64_t rows = est::n_rows(total_chunks, est::kWindow);
    L.slice_group = c.take(4 * n_slices);
    L.group_bad = c.take(4 * n_groups);
    L.row32 = c.take_unrounded(rows * keys_pad * 4);
    L.row16 = c.take_unrounded(rows * keys_pad * 2);             // directly behind row32, unrounded: the header documents 6 168 bytes a row
    L.total = c.at;
    return L;
}

// ------------------------------------------------------------------ the estimator checker (avr_est_verify.hip)

namespace estv {
constexpr uint32_t kTabStride = 1028;                  // a 16-bit table's stride in the workspace
constexpr uint32_t kTabStride8 = 128;                  // ... of one-byte key records
constexpr uint32_t kSpan = 16;                         // chunks per span (the checker's own: nothing ties it to the resolver's window)
inline uint64_t n_slots(uint64_t total_chunks, uint32_t S) { return 2 * ((total_chunks + S - 1) / S); }
}  // namespace estv

// slice -> group, then per piece slot a 16-bit table (what the key's next bin must carry after the piece, then the table at the
// piece's start) and a second one for the aggregate of the block of pieces that ends there; no larger than EstLayout for the same
// batch, so the resolver's workspace can be handed on as it stands.  stride: kTabStride, or kTabStride8 for one-byte key records (512
// bytes a slot)
struct EstVerifyLayout { uint64_t slice_group, tab, agg, total; };
inline EstVerifyLayout est_verify_layout(uint64_t n_slices, uint64_t total_chunks, uint32_t stride = estv::kTabStride) {
    EstVerifyLayout L;
    Cursor c;
    const uint64_t slots = estv::n_slots(total_chunks, estv::kSpan);
    L.slice_group = c.take(4 * n_slices);
    L.tab = c.take_unrounded(slots * stride * 2);
    L.agg = c.take_unrounded(slots * stride * 2);
    L.total = c.at;
    return L;
}

}  // namespace avr
