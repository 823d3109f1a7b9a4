// The estimator checker: are resolved K2 range records (bin | pos << 1 | neg << 8) the ones the sequential rule gives for their KEY
// records (bin | key << 1)?  An independent check of the resolver (avr_est.h), of which it includes and shares nothing: it never
// computes a rank, a total from a rank, a composed function or a row start.  It only holds every record to its predecessor.
//
// The rule restated.  step(e, b): pos += b, neg += 1 - b, and if pos + neg > 0x60 both are halved rounding up.  Over a GROUP
// (consecutive slices sharing one table), its bins in stream order:
//   1  bit 0 of a resolved record is bit 0 of its key record (and the key record is well-formed);
//   2  the first bin of a key in the group carries est_in[group][key] ({1, 1} without est_in);
//   3  every other bin carries step(e', b'): e' the RECORDED pair of the key's previous bin in the group, b' that bin;
//   4  from n_bins to the slice's next multiple of eight the records are AVR_NOP_RANGE (0);
//   5  est_out[group][key] is step of the key's last recorded pair and bin, or the start entry of a key the group never met.
// By induction 1-5 hold exactly when records and table are those of the rule, and each looks at one record and one predecessor.
//
// Geometry, from the chunk plan as the resolver takes it: chunks of kChunk bins numbered through the batch, a group = global chunks
// [a, b).  A SPAN is kSpan consecutive global chunks, one wave each; a PIECE is a group's part of a span.  A group inside one span
// is checked by that span's wave alone.  A group that crosses a span boundary has a piece per span: slot 2w for the piece that
// comes into span w from the left, 2w + 1 for the one that starts in w and leaves it (at most one of each).  Per piece and key:
//   last    the estimator the key's NEXT bin must carry after the piece: step of the recorded pair of its last bin in the piece,
//           0 = the piece did not meet the key (a pair never is 0: neg + 1 - b or pos + b is at least 1)
//   start   the table at the piece's start: est_in, overridden by the last earlier piece that met the key ("the last one that met
//           it wins": associative, so the walk over a group's pieces runs in blocks of kPieceBlock, PieceSeq below)
// and then the walk (check), 64 bins a step: a lane's expected pair is next_of() of the nearest lower lane of the step with its key
// where there is one, else the table entry; the key's last lane of the step writes its own next_of() to the table.
// Everything here also compiles for the CPU: tests/est_verify_emul.cpp runs these functions with the lanes emulated.
#pragma once
#include <stdint.h>

#include "avr_layout.h"                                // estv::kSpan, kTabStride and the workspace: EstVerifyLayout

#if defined(__HIPCC__)
#define AVR_ESTV_HD __host__ __device__ inline
#else
#define AVR_ESTV_HD inline
#endif

namespace avr {
namespace estv {

constexpr uint32_t kKeys = 1026;                       // context ids 0..1023, bypass, terminate
constexpr uint32_t kFresh = 1u | (1u << 8);            // {1, 1}; a table entry is pos | neg << 8
static_assert(kSpan * kChunk < 65536, "last_entry: a bin's position in its piece (at most kSpan chunks) goes into 16 bits");
constexpr uint32_t kNone = 0xffffffffu;                // AVR_VERIFY_NONE
constexpr uint32_t kPieceBlock = 64;                   // pieces per block of the start walk
constexpr int32_t kOk = 0, kBadRecord = 3, kVerifyFailed = 4;    // AVR_SLICE_OK, _BAD_RECORD, _VERIFY_FAILED

AVR_ESTV_HD bool key_ok(uint32_t krec) { return (krec >> 1) < kKeys; }
// the pair a resolved record carries, as a table entry (bit 15 of the record stays in neg: a record with it set matches nothing)
AVR_ESTV_HD uint32_t pair_of(uint32_t rrec) { return ((rrec >> 1) & 0x7fu) | (rrec & 0xff00u); }
// the rule, from whatever pair was recorded: pos <= 127, neg <= 255 in, a 16-bit entry that is never 0 out
AVR_ESTV_HD uint32_t step(uint32_t e, uint32_t b) {
    uint32_t pos = (e & 0xffu) + b, neg = (e >> 8) + 1u - b;
    if (pos + neg > 0x60u) { pos = (pos + 1) >> 1; neg = (neg + 1) >> 1; }
    return pos | (neg << 8);
}
// what the key's next bin must carry behind a bin recorded as rrec whose key record is krec
AVR_ESTV_HD uint32_t next_of(uint32_t rrec, uint32_t krec) { return step(pair_of(rrec), krec & 1u); }
// conditions 1 to 3 for one bin: its key record, its resolved record, the pair it is expected to carry
AVR_ESTV_HD bool bin_bad(uint32_t krec, uint32_t rrec, uint32_t expected) {
    return !key_ok(krec) || ((krec ^ rrec) & 1u) || pair_of(rrec) != expected;
}
// records of a chunk of n bins that starts at bin `start` of a slice of nb, padding included (condition 4 lives behind n)
AVR_ESTV_HD uint32_t padded_bins(uint32_t start, uint32_t n, uint32_t nb) { return start + n == nb ? ((nb + 7u) & ~7u) - start : n; }
// the nearest lane below `lane` in mask, or -1
AVR_ESTV_HD int lower_lane(uint64_t mask, uint32_t lane) {
    const uint64_t below = mask & ((uint64_t(1) << lane) - 1);
    return below ? 63 - __builtin_clzll(below) : -1;
}
// what k_estv_last keeps per key: the bin's position in the piece above its next_of(); the largest position wins
AVR_ESTV_HD uint32_t last_entry(uint32_t pos_in_piece, uint32_t next) { return (pos_in_piece << 16) | next; }

// ------------------------------------------------------------------ spans and pieces
struct Group { uint32_t g, a, b; };                    // a group and its global chunks [a, b)
AVR_ESTV_HD bool crossing(uint32_t a, uint32_t b, uint32_t S) { return b > a && a / S != (b - 1) / S; }
// The (at most two) pieces of span w that belong to crossing groups: [0] comes in from the left, [1] starts here and leaves.
// c0 == c1: no such piece.
struct Piece { uint32_t c0, c1; Group gr; };
template <class GroupOf>
AVR_ESTV_HD void span_pieces(uint32_t w, uint32_t S, uint32_t total_chunks, GroupOf &&group_of, Piece pc[2]) {
    const uint32_t lo = w * S, hi = lo + S < total_chunks ? lo + S : total_chunks;
    pc[0] = pc[1] = Piece{0, 0, Group{0, 0, 0}};
    if (lo >= hi) return;
    const Group first = group_of(lo), last = group_of(hi - 1);
    if (first.a < lo) pc[0] = Piece{lo, first.b < hi ? first.b : hi, first};          // it began in an earlier span: it crosses
    if (last.a >= lo && last.b > hi) pc[1] = Piece{last.a, hi, last};
}
// The pieces of a crossing group in stream order: slot 2 * (a / S) + 1, then 2 * w for every further span up to (b - 1) / S.
struct PieceSeq {
    uint32_t w0, n;
    AVR_ESTV_HD uint32_t slot(uint32_t i) const { return i ? 2 * (w0 + i) : 2 * w0 + 1; }
    AVR_ESTV_HD uint32_t block_end(uint32_t kb) const { return (kb + 1) * kPieceBlock < n ? (kb + 1) * kPieceBlock : n; }
};
AVR_ESTV_HD PieceSeq piece_seq(const Group &gr, uint32_t S) { return PieceSeq{gr.a / S, (gr.b - 1) / S - gr.a / S + 1}; }
// The (at most two) blocks of the start walk that begin in span w, one per piece of span_pieces.
struct BlockHead { bool any; uint32_t g, kb; PieceSeq seq; };
AVR_ESTV_HD void span_block_heads(uint32_t w, uint32_t S, const Piece pc[2], BlockHead heads[2]) {
    heads[0].any = heads[1].any = false;
    if (pc[0].c0 < pc[0].c1) {
        const PieceSeq seq = piece_seq(pc[0].gr, S);
        if ((w - seq.w0) % kPieceBlock == 0) heads[0] = BlockHead{true, pc[0].gr.g, (w - seq.w0) / kPieceBlock, seq};
    }
    if (pc[1].c0 < pc[1].c1) heads[1] = BlockHead{true, pc[1].gr.g, 0, piece_seq(pc[1].gr, S)};
}
// "the last piece that met the key wins": cur, then a piece whose last-table holds v for the key
AVR_ESTV_HD uint32_t then(uint32_t cur, uint32_t v) { return v ? v : cur; }

// the workspace is avr_layout.h's EstVerifyLayout; its size for the emulator
inline uint64_t workspace_bytes(uint64_t n_slices, uint64_t total_chunks) { return est_verify_layout(n_slices, total_chunks).total; }

}  // namespace estv
}  // namespace avr
