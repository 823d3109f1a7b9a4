// The compress direction's adaptive estimators on the device: KEY records (bin, model key) in, K2 range records
// (bin, pos, neg) out -- what compress_recorder::record / h264_model::update_state_for_model_key do per bin on the host
// (recode.cpp:823-827, 1037-1052), for the 1026 keys h264_model keeps in flat_[] (residual hooks off).
//
// The rule.  An estimator is {pos, neg}, fresh {1, 1}.  A bin of its key is coded with the pair as it stands, then pos
// (bin 1) or neg (bin 0) goes up by one, and when pos + neg exceeds 0x60 both are halved, rounding up.  The total is 97
// at that moment -- odd, so exactly one of the two is odd and the total afterwards is always 49: a key's halvings sit at
// fixed ranks of its own bin sequence (from total t after 97 - t bins, then after every 48th), and the total before any
// bin follows from the bin's rank alone (total_after).  Only pos needs the bins' values.
//
// Estimators belong to a GROUP: consecutive slices sharing one table.  The slices' chunks (kChunk bins, the plan's
// chunk_base / chunk_slice) are numbered through the batch, so a group is a range of global chunks [a, b).  Chunks are
// taken in WINDOWS of kWindow consecutive global chunks, one wave a window, which walks its chunks in stream order 64 bins
// a step with the table of the group at hand in LDS (walk_group: the bins of one key inside a step, in lane order).
//   * A group that lies inside one window is resolved by that window's wave alone, start to end: no workspace, no
//     other kernel.  This is the shape of many independent short slices.
//   * A group that crosses a window boundary ("spanning") is cut into ROWS, its part of each window.  Row r of window w
//     is 2w for the group that comes in from the left and 2w + 1 for the one that starts inside and leaves to the right
//     (at most one of each), so rows need no allocation pass.  Per row and key:
//       count   bins of the key in the row                              (k_est_count, any order: LDS atomics)
//       scan    total of the estimator at the row's start               (k_est_scan_agg + k_est_scan, from the ranks: total_after)
//       func    the row as a FUNCTION pos at its start -> pos at its end (k_est_func, the walk with FnRun)
//       chain   pos at every row's start                                (k_est_chain_agg + k_est_chain: fn_compose, fn_apply)
//     and then the same walk as for the small groups, each row from its own start table (k_est_emit).
//     The function of a row: every halving is pos <- (pos + ones + 1) >> 1, and such steps compose into
//     pos -> (pos + a) >> s exactly (floor of floor); past s = 16 the form is renormalised to s = 8, which is exact
//     because pos < 128 makes (pos + a) >> s a step function of pos with one threshold (fn_normalise).  Scan and chain run over
//     blocks of kRowBlock rows (RowSeq below), so the longest serial walk over a group is its blocks plus one block's rows, a
//     step each -- not one per bin, per halving or per row.
// One-byte key records (AVR_KIND_RANGE_KEYS8: bin | dense id << 1, 128 ids, every one a key) go through the same kernels in a second
// instantiation (avr_est.hip: Keys8 -- 7 ballots to a key match, tables of 128 entries, 16 records to a 16-byte load); nothing below
// depends on the width.
// Everything here also compiles for the CPU: tests/est_emul.cpp runs these functions against a plain restatement.
#pragma once
#include <stdint.h>

#include "avr_layout.h"                                // kKeysPad, kWindow, n_rows and the workspace: EstLayout

#if defined(__HIPCC__)
#define AVR_EST_HD __host__ __device__ inline
#else
#define AVR_EST_HD inline
#endif

namespace avr {
namespace est {

constexpr uint32_t kKeys = 1026;                       // context ids 0..1023, bypass, terminate: h264_model's flat_[]
constexpr uint32_t kLimit = 0x60;                      // recode.cpp:1046: halve when pos + neg exceeds this
constexpr uint32_t kFresh = 1u | (1u << 8);            // {1, 1}; a table entry is pos | neg << 8
constexpr uint32_t kNoBad = 0xffffffffu;

AVR_EST_HD bool key_ok(uint32_t rec) { return (rec >> 1) < kKeys; }          // bits 12..15 clear and key <= AVR_SEL_TERMINATE
AVR_EST_HD uint32_t total(uint32_t st) { return (st & 0xffu) + (st >> 8); }
// the K2 record of a bin met with estimator st: bin | pos << 1 | neg << 8
AVR_EST_HD uint32_t record(uint32_t st, uint32_t bin) { return bin | ((st & 0xffu) << 1) | (st & 0xff00u); }
// one bin (recode.cpp:1037-1052 for the keys that halve at 0x60)
AVR_EST_HD uint32_t step(uint32_t st, uint32_t bin) {
    uint32_t pos = (st & 0xffu) + bin, neg = (st >> 8) + (1u - bin);
    if (pos + neg > kLimit) { pos = (pos + 1) >> 1; neg = (neg + 1) >> 1; }
    return pos | (neg << 8);
}
// total of an estimator that started at total t, before the bin of rank j of its key
AVR_EST_HD uint32_t total_after(uint32_t t, uint64_t j) {
    const uint64_t first = kLimit + 1 - t;             // bins up to and including the first halving
    return j < first ? t + uint32_t(j) : 49u + uint32_t((j - first) % 48u);
}

// records a walk writes for a chunk of n bins that starts at bin `start` of a slice of nb: behind the slice's last bin, the
// no-op records up to the slice's next multiple of eight
AVR_EST_HD uint32_t padded_bins(uint32_t start, uint32_t n, uint32_t nb) { return start + n == nb ? ((nb + 7u) & ~7u) - start : n; }

AVR_EST_HD uint32_t popc64(uint64_t m) { return uint32_t(__builtin_popcountll(m)); }
AVR_EST_HD uint32_t ctz64(uint64_t m) { return uint32_t(__builtin_ctzll(m)); }      // m != 0

// The bins of ONE key inside a step of up to 64 bins: `mask` = the step's lanes that hold the key, `ones` = the lanes whose bin
// is 1, st0 = the key's estimator before the step.  A lane with `below` lanes of the key before it, `below_ones` of them 1:
// no_halving(st0, n) says that n bins from st0 do not reach a halving, and then the estimator after them is advance().
AVR_EST_HD bool no_halving(uint32_t st0, uint32_t n) { return total(st0) + n <= kLimit; }
AVR_EST_HD uint32_t advance(uint32_t st0, uint32_t n, uint32_t n_ones) { return st0 + n_ones + ((n - n_ones) << 8); }
// ... and where a halving falls inside: the key's lanes one after the other.  pre[l] = the estimator lane l's bin meets;
// returns the estimator after the last.  (One halving per 48 bins of a key: about one key a step takes this way.)
template <class Pre>
AVR_EST_HD uint32_t walk_group(uint32_t st0, uint64_t mask, uint64_t ones, Pre &&pre) {
    uint32_t st = st0;
    while (mask) {
        const uint32_t l = ctz64(mask);
        mask &= mask - 1;
        pre(l, st);
        st = step(st, uint32_t(ones >> l) & 1u);
    }
    return st;
}

// ------------------------------------------------------------------ a row as a function of pos at its start
// fn = s << 27 | a  stands for  pos -> (pos + a) >> s,  s <= 16 and a < 97 << 16 between calls.
constexpr uint32_t kFnShift = 27, kFnMask = (1u << kFnShift) - 1, kFnIdentity = 0;
AVR_EST_HD uint32_t fn_apply(uint32_t fn, uint32_t pos) { return (pos + (fn & kFnMask)) >> (fn >> kFnShift); }
// s >= 8 and pos < 128: (pos + a) >> s = (a >> s) + (pos >= 2^s - (a mod 2^s)), and the same holds for the result with s = 8
AVR_EST_HD uint32_t fn_normalise(uint32_t s, uint32_t a) {
    const uint32_t hi = a >> s, lo = a & ((1u << s) - 1), theta = (1u << s) - lo;
    return (8u << kFnShift) | (hi << 8) | (theta >= 256u ? 0u : 256u - theta);
}
// followed by a halving with `ones` 1-bins since the row's start or the halving before: pos <- (pos + ones + 1) >> 1
AVR_EST_HD uint32_t fn_halve(uint32_t fn, uint32_t ones) {
    const uint32_t s = fn >> kFnShift, a = (fn & kFnMask) + ((ones + 1) << s);
    return s + 1 > 16 ? fn_normalise(s + 1, a) : ((s + 1) << kFnShift) | a;
}
// f, then g: (((pos + af) >> sf) + ag) >> sg = (pos + af + (ag << sf)) >> (sf + sg)
AVR_EST_HD uint32_t fn_compose(uint32_t f, uint32_t g) {
    const uint32_t sf = f >> kFnShift, s = sf + (g >> kFnShift);
    const uint64_t a = uint64_t(f & kFnMask) + (uint64_t(g & kFnMask) << sf);
    if (s <= 16) return (s << kFnShift) | uint32_t(a);
    const uint64_t hi = a >> s, lo = a & ((uint64_t(1) << s) - 1), theta = (uint64_t(1) << s) - lo;    // fn_normalise in 64 bits
    return (8u << kFnShift) | (uint32_t(hi) << 8) | (theta >= 256u ? 0u : 256u - uint32_t(theta));
}
// followed by `ones` 1-bins and no halving (the row's end)
AVR_EST_HD uint32_t fn_close(uint32_t fn, uint32_t ones) { return fn + (ones << (fn >> kFnShift)); }

// what the function walk keeps per key: the function so far, the total now, the 1-bins since the last halving
struct FnRun { uint32_t fn, tot, ones; };
AVR_EST_HD FnRun fn_walk_group(FnRun r, uint64_t mask, uint64_t ones) {
    const uint32_t n = popc64(mask);
    if (r.tot + n <= kLimit) { r.tot += n; r.ones += popc64(mask & ones); return r; }
    while (mask) {
        const uint32_t l = ctz64(mask);
        mask &= mask - 1;
        r.ones += uint32_t(ones >> l) & 1u;
        if (++r.tot > kLimit) { r.fn = fn_halve(r.fn, r.ones); r.ones = 0; r.tot = 49; }
    }
    return r;
}

// ------------------------------------------------------------------ windows and rows
// A group's chunks [a, b), a window's [w * W, (w + 1) * W).
AVR_EST_HD bool spanning(uint32_t a, uint32_t b, uint32_t W) { return b > a && a / W != (b - 1) / W; }
AVR_EST_HD uint32_t row_of(uint32_t w, uint32_t a, uint32_t W) { return 2 * w + (a >= w * W ? 1u : 0u); }
// The (at most two) rows of window w: [0] the spanning group that comes in from the left, [1] the spanning group that starts in
// the window and leaves it.  c0 == c1: no such row.  g = the row's group.
struct Row { uint32_t c0, c1, g, a, b; };
template <class GroupOf>
AVR_EST_HD void window_rows(uint32_t w, uint32_t W, uint32_t total_chunks, GroupOf &&group_of, Row rows[2]) {
    const uint32_t lo = w * W, hi = lo + W < total_chunks ? lo + W : total_chunks;
    rows[0] = rows[1] = Row{0, 0, 0, 0, 0};
    if (lo >= hi) return;
    Row first = group_of(lo), last = group_of(hi - 1);           // c0 / c1 unset: g, a, b of the chunk's group
    if (first.a < lo && spanning(first.a, first.b, W)) { first.c0 = lo; first.c1 = first.b < hi ? first.b : hi; rows[0] = first; }
    if (last.a >= lo && last.b > hi) { last.c0 = last.a; last.c1 = hi; rows[1] = last; }
}
// Rows of a spanning group in stream order: the first is 2 * (a / W) + 1, then 2 * w for every further window up to (b - 1) / W.
// The scan and the chain over a group's rows run in BLOCKS of kRowBlock rows: first every block's aggregate (its count sum, its
// composed function: *_agg kernels, kept in the 32-bit slot of the block's LAST row, whose own value nothing needs any more), then
// every block from the aggregates of the blocks before it.  The longest serial walk is a group's blocks plus one block's rows.
constexpr uint32_t kRowBlock = 64;
struct RowSeq {
    uint32_t w0, n;                                               // the group's first window, its rows
    AVR_EST_HD uint32_t row(uint32_t i) const { return i ? 2 * (w0 + i) : 2 * w0 + 1; }
    AVR_EST_HD uint32_t block_end(uint32_t kb) const { return (kb + 1) * kRowBlock < n ? (kb + 1) * kRowBlock : n; }
};
// The (at most two) blocks that begin in window w: [0] of the group that comes in from the left, [1] of the one that starts here.
struct BlockHead { bool any; uint32_t g, kb; RowSeq seq; };
AVR_EST_HD void window_block_heads(uint32_t w, uint32_t W, const Row rows[2], BlockHead heads[2]) {
    heads[0].any = heads[1].any = false;
    if (rows[0].c0 < rows[0].c1) {
        const uint32_t w0 = rows[0].a / W;
        if ((w - w0) % kRowBlock == 0) heads[0] = BlockHead{true, rows[0].g, (w - w0) / kRowBlock, RowSeq{w0, (rows[0].b - 1) / W - w0 + 1}};
    }
    if (rows[1].c0 < rows[1].c1) heads[1] = BlockHead{true, rows[1].g, 0, RowSeq{w, (rows[1].b - 1) / W - w + 1}};
}

// the workspace is avr_layout.h's EstLayout; its size for the emulator (tests/est_emul.cpp)
inline uint64_t workspace_bytes(uint64_t n_slices, uint64_t n_groups, uint64_t total_chunks) {
    return est_layout(n_slices, n_groups, total_chunks).total;
}

}  // namespace est
}  // namespace avr
