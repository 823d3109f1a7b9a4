// The CABAC arithmetic decoder of ITU-T H.264 (9.3.1.2 initialisation, 9.3.3.2: DecodeDecision Figure 9-3, DecodeBypass 9-5,
// DecodeTerminate 9-6) for streams whose records are KNOWN: the verifier behind the K1 encoders (avr_cabac_verify.hip).
//
// A K1 slice's output is a standard CABAC stream, and at verify time the context of every bin is known from the records the encoder
// read.  So the decoder is handed each bin's context (or, for resolved codes, its state), decodes the bin and compares.  It is written
// from the standard, keeps the context states itself by the plain sequential rule of Figure 9-3, in the CALLER's numbering of the
// contexts, and has no carries, no deferred digits and no finish().  The one thing it shares with the encoders -- the one-lane
// kernels, K1p with its census, dense map, chains and phase D, the code forms -- is the table of avr_tables.h (rangeTabLPS and the
// state transitions), which tests/test_cabi.py holds to the oracle's.
//
// `__host__ __device__` in the way avr_verify.h is: tests/cabac_verify_emul.cpp runs the very functions the kernel runs.
#pragma once
#include <stdint.h>

#include "avr_div.h"
#include "avr_tables.h"

#ifndef AVR_VERIFY_NONE
#define AVR_VERIFY_NONE 0xFFFFFFFFu
#endif

// On the device: ties a bin's record to the decoder's state before it, so that what is derived from the record -- the kind of the bin,
// as wave-wide conditions, a pair of SGPRs each -- is worked out when the bin's turn comes.  Without it hipcc works out the kinds of all
// sixteen bins of a chunk ahead of its first and keeps them to the end, which is more SGPRs than a wave has: they spill.
#if defined(__HIP_DEVICE_COMPILE__)
#define AVR_CV_IN_TURN(rec, state) asm volatile("" : "+v"(rec), "+v"(state))
#else
#define AVR_CV_IN_TURN(rec, state) (void)0
#endif

namespace avr {
namespace cabac_verify {

// The record forms behind the one walk: where a chunk lies is the Source's business, what its bytes mean is decided here.
//   kTiles2 / kSlices2   two-byte records (AVR_KIND_CABAC: bin | selector << 1), eight a 16-byte chunk
//   kTiles8 / kSlices8   one-byte records (AVR_KIND_CABAC8: bin | dense selector << 1), sixteen a chunk
//   kCodes               resolved codes (AVR_CODE_*: the (symbol, *state) pair of every bin), sixteen a chunk, no states kept
enum Form : int { kTiles2 = 0, kSlices2 = 1, kTiles8 = 2, kSlices8 = 3, kCodes = 4, kForms = 5 };
constexpr bool form_wide(int form) { return form == kTiles2 || form == kSlices2; }
constexpr bool form_tiled(int form) { return form == kTiles2 || form == kTiles8; }
constexpr uint32_t form_per_chunk(int form) { return form_wide(form) ? 8u : 16u; }
constexpr uint32_t form_max_states(int form) { return form == kCodes ? 0u : form_wide(form) ? 1024u : 126u; }

struct alignas(8) TabEntry { uint32_t x, y; };                   // CabacTables::packed[s]: rangeTabLPS[p][0..3] | next state after MPS, after LPS << 8
inline void fill_table(TabEntry *tab, const CabacTables &t) {
    for (int s = 0; s < 128; s++) tab[s] = TabEntry{t.packed[s][0], t.packed[s][1]};
}

// The coded bytes of one slice as a string of bits, most significant bit of each byte first (7.2), read in aligned 8-byte words (a region
// starts at a multiple of 8 and its capacity is one), one word ahead of the word in use -- verify::WordReader's scheme.  Every bit at or
// beyond byte `len` reads as zero whatever the region holds there: a word that starts at or past `len` is never loaded, the word
// that straddles it is masked.  len <= capacity, so no load leaves the region.
struct BitReader {
    const uint64_t *words;
    uint32_t len, widx, left;                                    // left: bits of `cur` not yet taken, at its top
    uint64_t cur, ahead;

    AVR_DIV_HD uint64_t load(uint32_t w) const {
        const uint64_t at = uint64_t(w) * 8;
        if (at >= len) return 0;
        const uint64_t v = words[w];                             // little endian: stream byte k of the word at bits 8k
        const uint32_t rem = len - uint32_t(at);
        return __builtin_bswap64(rem < 8 ? v & ((uint64_t(1) << (8 * rem)) - 1) : v);   // stream order: the first bit at the top
    }
    AVR_DIV_HD void init(const uint64_t *p, uint32_t n) {
        words = p; len = n; widx = 0; left = 64;
        cur = load(0);
        ahead = load(1);
    }
    AVR_DIV_HD uint32_t take(uint32_t n) {                       // the next n bits, n <= 9 (0: none), the first of them the most significant
        uint32_t v = uint32_t((cur >> 1) >> (63 - n));
        if (n <= left) {
            cur <<= n;
            left -= n;
        } else {                                                 // cur ran out: its last bits (zeros behind them), then the first of the next word
            const uint32_t need = n - left;
            cur = ahead;
            widx++;
            ahead = load(widx + 1);
            v |= uint32_t((cur >> 1) >> (63 - need));
            cur <<= need;
            left = 64 - need;
        }
        return v;
    }
};

// 9.3.1.2 and 9.3.3.2.  codIRange is `range`, codIOffset `offset`.  RenormD (Figure 9-4) shifts one bit at a time while
// codIRange < 256; here the count of those shifts is taken at once (it is the number of leading zeros of the 9-bit range) and the bits
// are read when the NEXT bin begins, together with the one bit DecodeBypass reads first: one read per bin, the same values of range and
// offset at every comparison as in the bit-serial form, whatever the bytes are (the arithmetic is the oracle's unsigned arithmetic).
struct CabacDecoder {
    uint32_t range, offset, pending;                             // pending: shifts of RenormD still owed to offset (range has had them)

    template <class Reader>
    AVR_DIV_HD void init(Reader &in) {                           // 9.3.1.2: codIRange = 510, codIOffset = read_bits(9)
        range = 510;
        offset = in.take(9);
        pending = 0;
    }
    // One bin.  lps4: the four rangeTabLPS values of the bin's pStateIdx, qCodIRangeIdx selecting the byte (unused for bypass).
    // Returns 1 where Figure 9-3 takes the LPS branch (the bin is !valMPS), for bypass the bin itself (Figure 9-5).  DecodeTerminate
    // (Figure 9-6) is this with lps4 = {2, 2, 2, 2}, pStateIdx 63's row: codIRange -= 2, binVal = codIOffset >= codIRange, RenormD --
    // which this form also does behind binVal 1, where the standard ends the slice and so nothing reads the difference.
    template <class Reader>
    AVR_DIV_HD uint32_t get(uint32_t lps4, uint32_t bypass, Reader &in) {
        const uint32_t n = pending + bypass;                     // <= 8
        offset = (offset << n) | in.take(n);
        const uint32_t r_lps = (lps4 >> (8 * ((range >> 6) & 3))) & 0xffu & (bypass - 1u);      // bypass: 0
        const uint32_t r_mps = range - r_lps;                    // bypass: the range as it is
        const uint32_t lps = offset >= r_mps;
        offset -= lps ? r_mps : 0u;
        range = lps ? r_lps + (range & (0u - bypass)) : r_mps;   // bypass: the range as it is on either side
        pending = uint32_t(__builtin_clz(range)) - 23u;          // 2 <= range <= 510: 0 .. 7
        range <<= pending;
        return lps;
    }
};

AVR_DIV_HD uint32_t is_zero(uint32_t x) { return (x - 1u) >> 31 & ~(x >> 31); }     // 1 for x == 0, else 0

struct Chunk16 { uint32_t w[4]; };                               // eight two-byte records, or sixteen one-byte records or codes

// One bin of a slice, `rec` its record or code.  Store: the slice's state bytes, get(ctx) / set(ctx, state), ctx < n_states, and a spare
// byte at n_states that holds nothing; Table: TabEntry by state.
//   a context bin      state from the store, decoded by Figure 9-3, the successor stored
//   bypass             Figure 9-5
//   terminate          Figure 9-6, as the decision at pStateIdx 63, valMPS 0 it is (state byte 126, never stored)
//   a resolved code    code >> 1 is the bin's state byte and code & 1 the bin: 126 (codes 252, 253) bypass, 127 (254, 255) the
//                      terminate bin seen from valMPS 1 -- AVR_CODE_TERMINATE(bin) = 255 - bin -- which decodes as any other state
//   anything else      (a selector that is no context of the slice) is no bin of a CABAC stream: reported as a bad bin
// Returns 0 where the decoded value is the record's, 1 where it is not.
template <int FORM, class Reader, class Store, class Table>
AVR_DIV_HD uint32_t decode_bin(CabacDecoder &d, Reader &in, uint32_t rec, Store &st, const Table &tab, uint32_t n_states) {
    constexpr bool kWide = form_wide(FORM), kIsCodes = FORM == kCodes;
    AVR_CV_IN_TURN(rec, d.pending);
    const uint32_t sel = rec >> 1, want = rec & 1u;
    // The kind of the bin as 0 / 1 integers and masks, not conditions (a condition is a pair of SGPRs on the device, a wave's scarce
    // registers), and no branch on it either: a bin without a context reads and writes the spare byte behind the slice's states.
    // sel and n_states are below 2^15.
    const uint32_t bypass = is_zero(sel ^ (kIsCodes || !kWide ? 126u : 1024u));
    const uint32_t terminate = kIsCodes ? 0u : is_zero(sel ^ (kWide ? 1025u : 127u));
    const uint32_t context = kIsCodes ? 0u : (sel - n_states) >> 31;             // n_states <= form_max_states: never bypass or terminate as well
    const uint32_t cmask = 0u - context;
    const uint32_t at = (sel & cmask) | (n_states & ~cmask);
    uint32_t s = sel;
    if (!kIsCodes) s = (st.get(at) & 127u & cmask) | (126u & ~cmask);
    const TabEntry e = tab[s];
    const uint32_t lps = d.get(e.x, bypass, in);
    const uint32_t bin = ((s & 1u) & ~(0u - bypass)) ^ lps;
    if (!kIsCodes) st.set(at, (e.y >> (8 * lps)) & 0xffu & cmask);
    return (bin ^ want) | (kIsCodes ? 0u : (context | bypass | terminate) ^ 1u);
}

// One whole chunk, bins `first` .. : returns the index of the first bin whose decoded value differs from its record's, or `bad` if
// there is none or `bad` is set already.
template <int FORM, class Reader, class Store, class Table>
AVR_DIV_HD uint32_t decode_chunk(CabacDecoder &d, Reader &in, const Chunk16 &cur, Store &st, const Table &tab, uint32_t first,
                                 uint32_t n_states, uint32_t bad) {
    constexpr bool kWide = form_wide(FORM);
    constexpr uint32_t kN = form_per_chunk(FORM);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < kN; k++) {
        const uint32_t rec = kWide ? (cur.w[k >> 1] >> (16 * (k & 1))) & 0xffffu : (cur.w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        const uint32_t at = (first + k) | (decode_bin<FORM>(d, in, rec, st, tab, n_states) - 1u);    // AVR_VERIFY_NONE for a bin that is right
        bad = at < bad ? at : bad;                               // (the indices rise: the least is the first)
    }
    return bad;
}

// The first `valid` records of a slice's last chunk, where that is not a whole one: what lies behind them is padding and never
// looked at, whatever it holds.  A loop of its own over the chunk as one 128-bit number, the next record at its bottom.
template <int FORM, class Reader, class Store, class Table>
AVR_DIV_HD uint32_t decode_rest(CabacDecoder &d, Reader &in, const Chunk16 &cur, Store &st, const Table &tab, uint32_t first,
                                uint32_t valid, uint32_t n_states, uint32_t bad) {
    constexpr uint32_t kBits = form_wide(FORM) ? 16u : 8u;
    uint64_t lo = uint64_t(cur.w[0]) | uint64_t(cur.w[1]) << 32, hi = uint64_t(cur.w[2]) | uint64_t(cur.w[3]) << 32;
    for (uint32_t k = 0; k < valid; k++) {
        const uint32_t at = (first + k) | (decode_bin<FORM>(d, in, uint32_t(lo) & ((1u << kBits) - 1), st, tab, n_states) - 1u);
        bad = at < bad ? at : bad;
        lo = lo >> kBits | hi << (64 - kBits);
        hi >>= kBits;
    }
    return bad;
}

// The walk over one slice: bins 0 .. n_bins - 1 in order, in chunks from `src` (load(c): chunk c; every load is unconditional, its index
// clamped to the slice's last chunk, two chunks ahead -- what a clamped load returns is never decoded), the stream from `words` with
// `len` = min(out_len, capacity) bytes.  Returns the first bad bin or AVR_VERIFY_NONE; stops with the chunk that holds the first bad bin.
// A record at an index >= n_bins is never decoded.
template <int FORM, class Source, class Store, class Table>
AVR_DIV_HD uint32_t verify_slice(const uint64_t *words, uint32_t len, uint32_t n_bins, uint32_t n_states, const Source &src, Store &st,
                                 const Table &tab) {
    constexpr uint32_t kN = form_per_chunk(FORM);
    BitReader in;
    in.init(words, len);
    CabacDecoder d;
    d.init(in);
    const uint32_t n_whole = n_bins / kN, rest = n_bins % kN;
    const uint32_t n_chunks = n_whole + (rest ? 1u : 0u), last = n_chunks ? n_chunks - 1 : 0;
    Chunk16 cur = {{0, 0, 0, 0}}, nx1 = cur;
    if (n_chunks) { cur = src.load(0); nx1 = src.load(last < 1u ? last : 1u); }
    uint32_t bad = AVR_VERIFY_NONE;
    for (uint32_t c = 0; c < n_whole && bad == AVR_VERIFY_NONE; c++) {
        const Chunk16 nx2 = src.load(c + 2 < last ? c + 2 : last);
        bad = decode_chunk<FORM>(d, in, cur, st, tab, c * kN, n_states, bad);
        cur = nx1;
        nx1 = nx2;
    }
    if (bad == AVR_VERIFY_NONE) bad = decode_rest<FORM>(d, in, cur, st, tab, n_whole * kN, rest, n_states, bad);
    return bad;
}

// Where every bin decoded right and the caller gave the encoder's final states: the decoder's own states differing from them is
// reported at index n_bins, which no bin has.
AVR_DIV_HD uint32_t conclude(uint32_t bad, uint32_t n_bins, bool states_differ) {
    return bad == AVR_VERIFY_NONE && states_differ ? n_bins : bad;
}

}  // namespace cabac_verify
}  // namespace avr
