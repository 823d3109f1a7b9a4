// The decoder of the recoded coder, arithmetic_code<uint64_t, uint8_t>::decoder (arithmetic_code.h:209-298), for
// streams whose records are KNOWN: the verifier behind the K2 encoders (avr_verify.hip).
//
// Decoding an unknown stream is interleaved with H.264 syntax parsing and stays on the host (csrc/host/avr_host.h: range_decoder).
// At verify time every bin's K2 record -- {pos, neg} and the bin itself -- still lies on the device, so the decoder is handed
// (range / (pos + neg)) * pos exactly as the encoder was, decodes the bin and compares.  It shares nothing with the encoders' carry
// machinery: it never propagates a carry, never defers a digit and never runs finish(), which is what makes it an independent check
// of k_range_encode and of the three passes of K2p.
//
// `__host__ __device__` in the way avr_div.h and avr_k2p.h are: tests/range_verify_emul.cpp runs the very functions the kernel runs.
#pragma once
#include <stdint.h>

#include "avr_div.h"

#ifndef AVR_VERIFY_NONE
#define AVR_VERIFY_NONE 0xFFFFFFFFu
#endif

namespace avr {
namespace verify {

// The coded bytes of one slice, read in aligned 8-byte words (a region starts at a multiple of 8 and its capacity is one), one word
// ahead of the word in use.  Every byte at or beyond `len` reads as zero (arithmetic_code.h:279-288) whatever the region holds there:
// a word that starts at or past `len` is never loaded, the word that straddles it is masked.  len <= capacity, so no load leaves
// the region.
struct WordReader {
    const uint64_t *words;
    uint32_t len, widx, left;
    uint64_t acc, ahead;

    AVR_DIV_HD uint64_t load(uint32_t w) const {
        const uint64_t at = uint64_t(w) * 8;
        if (at >= len) return 0;
        const uint64_t v = words[w];                             // little endian: stream byte k of the word at bits 8k
        const uint32_t rem = len - uint32_t(at);
        return rem < 8 ? v & ((uint64_t(1) << (8 * rem)) - 1) : v;
    }
    AVR_DIV_HD void init(const uint64_t *p, uint32_t n) {
        words = p; len = n; widx = 0; left = 8;
        acc = load(0);
        ahead = load(1);
    }
    AVR_DIV_HD uint32_t next() {                                 // consume_digit_aligned, :279-288
        const uint32_t b = uint32_t(acc) & 0xffu;
        acc >>= 8;
        if (--left == 0) {
            acc = ahead;
            widx++;
            ahead = load(widx + 1);
            left = 8;
        }
        return b;
    }
};

// arithmetic_code.h:218-288 for <uint64_t, uint8_t>.  Invariant: low < range, from the constructor on and whatever the bytes are -- so
// the branch a bin takes never has range 0 (symbol 1 needs low >= r0, hence r1 = range - r0 > low - r0 >= 0; symbol 0 needs
// low < r0), and the renormalisation ends after at most seven digits.
struct RangeDecoder64 {
    static constexpr uint64_t kOne = uint64_t(1) << 63;          // fixed_one, :54-55
    uint64_t low, range;
    uint32_t next_digit;

    template <class Reader>
    AVR_DIV_HD void consume(Reader &in) {                        // :259-275: the stream is read one bit late
        const uint32_t in_digit = in.next();
        const uint32_t digit = ((next_digit << 7) | (in_digit >> 1)) & 0xffu;
        next_digit = in_digit;
        low = (low << 8) + digit;
        range <<= 8;
    }
    template <class Reader>
    AVR_DIV_HD void init(Reader &in) {                           // :218-230
        next_digit = in.next();
        low = next_digit / 2;                                    // digit_alignment == 2, :251-252
        range = 256 / 2;
        while (range < kOne) consume(in);
    }
    // :232-248 with the probability already evaluated: r1 = range_of_1
    template <class Reader>
    AVR_DIV_HD uint32_t get(uint64_t r1, Reader &in) {
        const uint64_t r0 = range - r1;
        const uint32_t symbol = low >= r0;
        low -= symbol ? r0 : 0;
        range = symbol ? r1 : r0;
        if (range < (uint64_t(1) << 51))                         // min_range, :61-62
            while (range - 1 < (uint64_t(1) << 55) - 1) consume(in);     // range < 2^55, and no turn at all for a range of 0
        return symbol;
    }
};

struct Chunk8 { uint32_t w[4]; };                                // eight two-byte K2 records

// One chunk: the operands of its eight bins (bin, pos, total, 1 / total) are fetched before the first bin is decoded, as
// k_range_encode does, so no table latency sits on the range -> range chain.  A padding record (pos + neg == 0) decodes as the no-op
// it is: quotient 0, r1 = 0, r0 = range, symbol 0.  Returns the index of the first bin whose decoded symbol differs from its record's
// (`first` + its place in the chunk), or `bad` if there is none or `bad` is set already.
template <class Reader, class InvTable>
AVR_DIV_HD uint32_t decode_chunk(RangeDecoder64 &d, Reader &in, const Chunk8 &cur, const InvTable &inv_d, uint32_t first, uint32_t bad) {
    uint32_t bin[8], pos[8], tot[8];
    double inv[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        const uint32_t rec = (cur.w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
        pos[k] = (rec >> 1) & 0x7f;
        tot[k] = pos[k] + ((rec >> 8) & 0x7f);                   // recode.cpp:825
        bin[k] = tot[k] ? rec & 1 : 0;
        inv[k] = inv_d[tot[k]];                                  // 0 for total 0
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        const uint64_t quot = div_u64_small_f64(d.range, double(tot[k]), inv[k]);
        const uint32_t symbol = d.get(quot * pos[k], in);        // recode.cpp:826
        if (symbol != bin[k] && bad == AVR_VERIFY_NONE) bad = first + uint32_t(k);
    }
    return bad;
}

// The walk over one slice: n_bins records in order, in chunks of eight from `src` (load(c): chunk c; every load is unconditional,
// its index clamped to the slice's last chunk, two chunks ahead -- what a clamped load returns is never decoded), the stream from
// `words` with `len` = min(out_len, capacity) bytes.  Returns the first bad bin or AVR_VERIFY_NONE.  The walk stops with the chunk
// that holds the first bad bin (a padding record never is one: it decodes to the 0 it is compared with).
template <class Source, class InvTable>
AVR_DIV_HD uint32_t verify_slice(const uint64_t *words, uint32_t len, uint32_t n_bins, const Source &src, const InvTable &inv_d) {
    WordReader in;
    in.init(words, len);
    RangeDecoder64 d;
    d.init(in);
    const uint32_t n_chunks = (n_bins + 7) >> 3, last = n_chunks ? n_chunks - 1 : 0;
    Chunk8 cur = {{0, 0, 0, 0}}, nx1 = cur;
    if (n_chunks) { cur = src.load(0); nx1 = src.load(last < 1u ? last : 1u); }
    uint32_t bad = AVR_VERIFY_NONE;
    for (uint32_t c = 0; c < n_chunks && bad == AVR_VERIFY_NONE; c++) {
        const Chunk8 nx2 = src.load(c + 2 < last ? c + 2 : last);
        bad = decode_chunk(d, in, cur, inv_d, c * 8, bad);
        cur = nx1;
        nx1 = nx2;
    }
    return bad;
}

}  // namespace verify
}  // namespace avr
