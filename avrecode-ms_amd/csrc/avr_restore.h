// The decompressor's epilogue as a comparison: does a coded K1 slice restore the payload it was made from?
//
// A slice's payload comes back as tail_patch(drop_stop_byte(K1(bins))) (avr_drop_stop_byte, avr_tail_patch; recode.cpp:1508-1512,
// :1354-1360), and the container carries two facts about the original payload: the parity of its length and its last byte.  This is
// that rule written once, for the restore check behind the K1 encoders (avr_restore.hip), as a function of bytes: `out[0..L)` the
// coded bytes, `exp[0..E)` the payload the compressor holds.
//
//   finish       L1 = L - 1 if L > 0 and out[L - 1] == 0x80, else L (one byte is dropped, never two)
//   tail patch   with the values the compressor writes into the container -- parity E & 1, last byte exp[E - 1], both only for E >= 2
//                (no last byte is recorded for a payload of one byte or none, and then nothing is patched):
//                  (L1 & 1) != (E & 1)   the restored bytes are out[0..L1) and the last byte behind them, R = L1 + 1
//                  otherwise             out[0..L1) with byte L1 - 1 replaced by the last byte (where L1 > 0), R = L1
//   answer       the smallest j < min(R, E) with restored[j] != exp[j]; else min(R, E) if R != E; else AVR_VERIFY_NONE
//
// Offered per aligned 8-byte word (both strings start at multiples of 8): the restored word with its special byte put in and everything
// at or past R zero, the expected word, and the mask of the bytes below min(R, E).  A word of `out` that starts at or past L is never
// loaded and the one that straddles L is masked; the same for `exp` and E, which is readable to the next multiple of 8.  Nothing of the
// encoders is in here, and nothing of avr_drop_stop_byte / avr_tail_patch either: the tests hold the two statements of the rule equal.
//
// `__host__ __device__` in the way avr_cabac_verify.h is: tests/restore_emul.cpp runs the very functions the kernel runs.
#pragma once
#include <stdint.h>

#include "avr_div.h"

#ifndef AVR_VERIFY_NONE
#define AVR_VERIFY_NONE 0xFFFFFFFFu
#endif

namespace avr {
namespace restore {

constexpr uint64_t kNoByte = ~uint64_t(0);

// What the rule makes of the two lengths and the two bytes it looks at.  Lengths are 64 bits wide: L may be 2^32 - 1 (a saturated
// region capacity) and R one more.
struct Shape {
    uint64_t L, E, R;                                            // coded bytes, expected bytes, restored bytes
    uint64_t n;                                                  // min(R, E): the bytes that are compared
    uint64_t at;                                                 // where the container's last byte goes, or kNoByte
    uint32_t last;                                               // that byte
};

// The rule from the two facts the container carries, where it carries them (`patch`): the parity of the payload's length and its last
// byte.  out_tail: out[L - 1] (unused for L == 0).  Nothing is expected here: E and n are 0.  (avr_finish.h copies by this shape.)
AVR_DIV_HD Shape tail_shape(uint32_t L, uint32_t out_tail, bool patch, uint32_t parity, uint32_t last) {
    Shape s;
    s.L = L;
    s.E = 0;
    const uint64_t L1 = L > 0 && (out_tail & 0xffu) == 0x80u ? uint64_t(L) - 1 : uint64_t(L);      // finish
    s.R = L1;
    s.at = kNoByte;
    s.last = last & 0xffu;
    if (patch) {                                                 // the tail patch
        if ((L1 & 1) != (parity & 1)) { s.at = L1; s.R = L1 + 1; }
        else if (L1 > 0) s.at = L1 - 1;
    }
    s.n = 0;
    return s;
}

// ... and from the expected payload, as the compressor derives the two facts: both only for E >= 2.
// out_tail: out[L - 1] (unused for L == 0); exp_tail: exp[E - 1] (unused for E < 2)
AVR_DIV_HD Shape make_shape(uint32_t L, uint32_t E, uint32_t out_tail, uint32_t exp_tail) {
    Shape s = tail_shape(L, out_tail, E >= 2, E & 1u, exp_tail);
    s.E = E;
    s.n = s.R < s.E ? s.R : s.E;
    return s;
}

AVR_DIV_HD uint64_t low_bytes(uint64_t k) { return k >= 8 ? ~uint64_t(0) : (uint64_t(1) << (8 * k)) - 1; }    // bytes 0 .. k - 1 of a word

// Word w of the restored payload (little endian: byte 8w + k at bits 8k), zero at and past R.
AVR_DIV_HD uint64_t restored_word(const uint64_t *out_words, uint64_t w, const Shape &s) {
    const uint64_t first = w * 8;
    uint64_t v = 0;
    if (first < s.L) v = out_words[w] & low_bytes(s.L - first);
    if (s.at != kNoByte && (s.at >> 3) == w) {
        const uint32_t sh = 8 * uint32_t(s.at & 7);
        v = (v & ~(uint64_t(0xff) << sh)) | uint64_t(s.last) << sh;
    }
    return first < s.R ? v & low_bytes(s.R - first) : 0;
}

// Word w of the expectation, zero at and past E.
AVR_DIV_HD uint64_t expected_word(const uint64_t *exp_words, uint64_t w, const Shape &s) {
    const uint64_t first = w * 8;
    return first < s.E ? exp_words[w] & low_bytes(s.E - first) : 0;
}

// The index of the first byte below n in which word w of the two strings differs, or AVR_VERIFY_NONE.
AVR_DIV_HD uint32_t word_first_diff(const uint64_t *out_words, const uint64_t *exp_words, uint64_t w, const Shape &s) {
    const uint64_t first = w * 8;
    if (first >= s.n) return AVR_VERIFY_NONE;
    const uint64_t x = (restored_word(out_words, w, s) ^ expected_word(exp_words, w, s)) & low_bytes(s.n - first);
    return x ? uint32_t(first) + (uint32_t(__builtin_ctzll(x)) >> 3) : AVR_VERIFY_NONE;       // n <= E < 2^32 - 1
}

// What lane `lane` of the wave that has the slice finds: words lane, lane + 64, ... in rising order, four to a step, up to its first
// difference.
AVR_DIV_HD uint32_t lane_first_diff(const uint64_t *out_words, const uint64_t *exp_words, const Shape &s, uint32_t lane) {
    const uint64_t n_words = (s.n + 7) >> 3;
    uint32_t best = AVR_VERIFY_NONE;
    for (uint64_t w0 = lane; w0 < n_words && best == AVR_VERIFY_NONE; w0 += 256) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t d = word_first_diff(out_words, exp_words, w0 + 64 * u, s);
            best = d < best ? d : best;
        }
    }
    return best;
}

// From the least of the lanes' answers to the slice's: where no compared byte differs, a difference of the lengths is reported at the
// shorter one's end.
AVR_DIV_HD uint32_t conclude(uint32_t best, const Shape &s) {
    return best != AVR_VERIFY_NONE ? best : s.R != s.E ? uint32_t(s.n) : AVR_VERIFY_NONE;
}

}  // namespace restore
}  // namespace avr
