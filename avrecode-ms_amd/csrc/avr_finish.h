// The decompressor's epilogue as a copy: from a slice's coded bytes to the bytes its NAL unit holds.
//
// avr_restore.h states the rule -- drop the stop byte, patch the tail -- as a comparison; this is the same shape (restore::tail_shape)
// as a source of bytes, with the last step behind it: emulation prevention (H.264 7.4.1), which changes lengths.
//
//   escape(p, n, z)   s = z (the zero bytes directly in front of the payload, at most 2).  For every byte b: where s == 2 and b <= 3,
//                     emit 0x03 and set s = 0; emit b; s = b == 0 ? s + 1 : 0.
//
// The state machine has three states, so a run of bytes is a function from entry state to (exit state, escapes): an Xfer.  Runs
// compose (`then`), a lane of the wave that has the slice takes one 8-byte word per trip, the wave composes its 64 Xfers by shuffles
// (avr_plan_dev.hip) and carries the concrete state and the count of escapes from trip to trip.  Pass 1 only counts, pass 2 writes:
// each lane knows the state its word is entered in and the escapes in front of it.
//
// Words are read aligned: `base` is the aligned 8-byte word that holds the slice's first byte, `skew` that byte's place in it.  No word
// is loaded that holds no byte of the slice's [0, L).
//
// `__host__ __device__` in the way avr_restore.h is: tests/finish_emul.cpp runs the very functions the kernels run.
#pragma once
#include <stdint.h>

#include "avr_div.h"
#include "avr_restore.h"

// one word per slice, as include/avrecode_ms_amd.h documents it (AVR_FINISH_WORD)
#define AVR_FINISH_LAST(f)    ((f) & 0xffu)
#define AVR_FINISH_PARITY(f)  (((f) >> 8) & 1u)
#define AVR_FINISH_PATCH(f)   (((f) >> 9) & 1u)
#define AVR_FINISH_ESCAPE(f)  (((f) >> 10) & 1u)
#define AVR_FINISH_ZEROS(f)   (((f) >> 11) & 3u)

namespace avr {
namespace finish {

using restore::kNoByte;
using restore::low_bytes;
using restore::Shape;

constexpr uint32_t kTripBytes = 512;                             // a wave's trip: 64 lanes, a word each

AVR_DIV_HD Shape shape_of(uint32_t L, uint32_t out_tail, uint32_t word) {
    return restore::tail_shape(L, out_tail, AVR_FINISH_PATCH(word) != 0, AVR_FINISH_PARITY(word), AVR_FINISH_LAST(word));
}
AVR_DIV_HD uint32_t zeros_before(uint32_t word) { const uint32_t z = AVR_FINISH_ZEROS(word); return z > 2 ? 2 : z; }

// Bytes [k, k + 8) of the slice (little endian), those at or past L zero.  Byte j of the slice is byte skew + j of base's bytes.
AVR_DIV_HD uint64_t slice_word(const uint64_t *base, uint32_t skew, uint64_t k, uint64_t L) {
    if (k >= L) return 0;
    const uint64_t a = skew + k, w = a >> 3;
    const uint32_t sk = uint32_t(a & 7);
    uint64_t v = base[w] >> (8 * sk);                            // holds byte k < L
    if (sk && k + 8 - sk < L) v |= base[w + 1] << (64 - 8 * sk); // begins with byte k + 8 - sk
    return v & low_bytes(L - k);
}

// Bytes [k, k + 8) of the finished payload before escaping: the stop byte gone, the special byte put in, zero at and past R.
AVR_DIV_HD uint64_t patched_word(const uint64_t *base, uint32_t skew, uint64_t k, const Shape &s) {
    if (k >= s.R) return 0;
    uint64_t v = slice_word(base, skew, k, s.L);
    if (s.at != kNoByte && s.at >= k && s.at - k < 8) {
        const uint32_t sh = 8 * uint32_t(s.at - k);
        v = (v & ~(uint64_t(0xff) << sh)) | uint64_t(s.last) << sh;
    }
    return v & low_bytes(s.R - k);
}

// Of the `words` 8-byte words that follow the first `head` bytes of the patched payload, how many at the front are the slice's own bytes
// as they lie: whole below the special byte, below L and below R.  The special byte is the last of the R bytes, so at most one word is
// left.
AVR_DIV_HD uint64_t plain_words(const Shape &s, uint64_t head, uint64_t words) {
    uint64_t lim = s.L < s.R ? s.L : s.R;
    if (s.at != kNoByte && s.at < lim) lim = s.at;
    const uint64_t n = lim > head ? (lim - head) >> 3 : 0;
    return n < words ? n : words;
}

// What a run of bytes does to each entry state s: the state it leaves (2 bits at 2 s) and the escapes it takes (10 bits at 10 s; a
// trip of 512 bytes takes 257 at the most).
struct Xfer { uint32_t exit, cnt; };

AVR_DIV_HD Xfer identity() { return Xfer{0u | 1u << 2 | 2u << 4, 0u}; }
AVR_DIV_HD uint32_t exit_of(const Xfer &x, uint32_t s) { return (x.exit >> (2 * s)) & 3u; }
AVR_DIV_HD uint32_t count_of(const Xfer &x, uint32_t s) { return (x.cnt >> (10 * s)) & 1023u; }

// the run of a, then the run of b
AVR_DIV_HD Xfer then(const Xfer &a, const Xfer &b) {
    Xfer r{0u, 0u};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t s = 0; s < 3; s++) {
        const uint32_t e = exit_of(a, s);
        r.exit |= exit_of(b, e) << (2 * s);
        r.cnt |= (count_of(a, s) + count_of(b, e)) << (10 * s);
    }
    return r;
}

// The first `n` <= 8 bytes of `word` as a run.  A byte above 3 forgets the entry state: from there on the three walks are one.
AVR_DIV_HD Xfer run_of(uint64_t word, uint32_t n) {
    uint32_t st[3] = {0, 1, 2}, cnt[3] = {0, 0, 0};
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t b = uint32_t(word >> (8 * j)) & 0xffu;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t s = 0; s < 3; s++) {
            if (st[s] == 2 && b <= 3) { cnt[s]++; st[s] = 0; }
            st[s] = b == 0 ? st[s] + 1 : 0;
        }
    }
    return Xfer{st[0] | st[1] << 2 | st[2] << 4, cnt[0] | cnt[1] << 10 | cnt[2] << 20};
}

// The first `n` <= 8 bytes of `word`, entered in state s, escaped to dst[at ...]; nothing is written at or past `end`.  Returns the
// bytes it made.
AVR_DIV_HD uint32_t emit_run(uint64_t word, uint32_t n, uint32_t s, uint8_t *dst, uint64_t at, uint64_t end) {
    const uint64_t from = at;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t b = uint32_t(word >> (8 * j)) & 0xffu;
        if (s == 2 && b <= 3) {
            if (at < end) dst[at] = 3;
            at++;
            s = 0;
        }
        if (at < end) dst[at] = uint8_t(b);
        at++;
        s = b == 0 ? s + 1 : 0;
    }
    return uint32_t(at - from);
}

// A slice's length behind the patch and the escapes: what pass 1 leaves for the scan.
AVR_DIV_HD uint64_t final_length(const Shape &s, uint64_t escapes) { return s.R + escapes; }

// How far a slice of L coded bytes can grow: one byte appended, then an escape for every two bytes, the first after 2 - z.
AVR_DIV_HD uint64_t max_length(uint64_t L, uint32_t z) { return L + 1 + (L + 1 + z) / 2; }

}  // namespace finish
}  // namespace avr
