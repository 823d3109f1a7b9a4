// K1p: intra-slice parallel CABAC encode (the same bytes as K1, i.e. as cabac::encoder of
// /root/reference/cabac_code.h:26-82 on arithmetic_code.h, from many lanes per slice).
//
// Why a slice can be cut at all.  The reference codes a slice strictly serially
// (arithmetic_code.h:107-114: every bin narrows [low, low+range)).  But CABAC's arithmetic is
// exactly decomposable:
//   (1) context states evolve per context, independent of low/range (cabac_code.h:43-47);
//       phase A resolves them and rewrites every bin as a one-byte RESOLVED code
//           c = (s << 1) | bin   context bin coded in state s = 2*pStateIdx + valMPS, s <= 125
//           252, 253             bypass bin 0 / 1 (the slot of state 126, never a real context
//                                state: pStateIdx 63 is only reached by put_terminate)
//           254, 255             state 127 = (pStateIdx 63, valMPS 1) with bin 0 / 1: the table row
//                                of pStateIdx 63 is "LPS range 2" in every quarter, which is exactly
//                                put_terminate (cabac_code.h:57-67): terminate(b) is code 255 - b,
//                                and so is a context bin met at pStateIdx 63 with symbol b
//       so that for every non-bypass code  symbol = ((c >> 1) ^ c) & 1  and  row = rows[c >> 2];
//   (2) range, written R << norm with R in [256, 511] (what cabac_code.h:37-41 recomputes per
//       bin), is a finite-state chain over R that forgets its past at every coded LPS: after
//       an LPS R is rangeTabLPS[p][q] renormalised, so only the quarter q (2 bits) of the range
//       before that LPS matters.  A STRETCH runs from just after an LPS to the first LPS at or
//       past the next multiple of kChunk bins; phase B1 walks every stretch for the 4 possible
//       entry quarters (they merge within a few bins), phase B2 chains the 4->4 maps per slice
//       (serial, one table look-up per stretch) and so fixes every stretch's entry range and
//       its bit position T (total renormalisation shifts before it);
//   (3) low is a sum of per-bin terms at known bit positions (arithmetic_code.h:110), so phase
//       C codes each stretch with low = 0 from its true entry range, aligned to the global
//       16-bit digit grid, and ADDS its digits into a per-slice array of 32-bit digit sums;
//       phase D adds the carries up once, serially from the last digit, and applies the
//       reference's finish() (arithmetic_code.h:128-144) to the exact final (low, range).
//
// Everything below is `__host__ __device__`: the kernels in avr_k1p.hip are thin per-lane
// wrappers, and tests/k1p_emul.cpp runs the very same functions on the CPU (test build only).
#pragma once
#include <stdint.h>

#include "avr_chunk.h"

#if defined(__HIPCC__)
#define AVR_HD __host__ __device__ inline
#else
#define AVR_HD inline
#endif

namespace avr {
namespace k1p {

// Keep a value where it is computed (an empty asm statement the optimiser cannot look through): used to
// make a batch of independent LDS table reads issue together, ahead of the dependent arithmetic --
// hipcc otherwise sinks each read to its use, behind the previous bin's result, and every bin waits
// out a full LDS latency.
#if defined(__HIP_DEVICE_COMPILE__)
#define AVR_PIN2(a, b) asm volatile("" : "+v"(a), "+v"(b))
#else
#define AVR_PIN2(a, b) ((void)0)
#endif

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kMaxStretch = 16 * kChunk;  // a longer stretch sends the slice to the serial kernel
constexpr uint32_t kCodeBypass = 252;
constexpr uint32_t kCodePad = 252;             // padding of a resolved stream's last 16-byte group

struct alignas(16) U4 { uint32_t x, y, z, w; };

AVR_HD int clz32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz(x);
#else
    return x ? __builtin_clz(x) : 32;
#endif
}

// ---- phase A: one chunk's step of a context's state chain (k_k1p_ctxchain, k_k1p_chain_seg, k_k1p_chain_fix)
//
// k_k1p_tn's table, tn[tn_section(n) + (st << n | bits)], is the state after the n = 0 .. 8 bins `bits` (first bin in the low bit)
// from state st.  A run of `left` bins goes through it as  left % 8 bins first, by the section of that n (the identity for n = 0,
// which is also what a lane without bins reads), then whole bytes by the section of n = 8: the index of a whole byte is
// st << 8 | byte behind a constant, and which byte of the run it is is known when the code is written, so a whole byte costs one
// bit-field extract for all NS states and one shift-or per state.  Every look-up after the first is taken only by the lanes that
// have it, and only while some lane of the wave has it (AVR_ANY: on the CPU a lane is alone).
#if defined(__HIP_DEVICE_COMPILE__)
#define AVR_ANY(x) __any(x)
#define AVR_PIN1(a) asm volatile("" : "+v"(a))
#else
#define AVR_ANY(x) (x)
#define AVR_PIN1(a) ((void)0)
#endif
AVR_HD constexpr uint32_t tn_section(uint32_t n) { return (128u << n) - 128u; }
// Entry i of the table, i < tn_section(9), bin by bin (cabac_code.h:43-47); packed: CabacTables::packed, whose [s][1] is the state
// after an MPS in state s in its low byte and after an LPS in the next.
AVR_HD uint8_t tn_entry(uint32_t i, const uint32_t (*packed)[2]) {
    const uint32_t n = 31u - uint32_t(clz32((i >> 7) + 1)), j = i - tn_section(n);
    uint32_t st = j >> n;
    for (uint32_t b = 0; b < n; b++) {
        const uint32_t nx = packed[st][1], bin = (j >> b) & 1u;
        st = ((bin ^ st) & 1u) ? (nx >> 8) & 0xffu : nx & 0xffu;
    }
    return uint8_t(st);
}
// bits 32 (pos / 32) .. + 127 of a chunk's bit string: the window a run from bit `pos` starts in
AVR_HD U4 chain_window(const uint32_t *bw, uint32_t pos) {
    const uint32_t wi = (pos >> 5) & (kChunkBitDwords - 1);      // (past the last dword: the next chunk's, never used -- a run ends by bit kChunk)
    return U4{bw[wi], bw[wi + 1], bw[wi + 2], bw[wi + 3]};
}
// bits sh .. sh + 31 of hi:lo, sh < 32
AVR_HD uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
    return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
#endif
}
// Whole bytes first .. first + COUNT - 1 of the run, out of `avail` (some lane has byte `first`); true: some lane has more.
template <int NS, int COUNT>
AVR_HD bool chain_bytes(const uint8_t *tn, uint32_t avail, uint32_t first, uint32_t whole, uint32_t (&st)[NS]) {
#pragma unroll
    for (int i = 0; i < COUNT; i++) {
        if (i && !AVR_ANY(whole > first + i)) return false;
        if (whole > first + i) {
            const uint32_t byte = (avail >> (8 * i)) & 0xffu;
#pragma unroll
            for (int q = 0; q < NS; q++) st[q] = tn[tn_section(8) + (st[q] << 8 | byte)];
        }
    }
    return AVR_ANY(whole > first + COUNT);
}
// The context's `left` bins of the chunk are bits [pos, pos + left) of the chunk's bit string `bw` (pos + left <= kChunk; readable
// up to dword kChunkBitDwords); w: its four dwords from dword pos / 32 on, which hold the run's first 96 bins at least.  NS states
// at once, side by side.
template <int NS>
AVR_HD void chain_step(const uint8_t *tn, const uint32_t *bw, uint32_t pos, uint32_t left, const U4 &w, uint32_t (&st)[NS]) {
    const uint32_t sh = pos & 31u, rem = left & 7u, whole = left >> 3;
    const uint32_t b0 = funnel(w.y, w.x, sh);
    uint32_t off = tn_section(rem) + (b0 & ((1u << rem) - 1u));  // all of the index that does not wait for the state
    AVR_PIN1(off);                                               // (kept whole: the compiler would split it up again)
#pragma unroll
    for (int q = 0; q < NS; q++) st[q] = tn[(st[q] << rem) + off];
    if (!AVR_ANY(whole != 0)) return;
    const uint32_t b1 = funnel(w.z, w.y, sh);                    // the whole bytes start rem bins into the run
    if (!chain_bytes<NS, 4>(tn, funnel(b1, b0, rem), 0, whole, st)) return;
    const uint32_t b2 = funnel(w.w, w.z, sh);
    if (!chain_bytes<NS, 4>(tn, funnel(b2, b1, rem), 4, whole, st)) return;
    if (!chain_bytes<NS, 3>(tn, b2 >> rem, 8, whole, st)) return;         // 96 - rem bins of the window: eleven whole bytes
    for (uint32_t first = 11;; first += 4) {                     // a run of more than that: fetched as it goes
        const uint32_t at = pos + rem + 8 * first, wi = (at >> 5) & (kChunkBitDwords - 1);   // (a lane without the byte: any dword of the string)
        if (!chain_bytes<NS, 4>(tn, funnel(bw[wi + 1], bw[wi], at & 31u), first, whole, st)) return;
    }
}

// ---- resolved codes
AVR_HD uint32_t code_sym(uint32_t c) { return ((c >> 1) ^ c) & 1u; }
AVR_HD bool code_is_bypass(uint32_t c) { return (c >> 1) == 126u; }
// a coded "LPS" (symbol 1 on a non-bypass bin): the range after it depends on q only
AVR_HD bool code_is_boundary(uint32_t c) { return code_sym(c) && !code_is_bypass(c); }
// resolved code of put_terminate(b) and of a context bin met in state s (sym = bin ^ valMPS)
AVR_HD uint32_t code_terminate(uint32_t b) { return 255u - b; }
AVR_HD uint32_t code_context(uint32_t s, uint32_t bin) { return s >= 126 ? 255u - ((bin ^ s) & 1u) : (s << 1) | bin; }

// Range (9-bit, normalised) right after a boundary bin coded from quarter q, and its shift.
AVR_HD uint32_t post_lps_range(uint32_t row, uint32_t q, uint32_t *shift) {
    const uint32_t rl = (row >> (8 * q)) & 0xffu;
    const uint32_t sh = uint32_t(clz32(rl)) - 23;          // rl << sh in [256, 511]
    *shift = sh;
    return rl << sh;
}

// What phases B and C need to know about a resolved code, precomputed per code value (256 entries):
//   row   rangeTabLPS[p][0..3] of its state, one byte per range quarter (0 for a bypass bin)
//   meta  bit 0: the coded symbol (1 = the LPS side, cabac_code.h:34; 0 for bypass, whose halving of
//         the scale, cabac_code.h:52-54, is the extra shift instead); bit 1: the bin adds to low
//         (the symbol again, or for bypass the bin); bit 8: bypass
struct CodeEntry { uint32_t row, meta; };
AVR_HD CodeEntry code_entry(uint32_t c, const uint32_t *rows /* rows[p], p = pStateIdx */) {
    if (code_is_bypass(c)) return CodeEntry{0u, 0x100u | ((c & 1u) << 1)};
    return CodeEntry{rows[c >> 2], code_sym(c) * 3u};
}

// One bin on the normalised range, branch-free: returns the renormalisation shift it causes
// (= bits of output).  A bypass bin has row 0: rLPS = 0 leaves R alone, and meta adds its one shift.
// Either side's renormalisation is "shift the new range up to nine bits" (the MPS side's range - rLPS lies in [128, 511]:
// one shift iff below 256; the LPS side's is rLPS itself, cabac_code.h:40-41), so the side is chosen first and one count of
// leading zeros serves both.
AVR_HD int clz32_nz(uint32_t x) { return __builtin_clz(x); }   // x != 0
// rangeTabLPS[p][(range >> 6) & 3] out of the state's row (one byte per quarter), range in [256, 511]
AVR_HD uint32_t lps_range(uint32_t row, uint32_t R) {
#if defined(__HIP_DEVICE_COMPILE__)
    // one byte permute: range >> 6 is 4 .. 7, which as a selector means bytes 0 .. 3 of the first operand; the selector's
    // other three bytes are 0 = byte 0 of the second operand, the constant 0
    return __builtin_amdgcn_perm(row, 0u, R >> 6);
#else
    return (row >> ((R >> 3) & 24)) & 0xffu;
#endif
}
AVR_HD uint32_t mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}
AVR_HD uint32_t step_range(const CodeEntry &e, uint32_t *R) {
    const uint32_t rl = lps_range(e.row, *R);
    const uint32_t rm = *R - rl;                           // MPS side: range - rLPS
    const uint32_t x = (e.meta & 1u) ? rl : rm;            // never 0: a coded LPS has rLPS >= 2, rm >= 128
    const uint32_t sh = uint32_t(clz32_nz(x)) - 23;
    *R = x << sh;
    return sh + (e.meta >> 8);
}

// The same entry laid out for the inner loops (16 bytes, one LDS read), every field an operand as it stands:
//   side   all ones for a coded symbol 1 (the LPS side), else 0: the new range is a bit-field insert of rLPS over range - rLPS
//   k      what the bin adds to low, in half units, as a factor of range - rLPS: 2 for a coded symbol 1 (cabac_code.h:37-39),
//          1 for a bypass 1 (:52-54: the range itself, rLPS being 0 there), 0 otherwise
//   adj    bypass - 23: leading zeros of the new range + adj = the bits the bin shifts out
struct alignas(16) CodeEntryC { uint32_t row, side, k, adj; };
AVR_HD CodeEntryC code_entry_c(const CodeEntry &e) {
    const uint32_t sym = e.meta & 1u, adds = (e.meta >> 1) & 1u, byp = e.meta >> 8;
    return CodeEntryC{e.row, sym ? ~0u : 0u, adds ? (byp ? 1u : 2u) : 0u, byp - 23u};
}
// One bin: the new range, what it adds to low (*v), returns the shift (the range's own: *sh0)
AVR_HD uint32_t step_range_c(const CodeEntryC &e, uint32_t *R, uint32_t *v) {
    const uint32_t rl = lps_range(e.row, *R);
    const uint32_t rm = *R - rl;
    const uint32_t x = (rl & e.side) | (rm & ~e.side);
    const uint32_t lz = uint32_t(clz32_nz(x));
    *v = mul24(rm, e.k);
    *R = x << (lz - 23);
    return lz + e.adj;
}

// ------------------------------------------------------------------ phase B1

struct Stretch {
    uint32_t first;          // index of the boundary bin that opens the stretch (kNone: chunk inactive;
                             // chunk 0 is always active and starts at bin 0 with R = 510)
    uint32_t end;            // one past the stretch's last bin
    uint32_t t_exit[4];      // shifts inside the stretch, per entry quarter
    uint16_t r_exit[4];      // normalised range after the last bin, per entry quarter
    uint8_t exit_q;          // quarter seen by the closing boundary bin, 2 bits per entry quarter
    uint8_t too_long;        // stretch exceeded kMaxStretch: the slice goes to the serial kernel
    uint8_t pad[2];
};

// Where a slice's resolved codes are read from: load16(i), i a multiple of 16, gives codes i .. i+15; byte(i) one code.
// LinearCodes: the slice's codes in a row (the layout of the public entry points: 16-byte aligned, readable up to the
// next multiple of 16).  The kernels have a second one for their own, wave-interleaved buffer (avr_k1p.hip).
struct LinearCodes {
    const uint8_t *p;
    AVR_HD U4 load16(uint32_t i) const { return *reinterpret_cast<const U4 *>(p + i); }
    AVR_HD uint32_t byte(uint32_t i) const { return p[i]; }
};

// Visit the resolved codes [from .. n) of `src` in order, 16 bytes per load.  f(i, code) returns true to stop.
template <class Src, class F>
AVR_HD void for_codes_in(const Src &src, uint32_t from, uint32_t n, F &&f) {
    for (uint32_t base = from & ~15u; base < n; base += 16) {
        const U4 v = src.load16(base);
        uint32_t w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t d = w0;
            w0 = w1; w1 = w2; w2 = w3;
            const uint32_t i = base + 4 * k;
            // (i + b - from) < (n - from) is "from <= i + b < n" in one unsigned compare
            if (i + 0 - from < n - from && f(i + 0, d & 0xffu)) return;
            if (i + 1 - from < n - from && f(i + 1, (d >> 8) & 0xffu)) return;
            if (i + 2 - from < n - from && f(i + 2, (d >> 16) & 0xffu)) return;
            if (i + 3 - from < n - from && f(i + 3, d >> 24)) return;
        }
    }
}
template <class F>
AVR_HD void for_codes(const uint8_t *res, uint32_t from, uint32_t n, F &&f) { for_codes_in(LinearCodes{res}, from, n, f); }

// The same for codes that all get the same treatment: g(code) for every code of res[from .. to), no
// index, no early exit.  The bulk is taken 64 bytes per lane per trip (four 16-byte loads issued
// together): lanes stream from addresses a kilobyte apart, so a 16-byte load drags in a whole
// cache line per lane and nothing keeps it resident until the lane comes back for the rest.
template <class G, class G4>
AVR_HD void for_codes_all(const uint8_t *res, uint32_t from, uint32_t to, G &&g, G4 &&g4) {
    if (from >= to) return;
    auto group16 = [&](const U4 &v) {
        uint32_t w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t d = w0;
            w0 = w1; w1 = w2; w2 = w3;
            g4(d);                                         // four codes, first in the low byte
        }
    };
    // code by code up to a 16-byte boundary, 16-byte groups up to a cache line, then lines, and back down
    const uint32_t head_end = ((from + 15) & ~15u) < to ? ((from + 15) & ~15u) : to;
    for_codes(res, from, head_end, [&](uint32_t, uint32_t c) { g(c); return false; });
    uint32_t base = head_end;
    for (; (base & 63) && base + 16 <= to; base += 16) group16(*reinterpret_cast<const U4 *>(res + base));
    if (base + 64 <= to) {                                 // the next line is in flight while this one is worked on
        const U4 *p = reinterpret_cast<const U4 *>(res + base);
        U4 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
        for (; base + 64 <= to; base += 64) {
            const U4 *q = reinterpret_cast<const U4 *>(res + (base + 128 <= to ? base + 64 : base));   // unconditional: see c_stretch_in
            const U4 n0 = q[0], n1 = q[1], n2 = q[2], n3 = q[3];
            group16(v0); group16(v1); group16(v2); group16(v3);
            v0 = n0; v1 = n1; v2 = n2; v3 = n3;
        }
    }
    for (; base + 16 <= to; base += 16) group16(*reinterpret_cast<const U4 *>(res + base));
    if (base < to) for_codes(res, base, to, [&](uint32_t, uint32_t c) { g(c); return false; });
}

// The table entries of the four codes in a dword, read together (see AVR_PIN2).
AVR_HD void code_entries4(const CodeEntry *codes, uint32_t d, CodeEntry e[4]) {
    e[0] = codes[d & 0xffu]; e[1] = codes[(d >> 8) & 0xffu]; e[2] = codes[(d >> 16) & 0xffu]; e[3] = codes[d >> 24];
    AVR_PIN2(e[0].row, e[0].meta); AVR_PIN2(e[1].row, e[1].meta); AVR_PIN2(e[2].row, e[2].meta); AVR_PIN2(e[3].row, e[3].meta);
}
AVR_HD void code_entries4(const CodeEntryC *codes, uint32_t d, CodeEntryC e[4]) {
    e[0] = codes[d & 0xffu]; e[1] = codes[(d >> 8) & 0xffu]; e[2] = codes[(d >> 16) & 0xffu]; e[3] = codes[d >> 24];
    AVR_PIN2(e[0].row, e[0].side); AVR_PIN2(e[1].row, e[1].side); AVR_PIN2(e[2].row, e[2].side); AVR_PIN2(e[3].row, e[3].side);
}

AVR_HD void b1_stretch(const uint8_t *res, uint32_t n, uint32_t chunk, const CodeEntry *codes, uint32_t max_stretch,
                       Stretch *o) {
    const uint32_t lo = chunk_start(chunk), limit = chunk_start(chunk + 1);   // limit: not clamped to n
    uint32_t R[4], T[4] = {0, 0, 0, 0};
    uint32_t i;
    o->too_long = 0;
    o->exit_q = 0;
    o->pad[0] = o->pad[1] = 0;
    if (chunk == 0) {
        o->first = 0;                                      // opens at bin 0 with the initial range 510 (cabac_code.h:30)
        R[0] = R[1] = R[2] = R[3] = 510;
        i = 0;
    } else {
        uint32_t f = kNone;
        const uint32_t hi = limit < n ? limit : n;
        for_codes(res, lo, hi, [&](uint32_t idx, uint32_t c) { if (code_is_boundary(c)) { f = idx; return true; } return false; });
        if (f == kNone) {
            o->first = kNone; o->end = 0;
            for (int q = 0; q < 4; q++) { o->t_exit[q] = 0; o->r_exit[q] = 0; }
            return;
        }
        o->first = f;
        const uint32_t row = codes[res[f]].row;
        for (uint32_t q = 0; q < 4; q++) { uint32_t sh; R[q] = post_lps_range(row, q, &sh); }
        i = f + 1;
    }
    // Until the four candidates have merged.  That takes a while -- on config 2 a mean of 66 bins, and the
    // slowest of a wave's 64 lanes needs about 240 -- so the part of it that lies inside the chunk, where
    // no bin can close the stretch, is walked 16 codes per load like the merged part.
    bool closed = false;
    auto merged = [&]() { return R[0] == R[1] && R[1] == R[2] && R[2] == R[3]; };
    auto code_by_code = [&](uint32_t stop) {               // up to `stop`, or merged, or closed
        if (i >= stop) return;
        uint32_t i_next = stop;
        for_codes(res, i, stop, [&](uint32_t idx, uint32_t c) {
            if (merged()) { i_next = idx; return true; }
            const bool closing = idx >= limit && code_is_boundary(c);
            if (closing)
                for (uint32_t q = 0; q < 4; q++) o->exit_q |= uint8_t(((R[q] >> 6) & 3) << (2 * q));
            const CodeEntry e = codes[c];
            for (uint32_t q = 0; q < 4; q++) T[q] += step_range(e, &R[q]);
            i_next = idx + 1;
            if (closing) { closed = true; return true; }
            return false;
        });
        i = i_next;
    };
    {
        const uint32_t interior_end = limit < n ? limit : n;
        const uint32_t a16 = (i + 15) & ~15u;
        code_by_code(a16 < interior_end ? a16 : interior_end);
        while (!merged() && i + 16 <= interior_end) {      // i is a multiple of 16 here
            const U4 v = *reinterpret_cast<const U4 *>(res + i);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
            for (uint32_t k = 0; k < 4; k++) {
                CodeEntry e[4];
                code_entries4(codes, w[k], e);
                for (uint32_t b = 0; b < 4; b++)
                    for (uint32_t q = 0; q < 4; q++) T[q] += step_range(e[b], &R[q]);
            }
            i += 16;
        }
        code_by_code(n);
    }
    // merged: one range, 16 codes per load.  Below `limit` no bin can close the stretch.
    uint32_t Rm = R[0], Tm = 0, end = i;
    if (!closed && i < n) {
        const uint32_t interior_end = limit < n ? limit : n;
        if (i < interior_end) {
            for_codes_all(res, i, interior_end, [&](uint32_t c) { Tm += step_range(codes[c], &Rm); },
                          [&](uint32_t d) {
                              CodeEntry e[4];
                              code_entries4(codes, d, e);
                              Tm += step_range(e[0], &Rm); Tm += step_range(e[1], &Rm);
                              Tm += step_range(e[2], &Rm); Tm += step_range(e[3], &Rm);
                          });
            i = interior_end;
        }
        end = n;
        for_codes(res, i, n, [&](uint32_t idx, uint32_t c) {
            const bool closing = idx >= limit && code_is_boundary(c);
            if (closing) o->exit_q = uint8_t(((Rm >> 6) & 3) * 0x55u);
            Tm += step_range(codes[c], &Rm);
            if (closing) { end = idx + 1; return true; }
            if (idx - lo > max_stretch) { o->too_long = 1; end = idx + 1; return true; }
            return false;
        });
        R[0] = R[1] = R[2] = R[3] = Rm;
    }
    o->end = end;
    for (uint32_t q = 0; q < 4; q++) { o->t_exit[q] = T[q] + Tm; o->r_exit[q] = uint16_t(R[q]); }
}

// ---- phase B1 as the kernels walk it (k_k1p_replay, k_k1p_b1): B1Walk.  b1_stretch above stays the CPU's statement of the result;
// tests/b1walk_emul.cpp runs this code on the host, group by group, and holds every field of Stretch to it.

struct alignas(8) U2 { uint32_t x, y; };

// v_perm_b32 as far as it is used here: byte i of the result is byte sel[i] of s0:s1 (0 .. 3: s1's bytes, 4 .. 7: s0's), zero for sel[i] = 12
AVR_HD uint32_t perm_b32(uint32_t s0, uint32_t s1, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(s0, s1, sel);
#else
    const uint64_t both = uint64_t(s0) << 32 | s1;
    uint32_t r = 0;
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t b = (sel >> (8 * i)) & 0xffu;
        if (b < 8) r |= uint32_t((both >> (8 * b)) & 0xffu) << (8 * i);
    }
    return r;
#endif
}
// The packed 16-bit operations: two values to a register, each half on its own (a shift takes the low four bits of its count).
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
AVR_HD uint32_t pk_sub(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b)); }
AVR_HD uint32_t pk_add(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b)); }
AVR_HD uint32_t pk_shl(uint32_t a, uint32_t b) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) << __builtin_bit_cast(u16x2, b)); }
AVR_HD uint32_t pk_shr(uint32_t a, uint32_t n) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) >> __builtin_bit_cast(u16x2, n * 0x00010001u)); }
#else
AVR_HD uint32_t pk_halves(uint32_t lo, uint32_t hi) { return (lo & 0xffffu) | hi << 16; }
AVR_HD uint32_t pk_sub(uint32_t a, uint32_t b) { return pk_halves((a & 0xffffu) - (b & 0xffffu), (a >> 16) - (b >> 16)); }
AVR_HD uint32_t pk_add(uint32_t a, uint32_t b) { return pk_halves((a & 0xffffu) + (b & 0xffffu), (a >> 16) + (b >> 16)); }
AVR_HD uint32_t pk_shl(uint32_t a, uint32_t b) { return pk_halves((a & 0xffffu) << (b & 15u), (a >> 16) << ((b >> 16) & 15u)); }
AVR_HD uint32_t pk_shr(uint32_t a, uint32_t n) { return pk_halves((a & 0xffffu) >> n, (a >> 16) >> n); }
#endif

// A bin as B1Walk takes it, 16 bytes and one LDS read: { x: the LPS ranges of its state's four range quarters, y: next | code << 8 |
// meta << 16 (next: what k_k1p_replay keeps there, the context's state after the bin), z, w: CodeEntryC's side and adj }.
AVR_HD U4 b1_entry(const CodeEntry &ce, uint32_t next, uint32_t code) {
    const CodeEntryC cc = code_entry_c(ce);
    return U4{ce.row, next | code << 8 | ce.meta << 16, cc.side, cc.adj};
}
// per code, for the candidates' LPS side: { x: low byte of post_lps_range per range quarter, y: its shift per quarter }
AVR_HD U2 codes2_entry(uint32_t row) {
    U2 r{0, 0};
    for (uint32_t q = 0; q < 4; q++) {
        if (!((row >> (8 * q)) & 0xffu)) continue;
        uint32_t sh;
        const uint32_t rn = post_lps_range(row, q, &sh);
        r.x |= (rn & 0xffu) << (8 * q);
        r.y |= sh << (8 * q);
    }
    return r;
}

// B1's four candidate ranges, two to a register (16 bits each), stepped with the packed 16-bit instructions: a range in [256, 511]
// shifted down by six is 4 .. 7, which as a byte selector means the bytes of the first operand and, in the half's other byte, 0 = byte 0
// of the second.  So one byte permute picks each candidate's LPS range out of the state's row by the candidate's own quarter, and
// the LPS side (the range renormalised, whose bit 8 is the second operand's 1; its shift) comes out of the two rows of codes2 the same
// way instead of a count of leading zeros per candidate.  Both sides are computed and `side` (all ones: the LPS side) picks by bit,
// never by a branch: the candidates of a wave's lanes take either side at nearly every bin.
// One bin on a pair of candidates (step_range, twice): returns the two shifts, packed, without a bypass bin's own.
AVR_HD uint32_t step_pair(uint32_t &Rp, uint32_t row, uint32_t rown, uint32_t shrow, uint32_t side) {
    const uint32_t sel = pk_shr(Rp, 6);
    const uint32_t rl = perm_b32(row, 0u, sel);
    const uint32_t rm = pk_sub(Rp, rl);                              // MPS side: range - rLPS, in [128, 511]
    const uint32_t shm = pk_shr(rm, 8) ^ 0x00010001u;                // one shift iff below 256
    const uint32_t rn = perm_b32(rown, 1u, sel);                     // LPS side, renormalised: in [256, 511]
    const uint32_t shl = perm_b32(shrow, 0u, sel);
    Rp = (rn & side) | (pk_shl(rm, shm) & ~side);
    return (shl & side) | (shm & ~side);
}

// A chunk's stretch summary from its bins in order, eight at a time.
// mode: 0 = looking for the LPS that opens the stretch, 1 = four candidate ranges, 2 = they have met, 3 = closed.
// Inside the chunk (group_inside: all eight bins below i1) nothing can close the stretch and no path has a branch per bin:
//   merged8   mode 2: step_range_c on the one range left;
//   cand8     mode 1: step_pair on both pairs, the rows of codes2 read four bins at a time;
//   open8     mode 0, and mode 1 beside it: the bin that opens the stretch is the first set bit of the group's boundary bits; every
//             bin is stepped as in cand8 and at the opening bin the candidates are set from its row of codes2 and the shifts so
//             far dropped, by select.
// A wave takes each path some lane of it needs.
// Past the chunk (tail) a merged lane closes at the first boundary bin: tail8 finds it in the boundary bits -- or the bin by which
// the stretch is too long, or the slice's last -- and steps the bins up to it by select.
// one(), the bin-by-bin form of all of it, is left with what is rare: the last group of a slice's last chunk when the slice does not end
// on a multiple of eight (and that chunk's group of padding after it), and in the tail a lane whose candidates have not met.
struct B1Walk {
    uint32_t i0, i1, limit, n, max_stretch;
    const U2 *codes2;
    // Candidates 0, 1 in Rp0 (low, high half), 2, 3 in Rp1; Tp: their shifts since the last flush; T: before it.  Once they have met
    // (join) the one range left is all of Rp0 and its shifts go to T[0], T[1 .. 3] being what candidates 1 .. 3 had shifted more than
    // candidate 0 by then: a merged lane needs no registers of its own for them.
    uint32_t mode, Rp0, Rp1, Tp0, Tp1, T[4], end;
    bool merged;
    Stretch o;

    AVR_HD void init(uint32_t chunk, uint32_t i0_, uint32_t i1_, uint32_t n_, uint32_t max_stretch_, const U2 *codes2_) {
        i0 = i0_; i1 = i1_; limit = i0_ + kChunk; n = n_; max_stretch = max_stretch_; codes2 = codes2_;
        mode = 0; Rp0 = Rp1 = 0x01fe01feu; Tp0 = Tp1 = 0; T[0] = T[1] = T[2] = T[3] = 0; end = 0;
        merged = false;
        o.first = kNone; o.end = 0; o.exit_q = 0; o.too_long = 0; o.pad[0] = o.pad[1] = 0;
        for (int q = 0; q < 4; q++) { o.t_exit[q] = 0; o.r_exit[q] = 0; }
        if (chunk == 0) { o.first = 0; Rp0 = 510; mode = 2; merged = true; }    // opens at bin 0 with the initial range 510 (cabac_code.h:30)
    }
    // at least every 8 bins: 8 x 9 shifts fit 16 bits with room.  byp: the bypass bins among them, one shift each, where Tp has them not
    AVR_HD void flush_t(uint32_t byp = 0) {
        T[0] += (Tp0 & 0xffffu) + byp; T[1] += (Tp0 >> 16) + byp; T[2] += (Tp1 & 0xffffu) + byp; T[3] += (Tp1 >> 16) + byp;
        Tp0 = Tp1 = 0;
    }
    AVR_HD bool met() const { return Rp0 == Rp1 && (Rp0 >> 16) == (Rp0 & 0xffffu); }
    // the candidates have met (Tp flushed: the differences are taken on all their shifts so far)
    AVR_HD void join() { Rp0 &= 0xffffu; T[1] -= T[0]; T[2] -= T[0]; T[3] -= T[0]; mode = 2; merged = true; }
    AVR_HD void open(uint32_t rown) {                            // post_lps_range for the four quarters
        Rp0 = perm_b32(rown, 1u, 0x00050004u);
        Rp1 = perm_b32(rown, 1u, 0x00070006u);
    }
    AVR_HD uint32_t step_merged(const U4 &e) {                   // step_range on the one range left
        uint32_t v;
        return step_range_c(CodeEntryC{e.x, e.z, 0u, e.w}, &Rp0, &v);
    }
    AVR_HD void one(uint32_t idx, const U4 &e) {                 // bin idx (< n), any mode
        const bool boundary = (e.y >> 16) & 1u;                  // a coded LPS (code_is_boundary)
        if (mode == 0) {
            if (idx < i1 && boundary) { o.first = idx; open(codes2[(e.y >> 8) & 0xffu].x); mode = 1; }
        } else if (mode == 1) {
            const bool closing = idx >= limit && boundary;
            if (closing)
                o.exit_q |= uint8_t(((Rp0 >> 6) & 3u) | ((Rp0 >> 22) & 3u) << 2 | ((Rp1 >> 6) & 3u) << 4 | ((Rp1 >> 22) & 3u) << 6);
            const U2 e2 = codes2[(e.y >> 8) & 0xffu];
            const uint32_t extra = (e.y >> 24) * 0x00010001u;    // a bypass bin's one shift
            Tp0 = pk_add(Tp0, step_pair(Rp0, e.x, e2.x, e2.y, e.z) + extra);
            Tp1 = pk_add(Tp1, step_pair(Rp1, e.x, e2.x, e2.y, e.z) + extra);
            if (closing) { end = idx + 1; mode = 3; }
            else if (met()) { flush_t(); join(); }
        } else if (mode == 2) {
            const bool closing = idx >= limit && boundary;
            if (closing) o.exit_q = uint8_t(((Rp0 >> 6) & 3) * 0x55u);
            T[0] += step_merged(e);
            if (closing) { end = idx + 1; mode = 3; }
            else if (idx >= limit && idx - i0 > max_stretch) { o.too_long = 1; end = idx + 1; mode = 3; }
        }
    }
    AVR_HD void merged8(const U4 e[8]) {
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) T[0] += step_merged(e[j]);
    }
    AVR_HD void rows4(const U4 e[4], U2 r[4]) const {            // four rows of codes2, read together and waited for once
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) r[j] = codes2[(e[j].y >> 8) & 0xffu];
        AVR_PIN2(r[0].x, r[0].y); AVR_PIN2(r[1].x, r[1].y); AVR_PIN2(r[2].x, r[2].y); AVR_PIN2(r[3].x, r[3].y);
    }
    AVR_HD void cand8(const U4 e[8]) {
        uint32_t w = 8 * 23u;                                    // adj is bypass - 23: the sum counts the bypass bins
#pragma unroll
        for (uint32_t h = 0; h < 8; h += 4) {
            U2 r[4];
            rows4(e + h, r);
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                Tp0 = pk_add(Tp0, step_pair(Rp0, e[h + j].x, r[j].x, r[j].y, e[h + j].z));
                Tp1 = pk_add(Tp1, step_pair(Rp1, e[h + j].x, r[j].x, r[j].y, e[h + j].z));
                w += e[h + j].w;
            }
        }
        flush_t(w);
        // candidates that have met stay together: looking once per group is enough, and the group's shifts are in T[] either way
        if (met()) join();
    }
    AVR_HD void open8(uint32_t base, const U4 e[8]) {
        uint32_t bm = 0;                                         // bit j: bin j is a coded LPS
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) bm |= e[j].z & (1u << j);
        // the bin that opens the stretch; 8: none of these; kNone: it is open already
        const uint32_t at = mode == 0 ? uint32_t(__builtin_ctz(bm | 0x100u)) : kNone;
        uint32_t w = 0;
#pragma unroll
        for (uint32_t h = 0; h < 8; h += 4) {                    // (a lane that is still looking steps the ranges it was set up with: any will do)
            U2 r[4];
            rows4(e + h, r);
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                Tp0 = pk_add(Tp0, step_pair(Rp0, e[h + j].x, r[j].x, r[j].y, e[h + j].z));
                Tp1 = pk_add(Tp1, step_pair(Rp1, e[h + j].x, r[j].x, r[j].y, e[h + j].z));
                w += e[h + j].w + 23u;
                const bool here = at == h + j;
                Rp0 = here ? perm_b32(r[j].x, 1u, 0x00050004u) : Rp0;
                Rp1 = here ? perm_b32(r[j].x, 1u, 0x00070006u) : Rp1;
                Tp0 = here ? 0u : Tp0; Tp1 = here ? 0u : Tp1; w = here ? 0u : w;
            }
        }
        if (at < 8) { o.first = base + at; mode = 1; }
        if (mode == 1) {
            flush_t(w);
            if (met()) join();                                   // (in the opening group itself, too)
        } else {
            Tp0 = Tp1 = 0;
        }
    }
    // bins base .. base+7, all of them below i1.  any_looking: some lane of those that walk side by side is in mode 0 (a lane alone:
    // this one).  A wave whose lanes have all merged skips the rest by the branch hipcc puts around a block no lane enters.
    AVR_HD void group_inside_as(uint32_t base, const U4 e[8], bool any_looking) {
        if (mode == 2) merged8(e);
        else if (any_looking) open8(base, e);
        else cand8(e);
    }
    AVR_HD void group_inside(uint32_t base, const U4 e[8]) { group_inside_as(base, e, AVR_ANY(mode == 0)); }
    AVR_HD void group(uint32_t base, const U4 e[8]) {            // bins base .. base+7 of the chunk, as many of them as the slice has
        if (base + 8 <= i1) {
            group_inside(base, e);
        } else if (mode != 3) {
            for (uint32_t j = 0; j < 8; j++) if (base + j < n) one(base + j, e[j]);
            flush_t();
        }
    }
    AVR_HD void chunk_done() { if (mode == 0) mode = 3; }        // no LPS in the chunk: no stretch opens here (first stays kNone)
    // Past the chunk, mode 2, base < n: every index is at or beyond `limit`, so the stretch ends with the first bin that is a coded LPS
    // or lies more than max_stretch bins from i0, that bin stepped like the ones before it; failing both it runs on to the slice's end.
    AVR_HD void tail8(uint32_t base, const U4 e[8]) {
        uint32_t bm = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) bm |= e[j].z & (1u << j);
        const uint32_t closes = uint32_t(__builtin_ctz(bm | 0x100u));                     // 8: no bin of these
        const uint32_t d = base - i0, far = max_stretch >= d ? max_stretch - d + 1 : 0;   // first j with base + j - i0 > max_stretch
        const uint32_t left = n - base - 1 < 7u ? n - base - 1 : 7u;                     // the group's last bin that the slice has
        const uint32_t stop = closes < far ? closes : far, last = stop < left ? stop : left;
        uint32_t before = Rp0;                                   // the range before bin `last`
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const bool on = j <= last;
            uint32_t r = Rp0, v;
            const uint32_t sh = step_range_c(CodeEntryC{e[j].x, e[j].z, 0u, e[j].w}, &r, &v);
            before = on ? Rp0 : before;
            Rp0 = on ? r : Rp0;
            T[0] += on ? sh : 0u;
        }
        if (last == closes) { o.exit_q = uint8_t(((before >> 6) & 3) * 0x55u); end = base + last + 1; mode = 3; }
        else if (last == far) { o.too_long = 1; end = base + last + 1; mode = 3; }
    }
    AVR_HD void tail(uint32_t base, const U4 e[8]) {             // past the chunk, until the stretch closes
        if (base >= n) return;                                   // (k_k1p_b1 comes with the second half of its sixteen codes whatever n is)
        if (mode == 2) {
            tail8(base, e);
        } else {
            for (uint32_t j = 0; j < 8; j++) if (base + j < n && mode != 3) one(base + j, e[j]);
            flush_t();
        }
    }
    AVR_HD const Stretch &finish() {
        if (o.first != kNone) {
            o.end = mode != 3 ? n : end;                         // not closed: ran to the end of the slice
            for (uint32_t q = 0; q < 4; q++) {                   // once merged, the one range carried on for all four candidates
                const uint32_t rq = ((q & 2u) ? Rp1 : Rp0) >> (16 * (q & 1u)) & 0xffffu;
                o.t_exit[q] = merged && q ? T[0] + T[q] : T[q];
                o.r_exit[q] = uint16_t(merged ? Rp0 : rq);
            }
        }
        return o;
    }
};

// ---- the replay's state chain (k_k1p_replay's `eight` and `eight8`): replay_step8.  tests/replay_step_emul.cpp runs it on the host
// against the plain loop per bin (state byte -> table entry -> write-back).
//
// Eight bins of one lane: col = the lane's state column (a byte per context), off[j] = where bin j's state byte lives in it (sel_off's
// value; the pseudo contexts too), bin[j] its bin, info[state << 1 | bin] = b1_entry (next state in byte 0 of .y).  e[j] = bin j's
// entry, and the column is left as the plain loop leaves it.
// Read as written the loop is two dependent LDS round trips a bin: bin j+1's state byte may be the one bin j writes.  Here bin j+1's
// byte is read together with bin j's entry, BEFORE bin j's write-back, and taken only where the two bins' offsets differ; where they
// are equal the next state of bin j is handed on in a register.  LDS operations of a wave complete in issue order, so that read sees
// every write up to bin j-1's: one round trip a bin.
//
// The states of a column: a context's 7-bit state (pStateIdx << 1 | valMPS), and the pseudo states of what is no context of the
// batch -- bypass, terminate, padding, none -- which never move.
constexpr uint32_t kStBypass = 128, kStTerminate = 129, kStPad = 130, kStNone = 131, kReplayStates = 132;

AVR_HD void replay_step8(uint8_t *col, const uint32_t off[8], const uint32_t bin[8], const U4 *info, U4 e[8]) {
    uint32_t st = col[off[0]];
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        e[j] = info[(st << 1) | bin[j]];
        uint32_t ahead = 0;
        if (j < 7) ahead = col[off[j + 1]];
        const uint32_t next = e[j].y & 0xffu;
        col[off[j]] = uint8_t(next);
        if (j < 7) st = off[j + 1] == off[j] ? next : ahead;
    }
}

// ------------------------------------------------------------------ phase B2 (one lane per slice)

struct Entry {             // what phase C needs per active stretch
    uint32_t t_start;        // shifts before the stretch = bit position of its first output bit
    uint32_t q;              // entry quarter
};

struct SliceTotals {
    uint32_t t_total;        // shifts over the whole slice
    uint32_t r_final;        // normalised range after the last bin
    uint32_t bad;            // 1: a stretch was too long
    uint32_t pad;
};

AVR_HD void b2_chain(const Stretch *st, uint32_t n_chunks, Entry *en, SliceTotals *tot) {
    uint32_t T = 0, q = 0, r = 510, bad = 0;
    for (uint32_t c = 0; c < n_chunks; c++) {
        if (st[c].first == kNone) continue;
        en[c].t_start = T;
        en[c].q = q;
        T += st[c].t_exit[q];
        r = st[c].r_exit[q];
        bad |= st[c].too_long;
        q = (st[c].exit_q >> (2 * q)) & 3;
    }
    tot->t_total = T;
    tot->r_final = r;
    tot->bad = bad;
    tot->pad = 0;
}

// Number of 16-bit digits the reference has produced (emitted or deferred) after t shifts:
// its range is R << (22 - t + 16 nd) and a digit is produced whenever that exponent would
// drop below 1 (min_range 0x200, cabac_code.h:22, arithmetic_code.h:115-122).
AVR_HD uint32_t ref_digits(uint32_t t) { return t <= 21 ? 0 : (t - 21 + 15) / 16; }

// ------------------------------------------------------------------ phase C (one lane per active stretch)

// Digit sums: 32-bit per 16-bit digit of the slice's code string.  `Adder` supplies
//   void store(uint32_t digit_index, uint32_t v)   exclusive position, plain store; called with consecutive indices
//   void add(uint32_t digit_index, uint32_t v)     shared position, atomic add
//   void flush()                                   no store() follows: whatever the adder holds back goes out
// A stretch shares its first two digits with the windows of earlier stretches and its final
// window (two digits) with later ones; everything between is its own (argument in DESIGN.md).
// An adder may take the stretch's digits itself instead of one store() / add() each, by offering (kStaged = true)
//   void begin(uint32_t g0)                        the index of the stretch's first digit
//   void push(uint32_t i, uint32_t v)              digit i, after digit i - 1; one lane's call, anywhere
//   void push2(uint32_t nd, uint32_t a, uint32_t b)   the next nd = 0, 1 or 2 digits: a, then b; unconditional work only
//   void look(uint32_t i)                          after a push2, i = index of the next digit: the place to make room, reached
//                                                  by a wave's lanes together; at most one push2 between two looks
//   void flush(uint32_t i)                         in place of flush()
// and has to bring about the same sums: add for digits g0 and g0 + 1, exclusive positions after them.
//
// The coder is kept in normalised form: R in [256, 511] as in B1, and low as a 64-bit integer L2 in
// units of half the reference's scale, i.e. with the reference's range R << e (arithmetic_code.h:107-114,
// cabac_code.h:37-41) L2 = 2 * low >> e, which is exact: every term of low is a multiple of the
// scale it was added at, and a bypass bin's R/2 (cabac_code.h:52-54) is what the factor 2 is for.
// A 16-bit digit of the code string is due whenever e drops to 0 or below (arithmetic_code.h:115-122);
// in this form that is just a bit position `sp` = 15 - e of L2/2 reaching 15.  Nothing forces the
// digit out at that very bin: L2 has room for 4 more bins, so the bulk loop looks after every 4th
// bin, at the same place for every lane of a wave -- where the reference's form has one lane or
// another emitting at almost every bin.  A digit taken late has the carries of the bins in between
// already in it (it can reach 2^17); the sums are integers and phase D carries them on.
//
// The look of the bulk loop has no loop and no branch of its own.  Four bins shift by at most 28 and a look leaves
// sp <= 14, so with s1 = sp + 1 in [-6, 43] there are nd = max(0, s1 >> 4) = 0, 1 or 2 digits due, and for nd > 0 the bits
// that stay are the low ks = 16 + (s1 & 15) = s1 - 16 (nd - 1).  Both digits come off in one shift, t = L2 >> ks: the
// older one is t >> 16 with every carry above it (nd == 2) or t itself (nd == 1), the younger t & 0xffff.  What stays fits
// 32 bits: for nd > 0 it is below 2^31, and for nd == 0 the coder's interval [L2, L2 + 2 R) lies inside the one the last
// look left, below 2^(16 + s1') + 2^10 with s1' >= 0, scaled by the d = s1 - s1' <= 15 shifts since: L2 < 2^(s1 + 16) +
// 2^(10 + d) < 2^32 (before the stretch's first digit L2 + 2 R <= 2 * 510 << d with d <= s1 + 6 <= 21).
template <class A, class = void> struct adder_is_staged { static constexpr bool value = false; };
template <class A> struct adder_is_staged<A, decltype(void(A::kStaged))> { static constexpr bool value = A::kStaged; };
template <class Src, class Adder>
AVR_HD void c_stretch_in(const Src &src, const Stretch &st, const Entry &en, uint32_t chunk,
                         const CodeEntryC *codes, Adder &S) {
    uint32_t R, from;
    if (chunk == 0) { R = 510; from = 0; }
    else { uint32_t sh; R = post_lps_range(codes[src.byte(st.first)].row, en.q, &sh); from = st.first + 1; }
    const uint32_t phase = en.t_start & 15, g0 = en.t_start >> 4;
    uint64_t L2 = 0;
    int sp = int(phase) - 7;                               // e = 22 - phase at the start (cabac_code.h:30 shifted onto the digit grid)
    uint32_t j = 0;                                        // digits produced
    constexpr bool staged = adder_is_staged<Adder>::value;
    if constexpr (staged) S.begin(g0);
    auto bin_e = [&](const CodeEntryC &e) {
        uint32_t v;
        const uint32_t sh = step_range_c(e, &R, &v);
        L2 = (L2 + v) << sh;
        sp += int(sh);
    };
    auto bin = [&](uint32_t c) { bin_e(codes[c]); };
    auto put = [&](uint32_t d) {                           // the stretch's next digit
        if constexpr (staged) S.push(g0 + j, d);
        else if (j < 2) S.add(g0 + j, d);
        else S.store(g0 + j, d);
        j++;
    };
    auto digits = [&]() {                                  // every digit that is due, oldest (topmost) first
        while (sp >= 15) {
            const uint32_t d = uint32_t(L2 >> (sp + 1));
            L2 &= (uint64_t(2) << sp) - 1;
            put(d);
            sp -= 16;
        }
    };
    auto digits2 = [&]() {                                 // the same after four bins of the bulk: see above
        const int s1 = sp + 1;
        const uint32_t nd = uint32_t(s1 > 0 ? s1 : 0) >> 4, ks = 16 + (uint32_t(s1) & 15u);
        const uint64_t t = L2 >> ks;
        const uint32_t a = nd == 2 ? uint32_t(t >> 16) : uint32_t(t), b = uint32_t(t) & 0xffffu;
        L2 = uint32_t(L2) & (nd ? (1u << ks) - 1 : ~0u);
        sp -= int(16 * nd);
        if constexpr (staged) { S.push2(nd, a, b); j += nd; S.look(g0 + j); }
        else { if (nd) put(a); if (nd == 2) put(b); }
    };
    const uint32_t to = st.end;
    if (from < to) {
        auto four = [&](uint32_t d) {                      // 4 bins shift by at most 28: sp <= 14 + 28, L2 < 2^61
            CodeEntryC e[4];
            code_entries4(codes, d, e);
            bin_e(e[0]); bin_e(e[1]); bin_e(e[2]); bin_e(e[3]);
            digits2();
        };
        auto group16 = [&](const U4 &v) { four(v.x); four(v.y); four(v.z); four(v.w); };
        // code by code up to a 16-byte boundary, 16-byte groups up to a cache line, then lines, and back down
        const uint32_t head_end = ((from + 15) & ~15u) < to ? ((from + 15) & ~15u) : to;
        for_codes_in(src, from, head_end, [&](uint32_t, uint32_t c) { bin(c); digits(); return false; });
        uint32_t base = head_end;
        for (; (base & 63) && base + 16 <= to; base += 16) group16(src.load16(base));
        U4 v0{0, 0, 0, 0}, v1 = v0, v2 = v0, v3 = v0;
        if (base + 64 <= to) { v0 = src.load16(base); v1 = src.load16(base + 16); v2 = src.load16(base + 32); v3 = src.load16(base + 48); }
        for (; base + 64 <= to; base += 64) {              // a whole cache line per lane per trip, the next one in flight
            const uint32_t w[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
            // the next line unconditionally (past the last whole line: this one again, a hit) -- a load inside a branch is waited for at the branch's end
            const uint32_t nb = base + 128 <= to ? base + 64 : base;
            v0 = src.load16(nb); v1 = src.load16(nb + 16); v2 = src.load16(nb + 32); v3 = src.load16(nb + 48);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
#endif
            for (uint32_t k = 0; k < 16; k++) four(w[k]);
        }
        for (; base + 16 <= to; base += 16) group16(src.load16(base));
        if (base < to) for_codes_in(src, base, to, [&](uint32_t, uint32_t c) { bin(c); digits(); return false; });
    }
    if constexpr (staged) S.flush(g0 + j);
    else S.flush();
    // what is left is the coder's window: the top of digit g0 + j (with any carry) and 15 - e bits of the next
    if (sp >= 0) {
        S.add(g0 + j, uint32_t(L2 >> (sp + 1)));
        S.add(g0 + j + 1, uint32_t(L2 & ((uint64_t(2) << sp) - 1)) << (15 - sp));
    } else {
        S.add(g0 + j, uint32_t(L2 << (-sp - 1)) );
    }
}

template <class Adder>
AVR_HD void c_stretch(const uint8_t *res, const Stretch &st, const Entry &en, uint32_t chunk,
                      const CodeEntryC *codes, Adder &S) {
    c_stretch_in(LinearCodes{res}, st, en, chunk, codes, S);
}

// ------------------------------------------------------------------ phase D (one lane per slice)

// finish() of arithmetic_code<uint32_t,uint16_t,0x200>::encoder (arithmetic_code.h:128-144) on the
// exact final window.  Returns the carry it sends into the digits and the bytes it appends.
AVR_HD uint32_t d_finish(uint32_t low, uint32_t range, uint8_t tail[5], uint32_t *carry) {
    for (uint32_t stop = 1u << 30; stop > 0; stop >>= 1) {         // :131-137
        const uint32_t x = (low | stop) & ~(stop - 1);
        if (stop < range && low <= x && x < uint32_t(low + range)) { low = x; break; }
    }
    uint32_t n = 0, cy = 0;
    while (low != 0 && n < 5) {                                    // :139-142
        if (low >= 0x80000000u) { cy = 1; low -= 0x80000000u; }
        const uint32_t d = low >> 23;
        tail[n++] = uint8_t(d);
        low = (low - (d << 23)) << 8;
    }
    *carry = cy;
    return n;
}

// S: the slice's digit sums (ref_digits(t_total) + 2 entries are read).  Writes the final byte
// string to out (capacity cap) and returns its length.
AVR_HD uint32_t d_slice(const uint32_t *S, const SliceTotals &tot, uint8_t *out, uint32_t cap) {
    const uint32_t nd = ref_digits(tot.t_total);
    // the reference's final low: the two window digits, with whatever carry bit they hold
    const uint32_t low = uint32_t((uint64_t(S[nd]) << 15) + (S[nd + 1] >> 1));
    const uint32_t range = tot.r_final << (22 - tot.t_total + 16 * nd);
    uint8_t tail[5];
    uint32_t carry;
    const uint32_t n_tail = d_finish(low, range, tail, &carry);
    for (uint32_t i = nd; i-- > 0;) {                              // add the carries up, last digit first
        const uint32_t v = S[i] + carry;
        carry = v >> 16;
        if (2 * i + 1 < cap) { out[2 * i] = uint8_t(v >> 8); out[2 * i + 1] = uint8_t(v); }
    }
    for (uint32_t k = 0; k < n_tail; k++)
        if (2 * nd + k < cap) out[2 * nd + k] = tail[k];
    return 2 * nd + n_tail;
}

}  // namespace k1p
}  // namespace avr
