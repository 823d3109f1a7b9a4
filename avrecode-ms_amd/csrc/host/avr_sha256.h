// SHA-256 (FIPS 180-4, sections 4.1.2, 4.2.2, 5.1.1, 5.3.3, 6.2), streaming, on the host: what the optional digest of a .recode file
// is made with (avr_host.h: Recoded::metadata) and checked with (avr_recode.h: decompressor::finish).  Plain C++17, no dependency:
// the command line and its CPU stand-in are the same code.
//
//     sha256 h;  h.update(p, n);  h.update(q, m);  std::string d = h.finish();      // 32 bytes; update() takes any split
//     std::string d = sha256::of(data, size);
//
// Not a hot path: the bytes are in host memory on their way to or from a file, and the command line around it runs at a fraction
// of what a scalar SHA-256 does (DESIGN.md section 6 has the figures).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

namespace avr {
namespace host {

class sha256 {
  public:
    static constexpr size_t DIGEST_BYTES = 32, BLOCK_BYTES = 64;

    sha256() { reset(); }
    void reset() {                                       // 5.3.3: the first 32 bits of the fractional parts of the square roots of the first 8 primes
        static const uint32_t h0[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
        memcpy(h_, h0, sizeof h_);
        bytes_ = 0;
        held_ = 0;
    }
    void update(const void *data, size_t size) {
        const uint8_t *p = static_cast<const uint8_t *>(data);
        bytes_ += size;
        if (held_) {                                     // fill up the block begun by an earlier call
            const size_t n = size < BLOCK_BYTES - held_ ? size : BLOCK_BYTES - held_;
            if (n) memcpy(block_ + held_, p, n);
            held_ += n; p += n; size -= n;
            if (held_ < BLOCK_BYTES) return;
            compress(block_);
            held_ = 0;
        }
        for (; size >= BLOCK_BYTES; p += BLOCK_BYTES, size -= BLOCK_BYTES) compress(p);
        if (size) memcpy(block_, p, size);
        held_ = size;
    }
    // 5.1.1: a one bit, zero bits up to 448 mod 512, the message length in bits as 64 bits, big endian.  The object is spent
    // afterwards (reset() starts another message).
    std::string finish() {
        const uint64_t bits = bytes_ * 8;
        block_[held_++] = 0x80;
        if (held_ > BLOCK_BYTES - 8) {
            memset(block_ + held_, 0, BLOCK_BYTES - held_);
            compress(block_);
            held_ = 0;
        }
        memset(block_ + held_, 0, BLOCK_BYTES - 8 - held_);
        for (int i = 0; i < 8; i++) block_[BLOCK_BYTES - 8 + i] = uint8_t(bits >> (56 - 8 * i));
        compress(block_);
        std::string out(DIGEST_BYTES, '\0');
        for (size_t i = 0; i < DIGEST_BYTES; i++) out[i] = char(uint8_t(h_[i / 4] >> (24 - 8 * (i % 4))));
        return out;
    }
    static std::string of(const void *data, size_t size) {
        sha256 h;
        h.update(data, size);
        return h.finish();
    }
    static std::string of(const std::string &s) { return of(s.data(), s.size()); }

  private:
    static uint32_t rotr(uint32_t x, int n) { return x >> n | x << (32 - n); }
    void compress(const uint8_t *m) {                    // 6.2.2, one 512-bit block
        // 4.2.2: the first 32 bits of the fractional parts of the cube roots of the first 64 primes
        static const uint32_t k[64] = {
            0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
            0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
            0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
            0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
            0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
            0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
            0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
            0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
        uint32_t w[64];
        for (int t = 0; t < 16; t++) w[t] = uint32_t(m[4 * t]) << 24 | uint32_t(m[4 * t + 1]) << 16 | uint32_t(m[4 * t + 2]) << 8 | uint32_t(m[4 * t + 3]);
        for (int t = 16; t < 64; t++) {
            const uint32_t s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ w[t - 15] >> 3;      // sigma0, 4.1.2
            const uint32_t s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ w[t - 2] >> 10;        // sigma1
            w[t] = s1 + w[t - 7] + s0 + w[t - 16];
        }
        uint32_t a = h_[0], b = h_[1], c = h_[2], d = h_[3], e = h_[4], f = h_[5], g = h_[6], h = h_[7];
        for (int t = 0; t < 64; t++) {
            const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + k[t] + w[t];   // Sigma1, Ch
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));             // Sigma0, Maj
            h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h_[0] += a; h_[1] += b; h_[2] += c; h_[3] += d; h_[4] += e; h_[5] += f; h_[6] += g; h_[7] += h;
    }

    uint32_t h_[8];
    uint64_t bytes_;
    size_t held_;                                        // bytes of block_ in use, < BLOCK_BYTES between calls
    uint8_t block_[BLOCK_BYTES];
};

}  // namespace host
}  // namespace avr
