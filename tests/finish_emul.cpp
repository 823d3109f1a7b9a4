// The epilogue kernels of avr_plan_dev.hip on the CPU: the functions of csrc/avr_finish.h called lane by lane and trip by trip, in the
// order k_finish_lengths and k_finish_copy call them, on heap buffers of exactly the bytes the kernels may touch (this program is built
// with AddressSanitizer and UBSan by tests/test_finish_emul.py).
//
//   finish_emul                self-check against the byte-by-byte rule written below: every string of length <= 8 over {0, 1, 3, 4, 0x80},
//                              with and without a trailing 0x80, times every finish word of the table (no patch; patch x parity x a
//                              few last bytes; each plain and escaped at every z); and short strings laid over every lane and trip
//                              seam of a longer slice
//   finish_emul cases IN OUT   IN: lines of `hex-bytes word skew dst_skew` ("-" for no bytes); OUT: the finished bytes in hex, a line
//                              each -- for the test's comparison with the oracle's epilogue and its own escape
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "avr_finish.h"

using namespace avr::finish;
typedef std::vector<uint8_t> Bytes;

// ------------------------------------------------------------------ the rule, byte by byte
static Bytes plain(const Bytes &out, uint32_t word) {
    Bytes p = out;
    if (!p.empty() && p.back() == 0x80) p.pop_back();
    if ((word >> 9) & 1) {
        const uint8_t last = uint8_t(word & 0xff);
        if ((p.size() & 1) != ((word >> 8) & 1)) p.push_back(last);
        else if (!p.empty()) p.back() = last;
    }
    if (!((word >> 10) & 1)) return p;
    uint32_t s = (word >> 11) & 3;
    if (s > 2) s = 2;
    Bytes e;
    for (uint8_t b : p) {
        if (s == 2 && b <= 3) { e.push_back(3); s = 0; }
        e.push_back(b);
        s = b == 0 ? s + 1 : 0;
    }
    return e;
}

// ------------------------------------------------------------------ the kernels, emulated
struct View {                                                    // what a wave knows of its slice (FinishSlice of avr_plan_dev.hip)
    const uint64_t *base;
    uint32_t skew, word;
    Shape shape;
};
struct Slice : View {
    uint64_t *mem;                                               // exactly the aligned words that hold a byte of the slice
    Slice(const uint8_t *out, size_t n, uint32_t skew_) {
        const size_t n_words = (skew_ + n + 7) / 8;
        mem = static_cast<uint64_t *>(malloc(n_words ? n_words * 8 : 1));
        memset(mem, 0xEE, n_words * 8);
        if (n) memcpy(reinterpret_cast<uint8_t *>(mem) + skew_, out, n);
        base = mem;
        skew = skew_;
        tail = n ? out[n - 1] : 0u;
        L = uint32_t(n);
    }
    const View &under(uint32_t word_) {                          // the same bytes under another finish word
        word = word_;
        shape = shape_of(L, tail, word_);
        return *this;
    }
    ~Slice() { free(mem); }
    uint32_t L, tail;
};

static bool g_network = true;                                    // compose by the shuffle network of the kernel, or in lane order

// finish_walk<kWrite> of avr_plan_dev.hip.  By the network, all 64 lanes take every step the kernel's take; in lane order only the lanes
// that hold a byte are walked (an empty run is the identity, and there is nothing for it to write).
static uint64_t walk(const View &f, bool write, uint8_t *dst, uint64_t end) {
    uint32_t z = zeros_before(f.word);
    uint64_t escapes = 0;
    const uint64_t R = f.shape.R;
    for (uint64_t k0 = 0; k0 < R; k0 += kTripBytes) {
        uint64_t word[64];
        uint32_t n[64];
        Xfer inc[64], ex[64];
        const uint32_t lanes = g_network || R - k0 >= kTripBytes ? 64u : uint32_t((R - k0 + 7) / 8);
        for (uint32_t lane = 0; lane < lanes; lane++) {
            const uint64_t k = k0 + 8u * lane;
            n[lane] = k < R ? (R - k < 8 ? uint32_t(R - k) : 8u) : 0u;
            word[lane] = n[lane] ? patched_word(f.base, f.skew, k, f.shape) : 0;
            inc[lane] = run_of(word[lane], n[lane]);
        }
        if (g_network) {
            for (uint32_t d = 1; d < 64; d <<= 1) {
                Xfer front[64];
                for (uint32_t lane = 0; lane < 64; lane++) front[lane] = inc[lane >= d ? lane - d : lane];
                for (uint32_t lane = d; lane < 64; lane++) inc[lane] = then(front[lane], inc[lane]);
            }
        } else {
            for (uint32_t lane = 1; lane < lanes; lane++) inc[lane] = then(inc[lane - 1], inc[lane]);
        }
        for (uint32_t lane = 0; lane < lanes; lane++) ex[lane] = lane ? inc[lane - 1] : identity();
        if (write)
            for (uint32_t lane = 0; lane < lanes; lane++)
                emit_run(word[lane], n[lane], exit_of(ex[lane], z), dst, k0 + 8u * lane + escapes + count_of(ex[lane], z), end);
        escapes += count_of(inc[lanes - 1], z);
        z = exit_of(inc[lanes - 1], z);
    }
    return escapes;
}

// k_finish_lengths
static uint64_t length_of(const View &f) {
    const uint64_t len = final_length(f.shape, AVR_FINISH_ESCAPE(f.word) ? walk(f, false, nullptr, 0) : 0);
    if (len > max_length(f.shape.L, zeros_before(f.word))) { printf("a slice of %llu bytes grew to %llu\n", (unsigned long long)f.shape.L, (unsigned long long)len); exit(1); }
    return len;
}

// k_finish_copy: dst[0, len), dst at dst_skew modulo 8
static void copy_to(const View &f, uint8_t *dst, uint32_t dst_skew, uint64_t len) {
    if (AVR_FINISH_ESCAPE(f.word)) {
        walk(f, true, dst, len);
        return;
    }
    const uint64_t to_word = (8u - (dst_skew & 7u)) & 7u, head = to_word < len ? to_word : len;
    for (uint32_t lane = 0; lane < 64 && lane < head; lane++) dst[lane] = uint8_t(patched_word(f.base, f.skew, 0, f.shape) >> (8 * lane));
    const uint64_t words = (len - head) >> 3, tail = (len - head) & 7u;
    const uint64_t plain = plain_words(f.shape, head, words);                                    // the words k_compact_wide's loop takes
    const uint32_t skew = uint32_t((f.skew + head) & 7u);
    const uint64_t *sw = f.base + ((f.skew + head) >> 3);
    for (uint32_t lane = 0; lane < 64; lane++) {
        for (uint64_t w = lane; w < plain; w += 64) {
            const uint64_t v = skew ? sw[w] >> (8 * skew) | sw[w + 1] << (64 - 8 * skew) : sw[w];
            memcpy(dst + head + 8 * w, &v, 8);
        }
        for (uint64_t w = plain + lane; w < words; w += 64) {
            const uint64_t v = patched_word(f.base, f.skew, head + 8 * w, f.shape);
            memcpy(dst + head + 8 * w, &v, 8);
        }
    }
    if (words - plain > 1) { printf("more than one word left to patched_word\n"); exit(1); }
    for (uint32_t lane = 0; lane < 64 && lane < tail; lane++)
        dst[head + 8 * words + lane] = uint8_t(patched_word(f.base, f.skew, head + 8 * words, f.shape) >> (8 * lane));
}

// One slice through both kernels, its destination a heap block of exactly dst_skew + its length
static Bytes emulate(const Bytes &out, uint32_t word, uint32_t skew, uint32_t dst_skew) {
    Slice slice(out.data(), out.size(), skew);
    const View &f = slice.under(word);
    const uint64_t len = length_of(f);
    if (len == 0) return Bytes();
    uint8_t *mem = static_cast<uint8_t *>(malloc(dst_skew + len)), *dst = mem + dst_skew;        // malloc aligns to 16: dst is dst_skew mod 8
    memset(mem, 0xDD, dst_skew + len);
    copy_to(f, dst, dst_skew, len);
    for (uint32_t j = 0; j < dst_skew; j++)
        if (mem[j] != 0xDD) { printf("a byte in front of the slice's place was written\n"); exit(1); }
    Bytes got(dst, dst + len);
    free(mem);
    return got;
}

static uint64_t g_cases = 0;
static void hold(const Bytes &out, uint32_t word, uint32_t skew, uint32_t dst_skew) {
    const Bytes want = plain(out, word), got = emulate(out, word, skew, dst_skew);
    g_cases++;
    if (want == got) return;
    printf("case %llu differs: %zu bytes, word 0x%x, skew %u, dst_skew %u: want %zu bytes, got %zu\n  out:", (unsigned long long)g_cases, out.size(), word,
           skew, dst_skew, want.size(), got.size());
    for (size_t j = 0; j < out.size() && j < 64; j++) printf(" %02x", out[j]);
    printf("\n");
    exit(1);
}

static const uint8_t kAlphabet[5] = {0, 1, 3, 4, 0x80};
static const uint32_t kLast[3] = {0x00, 0x03, 0x80};             // a last byte that makes an escape, one that needs one, one that does neither

static std::vector<uint32_t> words_for() {
    std::vector<uint32_t> w;
    for (uint32_t esc = 0; esc < 2; esc++)
        for (uint32_t z = 0; z < (esc ? 3u : 1u); z++) {
            w.push_back(esc << 10 | z << 11);                    // no patch
            for (uint32_t parity = 0; parity < 2; parity++)
                for (uint32_t l = 0; l < 3; l++) w.push_back(kLast[l] | parity << 8 | 1u << 9 | esc << 10 | z << 11);
        }
    w.push_back(0xffu | 1u << 9 | 1u << 10 | 3u << 11);          // zeros_before 3 is taken as 2
    return w;
}

// The strings of length `len` with codes [code0, code1), with and without a trailing 0x80, under every word of the table.  The source
// is a heap block of exactly its words, one per string; the destination is a block of this function's own between two bands of
// canary bytes (a heap block per case is what emulate() does, for the seams and the test's cases: too slow for 28 million).
static const uint32_t kThreads = 8;
static uint64_t sweep(uint32_t len, uint64_t code0, uint64_t code1) {
    const std::vector<uint32_t> all = words_for();
    uint64_t cases = 0;
    for (uint64_t code = code0; code < code1; code++) {
        uint8_t s[9];
        uint64_t c = code;
        for (uint32_t j = 0; j < len; j++) { s[j] = kAlphabet[c % 5]; c /= 5; }
        s[len] = 0x80;
        const uint32_t skew = uint32_t(code % 8), dst_skew = uint32_t((code / 8) % 8);
        for (uint32_t n = len; n <= len + 1; n++) {
            Slice slice(s, n, skew);
            for (uint32_t word : all) {
                uint8_t want[32];
                uint32_t n_want = 0, r = n;                      // the rule, byte by byte, on arrays
                uint8_t p[10];
                memcpy(p, s, n);
                if (r && p[r - 1] == 0x80) r--;
                if ((word >> 9) & 1) {
                    if ((r & 1) != ((word >> 8) & 1)) p[r++] = uint8_t(word);
                    else if (r) p[r - 1] = uint8_t(word);
                }
                uint32_t st = (word >> 11) & 3;
                st = st > 2 ? 2 : st;
                for (uint32_t j = 0; j < r; j++) {
                    if (((word >> 10) & 1) && st == 2 && p[j] <= 3) { want[n_want++] = 3; st = 0; }
                    want[n_want++] = p[j];
                    st = p[j] == 0 ? st + 1 : 0;
                }
                const View &f = slice.under(word);
                const uint64_t len_got = length_of(f);
                alignas(8) uint8_t block[8 + 8 + 32 + 8];
                memset(block, 0xDD, sizeof block);
                uint8_t *dst = block + 8 + dst_skew;
                if (len_got <= 32) copy_to(f, dst, dst_skew, len_got);
                bool ok = len_got == n_want && memcmp(dst, want, n_want) == 0;
                for (uint32_t j = 0; j < sizeof block; j++)
                    if ((block + j < dst || block + j >= dst + len_got) && block[j] != 0xDD) ok = false;
                cases++;
                if (!ok) {
                    printf("a string of %u bytes, code %llu, word 0x%x, skew %u, dst_skew %u: want %u bytes, got %llu, or a byte beside them was written\n", n,
                           (unsigned long long)code, word, skew, dst_skew, n_want, (unsigned long long)len_got);
                    exit(1);
                }
            }
        }
    }
    return cases;
}

static int self_check() {
    // `then` is associative: the shuffle network and the lane order give one answer.  Over every run of up to two bytes of the alphabet.
    std::vector<Xfer> runs;
    runs.push_back(identity());
    for (uint8_t a : kAlphabet) {
        runs.push_back(run_of(a, 1));
        for (uint8_t b : kAlphabet) runs.push_back(run_of(uint64_t(a) | uint64_t(b) << 8, 2));
    }
    for (const Xfer &a : runs)
        for (const Xfer &b : runs)
            for (const Xfer &c : runs) {
                const Xfer l = then(then(a, b), c), r = then(a, then(b, c));
                if (l.exit != r.exit || l.cnt != r.cnt) { printf("then() is not associative\n"); return 1; }
            }
    // every short string, alone, under every finish word of the table: in lane order (the network is held to it below, and by
    // associativity), each length's strings dealt out to a few threads
    g_network = false;
    for (uint32_t len = 0; len <= 8; len++) {
        uint64_t count = 1;
        for (uint32_t j = 0; j < len; j++) count *= 5;
        const uint32_t n_threads = count < 1000 ? 1 : kThreads;
        std::vector<std::thread> pool;
        std::vector<uint64_t> cases(n_threads, 0);
        for (uint32_t t = 0; t < n_threads; t++)
            pool.emplace_back([=, &cases] { cases[t] = sweep(len, count * t / n_threads, count * (t + 1) / n_threads); });
        for (uint32_t t = 0; t < n_threads; t++) { pool[t].join(); g_cases += cases[t]; }
    }
    // ... and short strings over every seam of a longer slice, by the network: a lane's word ends every 8 bytes, a trip every 512
    g_network = true;
    const uint32_t seam_words[] = {0u, 1u << 10, 1u << 10 | 2u << 11, 0x00u | 1u << 9 | 1u << 10 | 1u << 11, 0x03u | 1u << 8 | 1u << 9 | 1u << 10, 0x03u | 1u << 9};
    for (uint32_t len = 1; len <= 4; len++) {
        uint64_t count = 1;
        for (uint32_t j = 0; j < len; j++) count *= 3;
        for (uint64_t code = 0; code < count; code++) {
            Bytes s(len);
            uint64_t c = code;
            for (uint32_t j = 0; j < len; j++) { s[j] = kAlphabet[c % 3]; c /= 3; }     // 0, 1, 3: the bytes that matter
            for (uint32_t at : {0u, 3u, 500u, 504u, 505u, 506u, 507u, 508u, 509u, 510u, 511u, 512u, 1019u, 1021u, 1023u, 1024u}) {
                for (uint32_t total : {at + len, 1030u}) {
                    if (total < at + len) continue;
                    Bytes out(total, 0xFF);
                    memcpy(out.data() + at, s.data(), len);
                    for (uint32_t word : seam_words) hold(out, word, uint32_t(code % 8), uint32_t((code + at) % 8));
                }
            }
        }
    }
    // the most a slice can grow
    for (uint32_t n : {1u, 2u, 511u, 512u, 513u, 2000u})
        for (uint32_t z = 0; z < 3; z++) hold(Bytes(n, 0), 1u << 10 | z << 11, z, n % 8);
    printf("ok %llu cases\n", (unsigned long long)g_cases);
    return 0;
}

static int run_cases(const char *in_path, const char *out_path) {
    FILE *in = fopen(in_path, "r"), *out = fopen(out_path, "w");
    if (!in || !out) { printf("cannot open the case files\n"); return 2; }
    std::vector<char> line(1 << 16);
    char hex[1 << 15];
    uint32_t word, skew, dst_skew;
    while (fgets(line.data(), int(line.size()), in)) {
        if (sscanf(line.data(), "%32767s %u %u %u", hex, &word, &skew, &dst_skew) != 4) { printf("bad line\n"); return 2; }
        Bytes b;
        if (strcmp(hex, "-") != 0)
            for (size_t j = 0; hex[j] && hex[j + 1]; j += 2) {
                unsigned v;
                sscanf(hex + j, "%2x", &v);
                b.push_back(uint8_t(v));
            }
        const Bytes got = emulate(b, word, skew & 7, dst_skew & 7);
        std::string s;
        char two[3];
        for (uint8_t x : got) { snprintf(two, sizeof two, "%02x", x); s += two; }
        fprintf(out, "%s\n", s.empty() ? "-" : s.c_str());
    }
    fclose(in);
    fclose(out);
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && strcmp(argv[1], "cases") == 0) return run_cases(argv[2], argv[3]);
    return self_check();
}
