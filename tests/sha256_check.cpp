// csrc/host/avr_sha256.h as a stand-alone program, for tests/test_sha256.py (built with AddressSanitizer and UBSan, run as a child process):
//
//     sha256_check <file> <splits>
//
// prints the SHA-256 of the file's bytes as hex, one line per way of feeding them: first in one update() call, then <splits> times
// in pieces -- seeded draws (the seed is the line's number), the piece lengths from ranges that straddle the 64-byte block in every way
// (0 and 1 byte, below, at and above a block, many blocks), a zero-length update among them.  The bytes are copied into a heap
// buffer of exactly their length, and every piece into one of exactly its length, so that a read past either is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <random>
#include <vector>

#include "host/avr_sha256.h"

static void print_hex(const std::string &d) {
    for (unsigned char c : d) printf("%02x", c);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <file> <splits>\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const std::vector<char> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t n = file.size();
    char *data = static_cast<char *>(malloc(n ? n : 1));           // exactly n bytes (one where n is 0, never read)
    if (n) memcpy(data, file.data(), n);

    print_hex(avr::host::sha256::of(data, n));
    {                                                    // an object used again, through reset(), after a whole message
        avr::host::sha256 h;
        h.update(data, n);
        h.finish();
        h.reset();
        h.update(data, n);
        print_hex(h.finish());
    }
    static const size_t caps[] = {1, 2, 7, 55, 56, 63, 64, 65, 128, 200, 4096, 100000};
    for (int seed = 0; seed < atoi(argv[2]); seed++) {
        std::mt19937_64 rng(uint64_t(seed) + 1);
        avr::host::sha256 h;
        size_t at = 0;
        h.update(nullptr, 0);
        while (at < n) {
            const size_t cap = caps[rng() % (sizeof caps / sizeof caps[0])];
            size_t k = size_t(rng() % (cap + 1));        // 0 .. cap
            if (k > n - at) k = n - at;
            char *piece = static_cast<char *>(malloc(k ? k : 1));
            if (k) memcpy(piece, data + at, k);
            h.update(piece, k);
            free(piece);
            at += k;
        }
        h.update(data + n, 0);
        print_hex(h.finish());
    }
    free(data);
    return 0;
}
