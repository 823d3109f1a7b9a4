// Phase B1 as the kernels walk it (B1Walk of csrc/avr_k1p.h: what a lane of k_k1p_replay and k_k1p_b1 runs, eight bins at a time)
// compiled for the host and run the way k_k1p_b1 runs it -- whole lines of groups inside the chunk, the chunk's last groups, then the
// tail past the chunk -- over every chunk of every code stream of a file, and held field by field to b1_stretch, the CPU's statement
// of the result.  A stand-alone program (tests/test_k1p_b1walk_emul.py builds it with AddressSanitizer and UBSan and makes the
// streams); every stream lies in a heap block of exactly the bytes a slice's codes are readable for.
//
//   b1walk_emul FILE     FILE: u32 count, then per stream u32 n, u32 max_stretch, n codes
//
// A lane of a wave takes the path its wave needs, not only its own: every chunk is walked twice, as a lane alone (whose wave is what
// the lane is) and as a lane beside one that is still looking for its opening bin (the opening path for lanes on four candidates
// too).  Per stream a line "i chunks first end meet too_long" goes to stdout for the test to see what
// its streams cover: chunk 1's opening bin, end, the bin after which the four candidates are one (a walk of step_range here), and
// whether it was too long ("-" for a stream of one chunk); then "ok <chunks walked>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>


#include "avr_k1p.h"
#include "avr_tables.h"

using namespace avr;
using namespace avr::k1p;

namespace {

constexpr CabacTables kT = make_cabac_tables();
CodeEntry g_codes[256];
U4 g_cinfo[256];
U2 g_codes2[256];

void make_tables() {
    uint32_t rows[64];
    for (uint32_t p = 0; p < 64; p++) rows[p] = kT.packed[2 * p][0];
    for (uint32_t c = 0; c < 256; c++) {
        g_codes[c] = code_entry(c, rows);
        g_cinfo[c] = b1_entry(g_codes[c], 0u, c);
        g_codes2[c] = codes2_entry(g_codes[c].row);
    }
}

// k_k1p_b1's loops around B1Walk; beside_looking: the wave holds a lane in mode 0
Stretch walk(const uint8_t *res, uint32_t n, uint32_t c, uint32_t max_stretch, bool beside_looking) {
    const ChunkSpan span = chunk_span(c, n);
    const uint32_t i0 = span.i0, i1 = span.i1;
    B1Walk b1;
    b1.init(c, i0, i1, n, max_stretch, g_codes2);
    U4 e[8];
    auto eight = [&](uint32_t at) { for (uint32_t j = 0; j < 8; j++) e[j] = g_cinfo[res[at + j]]; };
    auto inside = [&](uint32_t at) {
        eight(at);
        if (beside_looking) b1.group_inside_as(at, e, true);
        else b1.group_inside(at, e);
    };
    if (i0 < n) {
        uint32_t i = i0;
        for (; i + 64 <= i1; i += 64)
            for (uint32_t g = 0; g < 64; g += 8) inside(i + g);
        for (; i < i1; i += 16) {
            eight(i); b1.group(i, e);
            eight(i + 8); b1.group(i + 8, e);
        }
        b1.chunk_done();
        for (i = i0 + kChunk; b1.mode != 3 && i < n; i += 16) {
            eight(i); b1.tail(i, e);
            if (b1.mode != 3) { eight(i + 8); b1.tail(i + 8, e); }
        }
    }
    return b1.finish();
}

// the bin after which the four candidates of the stretch that opens at `first` are one range (kNone: not before the slice ends)
uint32_t meet_of(const uint8_t *res, uint32_t n, uint32_t first) {
    uint32_t R[4];
    for (uint32_t q = 0; q < 4; q++) { uint32_t sh; R[q] = post_lps_range(g_codes[res[first]].row, q, &sh); }
    for (uint32_t i = first;; i++) {
        if (R[0] == R[1] && R[1] == R[2] && R[2] == R[3]) return i;
        if (i + 1 >= n) return kNone;
        for (uint32_t q = 0; q < 4; q++) step_range(g_codes[res[i + 1]], &R[q]);
    }
}

bool same(const Stretch &a, const Stretch &b) {
    bool ok = a.first == b.first && a.end == b.end && a.exit_q == b.exit_q && a.too_long == b.too_long;
    for (int q = 0; q < 4; q++) ok = ok && a.t_exit[q] == b.t_exit[q] && a.r_exit[q] == b.r_exit[q];
    return ok;
}

void show(const char *what, const Stretch &s) {
    fprintf(stderr, "  %s: first %u end %u t_exit %u %u %u %u r_exit %u %u %u %u exit_q %02x too_long %u\n", what, s.first, s.end, s.t_exit[0],
            s.t_exit[1], s.t_exit[2], s.t_exit[3], s.r_exit[0], s.r_exit[1], s.r_exit[2], s.r_exit[3], s.exit_q, s.too_long);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    make_tables();
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    uint64_t walked = 0;
    int bad = 0;
    for (uint32_t s = 0; s < count; s++) {
        uint32_t head[2];
        if (fread(head, 4, 2, f) != 2) return 2;
        const uint32_t n = head[0], max_stretch = head[1];
        // a slice's codes are readable up to the next multiple of 16 with a group to spare, padded with kCodePad
        const size_t bytes = ((size_t(n) + 15) & ~size_t(15)) + 16;
        uint8_t *res = static_cast<uint8_t *>(aligned_alloc(16, bytes));
        memset(res, kCodePad, bytes);
        if (n && fread(res, 1, n, f) != n) return 2;
        const uint32_t chunks = chunks_of(n);
        Stretch second{};
        for (uint32_t c = 0; c < chunks; c++) {
            Stretch want;
            b1_stretch(res, n, c, g_codes, max_stretch, &want);
            if (c == 1) second = want;
            for (int beside = 0; beside < 2; beside++) {
                const Stretch got = walk(res, n, c, max_stretch, beside != 0);
                walked++;
                if (!same(got, want) && bad++ < 10) {
                    fprintf(stderr, "stream %u (%u bins, max_stretch %u) chunk %u%s\n", s, n, max_stretch, c, beside ? ", beside a looking lane" : "");
                    show("B1Walk    ", got);
                    show("b1_stretch", want);
                }
            }
        }
        if (chunks < 2) printf("%u %u - - - -\n", s, chunks);
        else printf("%u %u %u %u %u %u\n", s, chunks, second.first, second.end, second.first == kNone ? kNone : meet_of(res, n, second.first), second.too_long);
        free(res);
    }
    fclose(f);
    if (bad) { fprintf(stderr, "%d chunk walks differ\n", bad); return 1; }
    printf("ok %llu\n", static_cast<unsigned long long>(walked));
    return 0;
}
