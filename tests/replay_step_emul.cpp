// The replay's state chain (replay_step8 of csrc/avr_k1p.h: what k_k1p_replay's `eight` and `eight8` call, eight bins a group)
// compiled for the host and held, group by group, to the plain loop per bin -- read the state byte, look up info[state << 1 | bin],
// write the next state back -- over a lane's state column laid out as the kernel lays it out.  A stand-alone program
// (tests/test_k1p_replay_step_emul.py builds it with AddressSanitizer and UBSan and makes the streams); the column, the records
// and the tables lie in heap blocks of exactly their size.
//
//   replay_step_emul FILE     FILE: u32 count, then per stream u32 n, u32 nk, nk initial states, n two-byte records, n expected codes
//
// Every stream is walked twice: as two-byte records and as one-byte records (whose last group is masked: bytes at or past n go
// to the padding pseudo state whatever they hold, and hold here the last real bin's context with the other bin).  After every group
// the eight entries and the whole column are those of the plain loop, and every code is the one the file expects (made by a walk of the contexts'
// states that knows nothing of these tables).  Before the streams: every row of the table, every state x bin as bin j with bin j+1 in
// the same slot, at every j.  "ok <bins walked>" at the end.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "avr_k1p.h"
#include "avr_tables.h"

using namespace avr;
using namespace avr::k1p;

namespace {

constexpr CabacTables kT = make_cabac_tables();
constexpr uint32_t kLane = 37;                                   // the lane whose column this is: 4 bytes of every 256-byte row
U4 *g_info;                                                      // [2 * kReplayStates], as k_k1p_replay fills it

void make_tables() {
    uint32_t rows[64];
    for (uint32_t p = 0; p < 64; p++) rows[p] = kT.packed[2 * p][0];
    g_info = static_cast<U4 *>(aligned_alloc(16, sizeof(U4) * 2 * kReplayStates));
    for (uint32_t i = 0; i < 2 * kReplayStates; i++) {
        const uint32_t st = i >> 1, bin = i & 1u;
        uint32_t next, code;
        if (st < 128) {
            const uint32_t nx = kT.packed[st][1];
            next = ((bin ^ st) & 1u) ? (nx >> 8) & 0xffu : nx & 0xffu;
            code = code_context(st, bin);
        } else {
            next = st;
            code = st == kStBypass ? kCodeBypass | bin : st == kStTerminate ? code_terminate(bin) : kCodePad;
        }
        g_info[i] = b1_entry(code_entry(code, rows), next, code);
    }
}

// a lane's column: rows of 256 bytes (four slots x 64 lanes), slot kk at row kk / 4, byte kk % 4 of the lane's four
struct Column {
    uint32_t nk, bytes;
    uint8_t *mem, *stb;
    Column(uint32_t nk_, const uint8_t *states) : nk(nk_) {
        bytes = ((nk + 8) >> 2) << 8;
        mem = static_cast<uint8_t *>(malloc(bytes));
        memset(mem, 0xee, bytes);
        stb = mem + kLane * 4;
        for (uint32_t k = 0; k < nk; k++) stb[slot(k)] = states[k];
        const uint32_t pseudo[5] = {kStNone, kStBypass, kStTerminate, kStPad, kStNone};
        for (uint32_t j = 0; j < 5; j++) stb[slot(nk + j)] = uint8_t(pseudo[j]);
    }
    Column(const Column &) = delete;
    ~Column() { free(mem); }
    static uint32_t slot(uint32_t kk) { return ((kk & ~3u) << 6) + (kk & 3u); }
};

// sel_off of the two-byte form: contexts by their id (the streams use dense ids), 1024 bypass, 1025 terminate, 1026 no-op, the rest none
uint32_t off2(uint32_t sel, uint32_t nk) {
    const uint32_t kLast = 1023, over = (sel < kLast ? kLast : sel > kLast + 4 ? kLast + 4 : sel) - kLast;
    return Column::slot((sel < nk ? sel : nk) + over);
}
// ... and of the one-byte form: 126 bypass, 127 terminate, [nk, 126) none
uint32_t off1(uint32_t sel, uint32_t nk) { return Column::slot(sel < nk ? sel : sel == 126 ? nk + 1 : sel == 127 ? nk + 2 : nk + 4); }

int g_bad = 0;
uint64_t g_walked = 0;

void plain8(uint8_t *stb, const uint32_t off[8], const uint32_t bin[8], U4 e[8]) {
    for (uint32_t j = 0; j < 8; j++) {
        uint8_t *sp = stb + off[j];
        const uint32_t st = *sp;
        e[j] = g_info[(st << 1) | bin[j]];
        *sp = uint8_t(e[j].y);
    }
}

// one group on both columns; want[j]: the code bin j has to get (256: none asked for)
void group(const char *what, uint32_t at, Column &plain, Column &a, const uint32_t off[8], const uint32_t bin[8], const uint32_t want[8]) {
    U4 ep[8], ea[8];
    plain8(plain.stb, off, bin, ep);
    replay_step8(a.stb, off, bin, g_info, ea);
    bool ok = !memcmp(ep, ea, sizeof ep) && !memcmp(plain.mem, a.mem, plain.bytes);
    for (uint32_t j = 0; j < 8; j++) ok = ok && (want[j] > 255 || ((ep[j].y >> 8) & 0xffu) == want[j]);
    g_walked += 8;
    if (!ok && g_bad++ < 10) {
        fprintf(stderr, "%s, group at bin %u:\n", what, at);
        for (uint32_t j = 0; j < 8; j++)
            fprintf(stderr, "  bin %u off %4u bin %u: plain next %3u code %3u | replay_step8 %3u %3u | expected code %u\n", j, off[j], bin[j],
                    ep[j].y & 0xffu, (ep[j].y >> 8) & 0xffu, ea[j].y & 0xffu, (ea[j].y >> 8) & 0xffu, want[j]);
    }
}

void every_row() {
    for (uint32_t st = 0; st < kReplayStates; st++)
        for (uint32_t b = 0; b < 2; b++)
            for (uint32_t j = 0; j < 8; j++) {
                // slot 0 holds the state (a pseudo state too: as far as the step knows a slot is a slot); the other bins of the group are on slots 1 and 2
                uint8_t states[3] = {uint8_t(st), 20, 77};
                Column plain(3, states), ca(3, states);
                uint32_t off[8], bin[8], want[8];
                for (uint32_t i = 0; i < 8; i++) { off[i] = Column::slot(1 + (i & 1)); bin[i] = (i >> 1) & 1u; want[i] = 256; }
                off[j] = Column::slot(0); bin[j] = b;
                if (j < 7) { off[j + 1] = Column::slot(0); bin[j + 1] = st & 1u; }
                group("every row", st * 2 + b, plain, ca, off, bin, want);
                if (j == 7) {                                    // ... and the successor seen by the next group's first bin
                    for (uint32_t i = 0; i < 8; i++) off[i] = Column::slot(i == 0 ? 0 : 1 + (i & 1));
                    group("every row, next group", st * 2 + b, plain, ca, off, bin, want);
                }
            }
}

void stream(uint32_t s, uint32_t n, uint32_t nk, const uint8_t *states, const uint16_t *recs, const uint8_t *codes) {
    char what[64];
    {
        snprintf(what, sizeof what, "stream %u, two-byte records", s);
        Column plain(nk, states), ca(nk, states);
        for (uint32_t i = 0; i < n; i += 8) {
            uint32_t off[8], bin[8], want[8];
            for (uint32_t j = 0; j < 8; j++) {
                const uint32_t r = i + j < n ? recs[i + j] : 1026u << 1;     // a slice's records are padded with no-ops to a multiple of 8
                off[j] = off2((r >> 1) & 0x7ffu, nk); bin[j] = r & 1u;
                want[j] = i + j < n ? codes[i + j] : kCodePad;
            }
            group(what, i, plain, ca, off, bin, want);
        }
    }
    {
        snprintf(what, sizeof what, "stream %u, one-byte records", s);
        Column plain(nk, states), ca(nk, states);
        const uint32_t padded = (n + 7) & ~7u;
        uint8_t *r8 = static_cast<uint8_t *>(malloc(padded ? padded : 1));
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t sel = recs[i] >> 1;
            r8[i] = uint8_t((recs[i] & 1u) | (sel < 1024 ? sel : sel == 1024 ? 126u : 127u) << 1);
        }
        for (uint32_t i = n; i < padded; i++) r8[i] = r8[n - 1] ^ 1u;        // what the mask has to keep out of the last real bin's context
        const uint32_t pad_off = Column::slot(nk + 3);
        for (uint32_t i = 0; i < n; i += 8) {
            uint32_t off[8], bin[8], want[8];
            const bool masked = i + 8 > n;
            for (uint32_t j = 0; j < 8; j++) {
                off[j] = off1(r8[i + j] >> 1, nk);
                if (masked) off[j] = i + j < n ? off[j] : pad_off;
                bin[j] = r8[i + j] & 1u;
                want[j] = i + j < n ? codes[i + j] : kCodePad;
            }
            group(what, i, plain, ca, off, bin, want);
        }
        free(r8);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    make_tables();
    every_row();
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t s = 0; s < count; s++) {
        uint32_t head[2];
        if (fread(head, 4, 2, f) != 2) return 2;
        const uint32_t n = head[0], nk = head[1];
        if (!n || !nk || nk > 126) return 2;
        std::vector<uint8_t> states(nk), codes(n);
        std::vector<uint16_t> recs(n);
        if (fread(states.data(), 1, nk, f) != nk || fread(recs.data(), 2, n, f) != n || fread(codes.data(), 1, n, f) != n) return 2;
        stream(s, n, nk, states.data(), recs.data(), codes.data());
    }
    fclose(f);
    free(g_info);
    if (g_bad) { fprintf(stderr, "%d groups differ\n", g_bad); return 1; }
    printf("ok %llu\n", static_cast<unsigned long long>(g_walked));
    return 0;
}
