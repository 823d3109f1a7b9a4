// The per-chunk step of K1p's context chains (chain_step of csrc/avr_k1p.h: what a lane of k_k1p_ctxchain, k_k1p_chain_seg and
// k_k1p_chain_fix runs for every chunk) compiled for the host, with the table it reads made entry by entry as k_k1p_tn makes it.
// tests/test_k1p_chain_step_emul.py holds it against a walk of the transition table, bin by bin.
#include <stdint.h>

#include "avr_k1p.h"
#include "avr_tables.h"

using namespace avr;
using namespace avr::k1p;

namespace {
constexpr CabacTables kT = make_cabac_tables();
}

extern "C" {

uint32_t chain_emul_chunk_bins() { return kChunk; }
uint32_t chain_emul_tn_bytes() { return tn_section(9); }
void chain_emul_tn(uint8_t *tn) {
    for (uint32_t i = 0; i < tn_section(9); i++) tn[i] = tn_entry(i, kT.packed);
}

// Case i: the run of left[i] bins from bit pos[i] of the bit string `bits` (kChunkBitDwords + 4 dwords: the window of a run that
// starts in the last dword reaches three past it) from the states st[ns * i ..], ns = 1 or 2 walked side by side; the states after
// it come back in their place.
void chain_emul_steps(const uint8_t *tn, const uint32_t *bits, uint64_t n, const uint32_t *pos, const uint32_t *left, uint32_t ns, uint32_t *st) {
    for (uint64_t i = 0; i < n; i++) {
        const U4 w = chain_window(bits, pos[i]);
        if (ns == 1) {
            uint32_t s[1] = {st[i]};
            chain_step<1>(tn, bits, pos[i], left[i], w, s);
            st[i] = s[0];
        } else {
            uint32_t s[2] = {st[2 * i], st[2 * i + 1]};
            chain_step<2>(tn, bits, pos[i], left[i], w, s);
            st[2 * i] = s[0];
            st[2 * i + 1] = s[1];
        }
    }
}

}  // extern "C"
