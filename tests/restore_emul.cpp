// TEST BUILD ONLY: the restore check's per-word functions (avrecode-ms_amd/csrc/avr_restore.h) compiled by g++, one emulated wave per
// slice: what k_restore_check does with its 64 lanes, lane by lane, and the least of their answers in place of the cross-lane shuffles.
#include <cstdint>

#include "avr_restore.h"

namespace rs = avr::restore;

// region: the slice's output region, `cap` bytes (a multiple of 8) of which min(out_len, cap) are its coded bytes; expect: E bytes,
// readable to the next multiple of 8.  Both 8-byte aligned.
extern "C" uint32_t restore_emul(const uint8_t *region, uint64_t cap, uint32_t out_len, const uint8_t *expect, uint32_t E) {
    const uint32_t cap32 = cap < 0xffffffffull ? uint32_t(cap) : 0xffffffffu;                        // region_capacity (avr_coder.h)
    const uint32_t L = out_len < cap32 ? out_len : cap32;
    const rs::Shape s = rs::make_shape(L, E, L ? region[L - 1] : 0u, E >= 2 ? expect[E - 1] : 0u);
    uint32_t best = AVR_VERIFY_NONE;
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t d = rs::lane_first_diff(reinterpret_cast<const uint64_t *>(region), reinterpret_cast<const uint64_t *>(expect), s, lane);
        best = d < best ? d : best;
    }
    return rs::conclude(best, s);
}
