// CPU emulation of k_range_verify (csrc/avr_verify.hip): RangeDecoder64 and the slice walk of csrc/avr_verify.h -- the very functions
// the kernel runs -- over one slice.  Test build only (tests/test_range_verify_emul.py compares with the oracle's decoder).
#include <cstdint>
#include <cstring>
#include <vector>

#include "avr_verify.h"

namespace {
struct SliceSource {                                       // the slice-major layout: chunk c is records 8c .. 8c + 7
    const uint16_t *recs;
    avr::verify::Chunk8 load(uint32_t c) const {
        avr::verify::Chunk8 v;
        memcpy(v.w, recs + size_t(c) * 8, 16);
        return v;
    }
};
}  // namespace

extern "C" {

// recs: n_bins records followed by no-op records up to a multiple of 8.  region: `cap` bytes (a multiple of 8), of which the first
// out_len are the slice's; what lies behind them is the caller's to fill.  The region is copied into a buffer of exactly cap bytes, so a
// read outside it is a read outside an allocation.  Returns the first bad bin or AVR_VERIFY_NONE.
uint32_t range_verify_emul(const uint16_t *recs, uint32_t n_bins, const uint8_t *region, uint32_t cap, uint32_t out_len) {
    double inv_d[256];
    for (uint32_t d = 0; d < 256; d++) inv_d[d] = d ? 1.0 / double(d) : 0.0;
    std::vector<uint64_t> words(cap / 8);
    if (cap) memcpy(words.data(), region, cap);
    const SliceSource src{recs};
    return avr::verify::verify_slice(words.data(), out_len < cap ? out_len : cap, n_bins, src, inv_d);
}

}  // extern "C"
