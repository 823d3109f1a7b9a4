// CPU emulation of k_cabac_verify (csrc/avr_cabac_verify.hip): BitReader, CabacDecoder and the slice walk of csrc/avr_cabac_verify.h --
// the very functions the kernel runs -- over one slice in any of the five record forms.  Test build only
// (tests/test_cabac_verify_emul.py compares with the oracle's decoder; tests/cabac_verify_check.cpp is the same under sanitizers).
#include <cstdint>
#include <cstring>
#include <vector>

#include "avr_cabac_verify.h"

namespace {
namespace cv = avr::cabac_verify;

struct ByteSource {                                        // chunk c: the 16 bytes at base + c * stride
    const uint8_t *base;
    size_t stride;
    cv::Chunk16 load(uint32_t c) const {
        cv::Chunk16 v;
        memcpy(v.w, base + size_t(c) * stride, 16);
        return v;
    }
};
struct ArrayStates {                                       // the slice's state bytes, caller's numbering
    uint8_t *p;
    uint32_t get(uint32_t ctx) const { return p[ctx]; }
    void set(uint32_t ctx, uint32_t s) { p[ctx] = uint8_t(s); }
};

template <int FORM>
uint32_t walk(const uint64_t *words, uint32_t len, uint32_t n_bins, uint32_t n_states, const ByteSource &src, ArrayStates &st,
              const cv::TabEntry *tab) {
    return cv::verify_slice<FORM>(words, len, n_bins, n_states, src, st, tab);
}
}  // namespace

extern "C" {

// form: cabac_verify::Form.  recs: `recs_bytes` bytes holding the slice's records in that form's layout -- slice-major forms and codes:
// the slice from byte 0, in whole 16-byte chunks; tile forms: a one-slice tile, the slice in column `lane` (chunk c at byte
// (64 c + lane) * 16).  region: `cap` bytes (a multiple of 8), of which the first out_len are the slice's.  init_states: n_states
// bytes (none for codes); final_states: the encoder's, or null.  Records, region and states are copied into buffers of exactly the
// quoted sizes, so a read outside them is a read outside an allocation.  Returns the first bad bin, n_bins for final states that differ,
// or AVR_VERIFY_NONE.
uint32_t cabac_verify_emul(int form, const uint8_t *recs, size_t recs_bytes, uint32_t lane, uint32_t n_bins, const uint8_t *init_states,
                           uint32_t n_states, const uint8_t *final_states, const uint8_t *region, uint32_t cap, uint32_t out_len) {
    static const avr::CabacTables tables = avr::make_cabac_tables();
    cv::TabEntry tab[128];
    cv::fill_table(tab, tables);
    std::vector<uint8_t> r(recs, recs + recs_bytes), states(init_states, init_states + (form == cv::kCodes ? 0 : n_states));
    states.push_back(0);                                   // the spare byte behind the states (avr_cabac_verify.h: decode_chunk)
    std::vector<uint64_t> words(cap / 8);
    if (cap) memcpy(words.data(), region, cap);
    const bool tiled = cv::form_tiled(form);
    const ByteSource src{r.data() + (tiled ? size_t(lane) * 16 : 0), tiled ? size_t(64) * 16 : size_t(16)};
    ArrayStates st{states.data()};
    const uint32_t len = out_len < cap ? out_len : cap;
    uint32_t bad;
    switch (form) {
    case cv::kTiles2: bad = walk<cv::kTiles2>(words.data(), len, n_bins, n_states, src, st, tab); break;
    case cv::kSlices2: bad = walk<cv::kSlices2>(words.data(), len, n_bins, n_states, src, st, tab); break;
    case cv::kTiles8: bad = walk<cv::kTiles8>(words.data(), len, n_bins, n_states, src, st, tab); break;
    case cv::kSlices8: bad = walk<cv::kSlices8>(words.data(), len, n_bins, n_states, src, st, tab); break;
    default: bad = walk<cv::kCodes>(words.data(), len, n_bins, 0, src, st, tab); break;
    }
    const bool differ = form != cv::kCodes && final_states && n_states && memcmp(states.data(), final_states, n_states) != 0;
    return cv::conclude(bad, n_bins, differ);
}

}  // extern "C"
