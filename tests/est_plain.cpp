// The compress direction's estimator rule, plainly and serially, for inputs too large for tests/range_keys.py: a table of 1026
// {pos, neg} pairs a group, a bin coded with its key's pair as it stands, then pos or neg up by one, both halved (rounding up) when
// their sum exceeds 0x60.  Written from range_keys.resolve_group, which tests/test_est_emul.py pins it to; it shares nothing with
// csrc/avr_est.h.  Test build only.
#include <cstdint>
#include <cstring>

extern "C" {

// Group g = slices group_first[g] .. group_first[g + 1], begun from est_in[g] (1026 {pos, neg} byte pairs; null: {1, 1}).  A good
// slice gets its n_bins records at rec_off and zeros (AVR_NOP_RANGE) up to the next multiple of eight, and status 0.  A slice that
// holds a malformed record, and every later slice of its group, gets status 3 and no records; such a group's est_out is left alone.
// Nothing else of recs_out, status or est_out is written.  Returns the number of slices with status 3.
uint64_t est_plain_resolve(const uint16_t *keys, const uint64_t *rec_off, const uint32_t *n_bins, const uint32_t *group_first,
                           uint32_t n_groups, const uint8_t *est_in, uint8_t *est_out, uint16_t *recs_out, int32_t *status) {
    uint64_t n_bad = 0;
    for (uint32_t g = 0; g < n_groups; g++) {
        uint8_t tab[1026][2];
        if (est_in) memcpy(tab, est_in + uint64_t(g) * sizeof tab, sizeof tab); else memset(tab, 1, sizeof tab);
        bool ok = true;
        for (uint32_t i = group_first[g]; i < group_first[g + 1]; i++) {
            const uint16_t *in = keys + rec_off[i];
            uint16_t *out = recs_out + rec_off[i];
            const uint32_t n = n_bins[i];
            for (uint32_t j = 0; ok && j < n; j++) ok = (in[j] >> 1) < 1026;
            if (!ok) { status[i] = 3; n_bad++; continue; }
            for (uint32_t j = 0; j < n; j++) {
                uint8_t *e = tab[in[j] >> 1];
                const unsigned bin = in[j] & 1u;
                out[j] = uint16_t(bin | (unsigned(e[0]) << 1) | (unsigned(e[1]) << 8));
                e[1 - bin]++;
                if (unsigned(e[0]) + e[1] > 0x60) { e[0] = uint8_t((e[0] + 1) / 2); e[1] = uint8_t((e[1] + 1) / 2); }
            }
            for (uint32_t j = n; j < ((n + 7) & ~7u); j++) out[j] = 0;
            status[i] = 0;
        }
        if (ok && est_out) memcpy(est_out + uint64_t(g) * sizeof tab, tab, sizeof tab);
    }
    return n_bad;
}

}  // extern "C"
