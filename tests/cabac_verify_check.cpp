// Stand-alone check of the K1 verifier's host/device functions (csrc/avr_cabac_verify.h) under AddressSanitizer and UBSan: the five
// record forms on heap buffers of exactly the quoted sizes, over clean, flipped and truncated streams, each answer held against the
// oracle's spec decoder (oracle/spec_cabac.c), the streams coded by the oracle's encoder (oracle/avr_oracle.c).  Built and started as a
// child process by tests/test_cabac_verify_emul.py; prints "ok" and returns 0, or says what differed and returns 1.
#include <cstdio>
#include <cstdlib>

#include "avr_oracle.h"
#include "cabac_verify_emul.cpp"

namespace {

struct Rng {                                               // xorshift64*: the streams need to be the same on every run, nothing more
    uint64_t s;
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
    uint32_t below(uint32_t n) { return uint32_t((next() >> 33) % n); }
};

struct Slice {
    std::vector<uint16_t> recs;
    std::vector<uint8_t> states, final_states, data, mlps;
};

Slice make_slice(Rng &rng, uint32_t n, uint32_t n_ctx, bool terminate, uint32_t state_limit) {
    Slice s;
    uint8_t lps[512];
    s.mlps.resize(256);
    avr_oracle_cabac_tables(lps, s.mlps.data());
    std::vector<uint32_t> bias(n_ctx);
    for (auto &b : bias) b = rng.below(2) ? 5 + rng.below(20) : 75 + rng.below(20);          // percent of ones
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t kind = rng.below(100);
        if (kind < 20) s.recs.push_back(uint16_t(1024u << 1 | rng.below(2)));
        else if (kind < 23) s.recs.push_back(uint16_t(1025u << 1));
        else { const uint32_t c = rng.below(n_ctx); s.recs.push_back(uint16_t(c << 1 | (rng.below(100) < bias[c]))); }
    }
    if (terminate) s.recs.push_back(uint16_t(1025u << 1 | 1));
    for (uint32_t c = 0; c < n_ctx; c++) s.states.push_back(uint8_t(rng.below(state_limit)));
    s.final_states = s.states;
    s.data.resize(s.recs.size() + 64);
    int status = 0;
    const size_t len = avr_oracle_cabac_encode(s.recs.data(), s.recs.size(), s.final_states.data(), n_ctx, s.data.data(), s.data.size(), &status);
    if (status != AVR_ORACLE_OK) { printf("oracle encode status %d\n", status); exit(1); }
    s.data.resize(len);
    return s;
}

uint32_t oracle_first_bad(const Slice &s, const std::vector<uint8_t> &data) {
    std::vector<uint8_t> st(s.states), bins(s.recs.size() + 1), bytes(data);
    bytes.push_back(0);                                    // (a pointer to hand over for an empty stream)
    if (avr_spec_cabac_decode(bytes.data(), data.size(), s.recs.data(), s.recs.size(), st.data(), st.size(), bins.data()) != AVR_ORACLE_OK) {
        printf("oracle decode failed\n");
        exit(1);
    }
    for (size_t i = 0; i < s.recs.size(); i++)
        if (bins[i] != (s.recs[i] & 1)) return uint32_t(i);
    return AVR_VERIFY_NONE;
}

// the slice's records in one form, in a buffer of exactly the size the form quotes
std::vector<uint8_t> form_buffer(int form, const Slice &s, uint32_t lane) {
    const uint32_t n = uint32_t(s.recs.size());
    std::vector<uint8_t> rows;
    if (cv::form_wide(form)) {
        std::vector<uint16_t> a((n + 7) / 8 * 8, uint16_t(1026u << 1));
        std::copy(s.recs.begin(), s.recs.end(), a.begin());
        rows.resize(a.size() * 2);
        if (!rows.empty()) memcpy(rows.data(), a.data(), rows.size());
    } else {
        rows.assign((n + 15) / 16 * 16, 0xA5);             // padding that means something in either form: it is never decoded
        std::vector<uint8_t> st(s.states);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t b = s.recs[i] & 1u, sel = s.recs[i] >> 1;
            if (form != cv::kCodes) rows[i] = uint8_t((sel == 1024 ? 126u : sel == 1025 ? 127u : sel) << 1 | b);
            else if (sel == 1024) rows[i] = uint8_t(252u | b);
            else if (sel == 1025) rows[i] = uint8_t(255u - b);
            else {
                const uint32_t t = st[sel];
                rows[i] = uint8_t(t >= 126 ? 255u - ((b ^ t) & 1u) : (t << 1) | b);
                st[sel] = b != (t & 1u) ? s.mlps[127 - t] : s.mlps[128 + t];
            }
        }
    }
    if (!cv::form_tiled(form)) return rows;
    std::vector<uint8_t> tile(rows.size() * 64, 0x5A);
    for (size_t c = 0; c < rows.size() / 16; c++) memcpy(tile.data() + (c * 64 + lane) * 16, rows.data() + c * 16, 16);
    return tile;
}

int failures = 0;

void check(const Slice &s, const std::vector<std::vector<uint8_t>> &forms, uint32_t lane, const std::vector<uint8_t> &data, const char *what) {
    const uint32_t want = oracle_first_bad(s, data), n = uint32_t(s.recs.size()), cap = (n + 64 + 7) / 8 * 8;
    std::vector<uint8_t> region(cap, 0xFF);                // what lies past the length is not zero
    std::copy(data.begin(), data.end(), region.begin());
    for (int form = 0; form < cv::kForms; form++) {
        if (!cv::form_wide(form) && form != cv::kCodes && s.states.size() > 126) continue;
        const uint32_t got = cabac_verify_emul(form, forms[form].data(), forms[form].size(), lane, n, s.states.data(), uint32_t(s.states.size()),
                                               nullptr, region.data(), cap, uint32_t(data.size()));
        if (got != want && failures++ < 20) printf("%s: form %d n_bins %u n_states %zu: got %u, the oracle %u\n", what, form, n, s.states.size(), got, want);
        // a length beyond the capacity is the whole region, 0xFF tail included, and not a byte more
        const uint32_t all = cabac_verify_emul(form, forms[form].data(), forms[form].size(), lane, n, s.states.data(), uint32_t(s.states.size()),
                                               nullptr, region.data(), cap, 0xFFFFFFFFu);
        if (all != oracle_first_bad(s, region) && failures++ < 20) printf("%s: form %d n_bins %u: length beyond the capacity: got %u\n", what, form, n, all);
    }
}

}  // namespace

int main() {
    Rng rng{0x9E3779B97F4A7C15ull};
    const uint32_t counts[] = {0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200, 1023, 1024, 1025, 3000};
    const uint32_t ctxs[] = {1, 20, 126, 460};
    uint32_t n_checks = 0;
    for (uint32_t n_ctx : ctxs)
        for (uint32_t n : counts)
            for (int t = 0; t < 2; t++) {
                const Slice s = make_slice(rng, n, n_ctx, t != 0, n % 2 ? 128 : 126);
                const uint32_t lane = rng.below(64);
                std::vector<std::vector<uint8_t>> forms;
                for (int form = 0; form < cv::kForms; form++) forms.push_back(form_buffer(form, s, lane));
                if (oracle_first_bad(s, s.data) != AVR_VERIFY_NONE) { printf("the oracle does not decode its own stream (n %u)\n", n); return 1; }
                check(s, forms, lane, s.data, "clean");
                for (int form = 0; form < cv::kCodes; form++) {                  // the final states: right, and with one byte changed
                    if (!cv::form_wide(form) && n_ctx > 126) continue;
                    std::vector<uint8_t> fin(s.final_states), region((uint32_t(s.recs.size()) + 64 + 7) / 8 * 8, 0);
                    std::copy(s.data.begin(), s.data.end(), region.begin());
                    auto run = [&] { return cabac_verify_emul(form, forms[form].data(), forms[form].size(), lane, uint32_t(s.recs.size()), s.states.data(),
                                                              n_ctx, fin.data(), region.data(), uint32_t(region.size()), uint32_t(s.data.size())); };
                    if (run() != AVR_VERIFY_NONE && failures++ < 20) printf("final states: form %d n_bins %zu: a clean slice fails\n", form, s.recs.size());
                    fin[rng.below(n_ctx)] ^= 0x10;
                    if (run() != s.recs.size() && failures++ < 20) printf("final states: form %d n_bins %zu: a changed byte goes unseen\n", form, s.recs.size());
                }
                const size_t len = s.data.size();
                for (int k = 0; k < 12 && len; k++) {                            // flips anywhere, the last bytes included
                    std::vector<uint8_t> bad(s.data);
                    const size_t p = k < 3 ? 0 : k < 6 ? len - 1 : rng.below(uint32_t(len));
                    bad[p] ^= uint8_t(k % 3 == 0 ? 0x01 : k % 3 == 1 ? 0x80 : 0xFF);
                    check(s, forms, lane, bad, "flip");
                    n_checks++;
                }
                for (size_t cut : {size_t(0), len / 2, len ? len - 1 : 0}) {
                    check(s, forms, lane, std::vector<uint8_t>(s.data.begin(), s.data.begin() + cut), "cut");
                    n_checks++;
                }
            }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok (%u corrupted streams, five forms)\n", n_checks);
    return 0;
}
