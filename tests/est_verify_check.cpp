// Stand-alone check of the estimator checker's host/device functions (csrc/avr_est_verify.h) under AddressSanitizer and UBSan: the
// walk of tests/est_verify_emul.cpp on heap buffers of exactly the documented extents -- records up to the last slice's padding and
// not a record more, tables of 1026 pairs, one status and one first_bad per slice, the workspace of the quoted size -- over sound
// records made by the plain rule here, and over corrupted ones.  Built and started as a child process by
// tests/test_est_verify_emul.py; prints "ok" and returns 0, or says what differed and returns 1.
#include <cstdio>
#include <cstdlib>

#include "est_verify_emul.cpp"

namespace {

struct Rng {                                               // xorshift64*: the same streams on every run, nothing more
    uint64_t s;
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
    uint32_t below(uint32_t n) { return uint32_t((next() >> 33) % n); }
};

template <class T>
struct Heap {                                              // exactly n elements on the heap (n = 0: one byte nobody may touch)
    T *p;
    size_t n;
    explicit Heap(size_t n_) : p(static_cast<T *>(malloc(n_ ? n_ * sizeof(T) : 1))), n(n_) {}
    ~Heap() { free(p); }
    Heap(const Heap &) = delete;
};

int fail(const char *what, uint32_t a, uint32_t b, uint32_t c) {
    printf("%s: %u %u %u\n", what, a, b, c);
    return 1;
}

int run_case(Rng &rng, uint32_t n_slices, uint32_t max_bins, uint32_t n_keys, uint32_t chunk, uint32_t span, bool with_in, uint32_t gap) {
    Heap<uint32_t> n_bins(n_slices), group_first(n_slices + 1), first_bad(n_slices);
    Heap<uint64_t> rec_off(n_slices + 1);
    Heap<int32_t> status(n_slices);
    uint32_t n_groups = 0;
    rec_off.p[0] = 0;
    for (uint32_t i = 0; i < n_slices; i++) {
        n_bins.p[i] = rng.below(4) == 0 ? 0 : rng.below(max_bins);
        rec_off.p[i + 1] = rec_off.p[i] + (n_bins.p[i] + 7) / 8 * 8 + (i + 1 < n_slices ? 8 * gap : 0);
        if (i == 0 || rng.below(3) == 0) group_first.p[n_groups++] = i;
    }
    group_first.p[n_groups] = n_slices;
    const size_t total = rec_off.p[n_slices];
    Heap<uint16_t> keys(total), recs(total);
    Heap<uint8_t> est_in(size_t(n_groups) * kKeys * 2), est_out(size_t(n_groups) * kKeys * 2);
    for (size_t i = 0; i < total; i++) { keys.p[i] = 0xeeee; recs.p[i] = 0xabcd; }
    for (uint32_t g = 0; g < n_groups; g++) {
        uint8_t *in = est_in.p + size_t(g) * kKeys * 2, *out = est_out.p + size_t(g) * kKeys * 2;
        for (uint32_t k = 0; k < kKeys; k++) {
            const uint32_t tot = with_in ? 2 + rng.below(95) : 2, pos = with_in ? 1 + rng.below(tot - 1) : 1;
            in[2 * k] = out[2 * k] = uint8_t(pos);
            in[2 * k + 1] = out[2 * k + 1] = uint8_t(tot - pos);
        }
        for (uint32_t i = group_first.p[g]; i < group_first.p[g + 1]; i++) {
            for (uint32_t j = 0; j < n_bins.p[i]; j++) {           // the plain rule, written out once more
                const uint32_t k = rng.below(3) ? rng.below(4) : rng.below(n_keys), b = rng.below(3) != 0;
                keys.p[rec_off.p[i] + j] = uint16_t(b | (k << 1));
                uint32_t pos = out[2 * k], neg = out[2 * k + 1];
                recs.p[rec_off.p[i] + j] = uint16_t(b | (pos << 1) | (neg << 8));
                if (b) pos++; else neg++;
                if (pos + neg > 0x60) { pos = (pos + 1) / 2; neg = (neg + 1) / 2; }
                out[2 * k] = uint8_t(pos);
                out[2 * k + 1] = uint8_t(neg);
            }
            for (uint32_t j = n_bins.p[i]; j < (n_bins.p[i] + 7) / 8 * 8; j++) recs.p[rec_off.p[i] + j] = 0;
        }
    }
    auto call = [&](uint32_t poison) {
        for (uint32_t i = 0; i < n_slices; i++) { status.p[i] = 0; first_bad.p[i] = 0x55555555u; }
        return estv_emul_verify(keys.p, recs.p, rec_off.p, n_bins.p, n_slices, group_first.p, n_groups, with_in ? est_in.p : nullptr, est_out.p,
                                chunk, span, poison, status.p, first_bad.p, nullptr);
    };
    for (uint32_t poison : {0x00u, 0xffu, 0x5au}) {
        if (call(poison)) return fail("call failed", 0, 0, 0);
        for (uint32_t i = 0; i < n_slices; i++)
            if (first_bad.p[i] != kNone || status.p[i] != 0) return fail("finding on sound records (slice, first_bad, status)", i, first_bad.p[i], uint32_t(status.p[i]));
    }
    for (int round = 0; round < 12; round++) {             // one record altered: found at that very bin, and nothing before it in the batch
        const uint32_t i = rng.below(n_slices);
        if (!n_bins.p[i]) continue;
        const uint32_t j = rng.below(n_bins.p[i]);
        uint16_t &r = recs.p[rec_off.p[i] + j];
        const uint16_t keep = r;
        r = uint16_t(round % 3 == 0 ? r + 2 : round % 3 == 1 ? r + 0x100 : r ^ 1);
        if (call(0xff)) return fail("call failed", 0, 0, 0);
        r = keep;
        if (first_bad.p[i] != j || status.p[i] != kVerifyFailed) return fail("corruption not found (slice, bin, first_bad)", i, j, first_bad.p[i]);
        for (uint32_t s = 0; s < i; s++)
            if (first_bad.p[s] != kNone) return fail("finding before the corrupted slice (slice, first_bad)", s, first_bad.p[s], 0);
    }
    return 0;
}

}  // namespace

int main() {
    Rng rng{0x9e3779b97f4a7c15ull};
    int bad = 0;
    for (int k = 0; k < 24 && !bad; k++) {
        const uint32_t chunk = (const uint32_t[]){1024, 64, 16, 7}[k % 4], span = (const uint32_t[]){16, 3, 2, 1}[k % 4];
        bad |= run_case(rng, 1 + rng.below(20), chunk * span * 2 + 50, k % 2 ? 1026 : 40, chunk, span, (k / 2) % 2, k % 3);
    }
    // a long chain of pieces: more than one block of the start walk
    if (!bad) bad |= run_case(rng, 150, 40, 1026, 8, 2, true, 1);
    if (!bad) printf("ok\n");
    return bad;
}
