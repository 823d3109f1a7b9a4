// TEST INFRASTRUCTURE: a CPU stand-in for the part of the C ABI (include/avrecode_ms_amd.h) that the host side of the command line
// (csrc/host/avr_recode.h, csrc/host/recode_main.cpp) calls, with the oracle (oracle/) as the coder.  Linked with recode_main.cpp it
// gives a `recode` that runs every command on a machine without a GPU: the plain reference of the whole command, which the product
// is compared against (tests/test_gpu_damaged_recode.py, tests/test_gpu_cli_verify_faults.py), and the build that the
// damaged-container corpus and the verify switches' fault cases run under ASan + UBSan and TSan (tests/test_damaged_recode.py,
// tests/test_cli_verify_faults.py).  No HIP, no product library, and nothing of the product's verifiers (csrc/avr_verify.h,
// avr_cabac_verify.h, avr_est*.h, avr_restore.h): what it shares with them is the header of the C ABI.
//
// EVERY ROUTE OF THE COMMAND LINE.
//   * Slices of range records (avr_batch_add_slice_range) are coded by avr_oracle_range_encode, slices of resolved codes
//     (avr_batch_add_slice_codes) by avr_oracle_cabac_encode_codes; statuses are the oracle's (a bin after a put_terminate(1):
//     AVR_SLICE_BAD_RECORD for records, as on the device; for codes only here -- the device's coders from codes trust them, "resolved
//     codes have no bad value", and no recorder writes such a slice).
//   * Key records (avr_batch_begin_group, avr_batch_add_slice_range_keys; AVR_DEVICE_ESTIMATORS=1) are resolved per group by the
//     sequential rule -- a table of AVR_EST_KEYS {pos, neg} pairs, fresh {1, 1} or the caller's -- and then coded as range records.  A
//     malformed key: AVR_SLICE_BAD_RECORD for its slice and the rest of its group.  avr_batch_get_estimators: the group's table afterwards.
//   * avr_batch_set_verify (AVR_VERIFY=1): behind the encode every status-0 slice is decoded by avr_oracle_range_decode against its
//     records; the first differing bin fails the slice (AVR_SLICE_VERIFY_FAILED, avr_batch_get_verify).  With key records a second,
//     separate check: each resolved record against tests/est_plain.cpp's walk of the rule (avr_batch_get_verify_est).
//   * avr_batch_set_verify_k1 (AVR_VERIFY_K1=1): every status-0 slice of codes decoded by the decoder of H.264 9.3.1.2 / 9.3.3.2
//     (oracle/spec_cabac.c, avr_spec_cabac_decode_codes) against its codes.  The refusals are the product's: K2 verification of a K1
//     batch and K1 verification of a K2 batch are AVR_ERR_INVALID at avr_batch_run.
//   * avr_batch_expect (AVR_VERIFY_RESTORE=1): tail_patch(drop_stop_byte(coded bytes)) -- parity and last byte from the expectation,
//     as the container would carry them, no patch for an expectation shorter than two bytes -- against the expectation; the first
//     differing byte, or the shorter length where one is the beginning of the other (tests/restore_ref.py: first_diff), fails the
//     slice (avr_batch_get_restore).
//
// FAULT POINTS, the ones the device's test build has (csrc/avr_internal.h: TestHooks), read from the environment:
//     AVR_CPU_BATCH_FAULT="verify_flip=K,est_flip=K,est_flip_bin=M,restore_flip=K"
// K > 0 addresses slice K - 1 of the batch; K above the batch's slice count does nothing.  verify_flip: bit 7 of byte 0 of the slice's
// coded bytes complemented between the encode and the verifier, in a run that has that verifier on.  est_flip: one added to neg of
// bin est_flip_bin of the slice's resolved record between the resolver and the encode, in a run of key records with verify on.
// restore_flip: verify_flip in front of the restore check, in a run that carries it.
//
// AVR_CPU_BATCH_REPORT=1: avr_batch_run says on stderr how many slices and bins it was given (what a run had pending when it got
// as far as the coder).  AVR_CPU_BATCH_DUMP=<file>: avr_batch_run appends what it was given and what the coder made of it, before any
// fault point -- per run: kind, slice count; per slice: status, its records (resolved) or codes, its coded bytes, its expectation --
// for a test that works out a verifier's answer itself (tests/cli_verify_faults.py reads the format).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/avrecode_ms_amd.h"
#include "../oracle/avr_oracle.h"
#include "est_plain.cpp"

namespace {

thread_local std::string g_error;
int fail(int rc, const std::string &what) { g_error = what; return rc; }

struct slice {
    int kind;
    std::vector<uint16_t> recs;                          // range records; key records until the run resolves them (keys keeps them)
    std::vector<uint16_t> keys;
    std::vector<uint8_t> codes, out, expect;
    bool expected = false;
    int status = AVR_SLICE_OK;
    uint32_t first_bad = AVR_VERIFY_NONE, first_bad_est = AVR_VERIFY_NONE, first_diff = AVR_VERIFY_NONE;
};

struct estimators { uint8_t e[AVR_EST_KEYS][2]; };

struct group { size_t first; bool given; estimators in, out; };

struct faults { uint32_t verify_flip = 0, est_flip = 0, est_flip_bin = 0, restore_flip = 0; };

faults &fault_points() {                                 // "name=value,...": unknown names end the program, a typo must not pass for a sound run
    static faults f = [] {
        faults v;
        const char *p = getenv("AVR_CPU_BATCH_FAULT");
        std::string s = p ? p : "";
        for (size_t at = 0; at < s.size();) {
            size_t end = s.find(',', at);
            if (end == std::string::npos) end = s.size();
            const std::string pair = s.substr(at, end - at);
            const size_t eq = pair.find('=');
            const std::string name = pair.substr(0, eq);
            const uint32_t value = eq == std::string::npos ? 0u : uint32_t(strtoul(pair.c_str() + eq + 1, nullptr, 10));
            if (name == "verify_flip") v.verify_flip = value;
            else if (name == "est_flip") v.est_flip = value;
            else if (name == "est_flip_bin") v.est_flip_bin = value;
            else if (name == "restore_flip") v.restore_flip = value;
            else if (!name.empty()) { fprintf(stderr, "cpu_batch: unknown fault point %s\n", name.c_str()); exit(2); }
            at = end + 1;
        }
        return v;
    }();
    return f;
}

float ms_since(std::chrono::steady_clock::time_point t0) {   // never 0 for a check that ran: the host prints some lines only for a time > 0
    const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ms > 0.001f ? ms : 0.001f;
}

}  // namespace

struct avr_batch {
    size_t max_slices, max_bins, bins = 0;
    int kind = -1;
    bool ran = false, verify = false, verify_k1 = false;
    float verify_ms = 0, verify_est_ms = 0, restore_ms = 0;
    std::vector<slice> slices;
    std::vector<group> groups;
};

namespace {

int add(avr_batch *b, int kind, size_t n, slice **s) {
    if (!b) return fail(AVR_ERR_INVALID, "cpu_batch: null batch");
    if (b->ran) return fail(AVR_ERR_INVALID, "cpu_batch: the batch has run; reset it first");
    if (b->kind >= 0 && b->kind != kind) return fail(AVR_ERR_INVALID, "cpu_batch: a batch holds slices of one kind only");
    if (b->slices.size() >= b->max_slices || n > b->max_bins - b->bins) return fail(AVR_ERR_CAPACITY, "cpu_batch: more slices / bins than the batch was created for");
    b->kind = kind;
    b->bins += n;
    b->slices.emplace_back();
    *s = &b->slices.back();
    (*s)->kind = kind;
    return int(b->slices.size()) - 1;
}

// Key records -> range records, group by group: a bin is coded with its key's pair as it stands, then pos (bin 1) or neg (bin 0) goes
// up by one, and both are halved, rounding up, when their sum exceeds 0x60 (recode.cpp:823-827, 1037-1052).
void resolve_groups(avr_batch *b) {
    for (size_t g = 0; g < b->groups.size(); g++) {
        group &gr = b->groups[g];
        const size_t last = g + 1 < b->groups.size() ? b->groups[g + 1].first : b->slices.size();
        estimators tab;
        if (gr.given) tab = gr.in; else memset(&tab, 1, sizeof tab);
        bool ok = true;
        for (size_t i = gr.first; i < last; i++) {
            slice &s = b->slices[i];
            for (uint16_t k : s.keys) ok = ok && (k >> 1) < AVR_EST_KEYS;
            if (!ok) { s.status = AVR_SLICE_BAD_RECORD; s.recs.clear(); continue; }
            s.recs.resize(s.keys.size());
            for (size_t j = 0; j < s.keys.size(); j++) {
                uint8_t *e = tab.e[s.keys[j] >> 1];
                const unsigned bin = s.keys[j] & 1u;
                s.recs[j] = uint16_t(bin | unsigned(e[0]) << 1 | unsigned(e[1]) << 8);
                if (bin) e[0]++; else e[1]++;
                if (unsigned(e[0]) + unsigned(e[1]) > 0x60) { e[0] = uint8_t((e[0] + 1) >> 1); e[1] = uint8_t((e[1] + 1) >> 1); }
            }
        }
        gr.out = tab;
    }
}

// The estimator check: the records the encoder read against tests/est_plain.cpp's walk of the same key records, slice by slice.
void check_estimators(avr_batch *b) {
    const size_t n = b->slices.size();
    std::vector<uint64_t> rec_off(n + 1, 0);
    std::vector<uint32_t> n_bins(n), group_first;
    for (size_t i = 0; i < n; i++) {
        n_bins[i] = uint32_t(b->slices[i].keys.size());
        rec_off[i + 1] = rec_off[i] + ((n_bins[i] + 7) & ~size_t(7));
    }
    std::vector<uint16_t> keys(rec_off[n] + 8, 0), want(rec_off[n] + 8, 0);
    for (size_t i = 0; i < n; i++) std::copy(b->slices[i].keys.begin(), b->slices[i].keys.end(), keys.begin() + rec_off[i]);
    std::vector<uint8_t> est_in;
    bool any_given = false;
    for (const group &g : b->groups) { group_first.push_back(uint32_t(g.first)); any_given = any_given || g.given; }
    group_first.push_back(uint32_t(n));
    if (any_given) {
        est_in.resize(b->groups.size() * sizeof(estimators), 1);
        for (size_t g = 0; g < b->groups.size(); g++)
            if (b->groups[g].given) memcpy(&est_in[g * sizeof(estimators)], &b->groups[g].in, sizeof(estimators));
    }
    std::vector<int32_t> status(n, 0);
    est_plain_resolve(keys.data(), rec_off.data(), n_bins.data(), group_first.data(), uint32_t(b->groups.size()), any_given ? est_in.data() : nullptr,
                      nullptr, want.data(), status.data());
    for (size_t i = 0; i < n; i++) {
        slice &s = b->slices[i];
        if (s.status != AVR_SLICE_OK && s.status != AVR_SLICE_VERIFY_FAILED) continue;
        for (size_t j = 0; j < s.recs.size() && s.first_bad_est == AVR_VERIFY_NONE; j++)
            if (s.recs[j] != want[rec_off[i] + j]) s.first_bad_est = uint32_t(j);
        if (s.first_bad_est != AVR_VERIFY_NONE) s.status = AVR_SLICE_VERIFY_FAILED;
    }
}

uint32_t restore_first_diff(const slice &s) {            // the rule of tests/restore_ref.py, on the oracle's two helpers
    std::vector<uint8_t> r(s.out.size() + 1, 0);
    std::copy(s.out.begin(), s.out.end(), r.begin());
    size_t len = avr_oracle_drop_stop_byte(r.data(), s.out.size());
    if (s.expect.size() >= 2) len = avr_oracle_tail_patch(r.data(), len, int(s.expect.size() & 1), s.expect.back());
    const size_t n = std::min(len, s.expect.size());
    for (size_t j = 0; j < n; j++)
        if (r[j] != s.expect[j]) return uint32_t(j);
    return len != s.expect.size() ? uint32_t(n) : AVR_VERIFY_NONE;
}

void put32(FILE *f, uint32_t v) { fwrite(&v, 4, 1, f); }
void dump(const avr_batch *b, const char *path) {
    FILE *f = fopen(path, "ab");
    if (!f) return;
    put32(f, 0x42525641u);                               // "AVRB"
    put32(f, uint32_t(b->kind));
    put32(f, uint32_t(b->slices.size()));
    for (const slice &s : b->slices) {
        put32(f, uint32_t(s.status));
        if (s.kind == AVR_KIND_CABAC_CODES) { put32(f, uint32_t(s.codes.size())); fwrite(s.codes.data(), 1, s.codes.size(), f); }
        else { put32(f, uint32_t(s.recs.size())); fwrite(s.recs.data(), 2, s.recs.size(), f); }
        put32(f, uint32_t(s.out.size()));
        fwrite(s.out.data(), 1, s.out.size(), f);
        put32(f, s.expected ? uint32_t(s.expect.size()) : AVR_EXPECT_NONE);
        if (s.expected) fwrite(s.expect.data(), 1, s.expect.size(), f);
    }
    fclose(f);
}

void flip(avr_batch *b, uint32_t k) {                    // slice k - 1: bit 7 of byte 0 of its coded bytes
    if (k && k <= b->slices.size() && !b->slices[k - 1].out.empty()) b->slices[k - 1].out[0] ^= 0x80u;
}

}  // namespace

extern "C" {

const char *avr_last_error(void) { return g_error.c_str(); }

// The test build's call (csrc/avr_api.cpp, AVR_TEST_HOOKS), for a test that loads the stand-in as a library and changes the fault points
// between runs: one of the four names above, or "reset" (all off).  Not for use while another thread runs a batch.
int avr_test_hook_set(const char *name, uint32_t value) {
    faults &f = fault_points();
    const std::string n = name ? name : "";
    if (n == "reset") f = faults{};
    else if (n == "verify_flip") f.verify_flip = value;
    else if (n == "est_flip") f.est_flip = value;
    else if (n == "est_flip_bin") f.est_flip_bin = value;
    else if (n == "restore_flip") f.restore_flip = value;
    else return fail(AVR_ERR_INVALID, "cpu_batch: unknown fault point " + n);
    return AVR_OK;
}

avr_batch *avr_batch_create(int, size_t max_slices, size_t max_bins) {
    avr_batch *b = new avr_batch();
    b->max_slices = max_slices;
    b->max_bins = max_bins;
    return b;
}
void avr_batch_destroy(avr_batch *b) { delete b; }
int avr_batch_reset(avr_batch *b) {                      // the verify settings stay, as the product's do
    if (!b) return fail(AVR_ERR_INVALID, "cpu_batch: null batch");
    b->slices.clear();
    b->groups.clear();
    b->bins = 0;
    b->kind = -1;
    b->ran = false;
    return AVR_OK;
}

int avr_batch_add_slice_range(avr_batch *b, const uint16_t *recs, size_t n) {
    slice *s;
    const int idx = add(b, AVR_KIND_RANGE, n, &s);
    if (idx >= 0) s->recs.assign(recs, recs + n);
    return idx;
}
int avr_batch_add_slice_codes(avr_batch *b, const uint8_t *codes, size_t n) {
    slice *s;
    const int idx = add(b, AVR_KIND_CABAC_CODES, n, &s);
    if (idx >= 0) s->codes.assign(codes, codes + n);
    return idx;
}
int avr_batch_begin_group(avr_batch *b, const uint8_t *est_in) {
    if (!b) return fail(AVR_ERR_INVALID, "cpu_batch: null batch");
    if (b->ran) return fail(AVR_ERR_INVALID, "cpu_batch: the batch has run; reset it first");
    if (b->kind >= 0 && b->kind != AVR_KIND_RANGE_KEYS) return fail(AVR_ERR_INVALID, "cpu_batch: a batch holds slices of one kind only");
    group g{};
    g.first = b->slices.size();
    g.given = est_in != nullptr;
    if (est_in) {
        memcpy(&g.in, est_in, sizeof g.in);
        for (size_t k = 0; k < AVR_EST_KEYS; k++)
            if (!g.in.e[k][0] || !g.in.e[k][1] || unsigned(g.in.e[k][0]) + unsigned(g.in.e[k][1]) > 0x60)
                return fail(AVR_ERR_INVALID, "cpu_batch: an estimator with pos or neg 0, or pos + neg above 0x60");
    }
    b->groups.push_back(g);                              // (a group may stay without a slice, as in the product: its table afterwards is its start table)
    b->kind = AVR_KIND_RANGE_KEYS;
    return int(b->groups.size()) - 1;
}
int avr_batch_add_slice_range_keys(avr_batch *b, const uint16_t *recs, size_t n) {
    if (b && !b->ran && b->groups.empty() && (b->kind < 0 || b->kind == AVR_KIND_RANGE_KEYS)) {   // the first slice opens a fresh group
        const int rc = avr_batch_begin_group(b, nullptr);
        if (rc < 0) return rc;
    }
    slice *s;
    const int idx = add(b, AVR_KIND_RANGE_KEYS, n, &s);
    if (idx >= 0) s->keys.assign(recs, recs + n);
    return idx;
}
int avr_batch_get_estimators(avr_batch *b, size_t g, const uint8_t **pos_neg, size_t *n_keys) {
    if (!b || !b->ran) return fail(AVR_ERR_INVALID, "cpu_batch: avr_batch_get_estimators before avr_batch_run");
    if (g >= b->groups.size()) return fail(AVR_ERR_INVALID, "cpu_batch: group index out of range");
    if (pos_neg) *pos_neg = &b->groups[g].out.e[0][0];
    if (n_keys) *n_keys = AVR_EST_KEYS;
    return AVR_OK;
}
int avr_batch_set_verify(avr_batch *b, int on) {
    if (!b) return fail(AVR_ERR_INVALID, "cpu_batch: null batch");
    b->verify = on != 0;
    return AVR_OK;
}
int avr_batch_set_verify_k1(avr_batch *b, int on) {
    if (!b) return fail(AVR_ERR_INVALID, "cpu_batch: null batch");
    b->verify_k1 = on != 0;
    return AVR_OK;
}
int avr_batch_expect(avr_batch *b, size_t i, const uint8_t *bytes, size_t len) {
    if (!b) return fail(AVR_ERR_INVALID, "cpu_batch: null batch");
    if (b->ran) return fail(AVR_ERR_INVALID, "cpu_batch: the batch has run; reset it first");
    if (b->kind != AVR_KIND_CABAC_CODES) return fail(AVR_ERR_INVALID, "cpu_batch: a K2 batch takes no expectations");
    if (i >= b->slices.size()) return fail(AVR_ERR_INVALID, "cpu_batch: an expectation for a slice that has not been added");
    if (b->slices[i].expected) return fail(AVR_ERR_INVALID, "cpu_batch: a second expectation for one slice");
    if (len >= 0xFFFFFFFFu || (!bytes && len)) return fail(AVR_ERR_INVALID, "cpu_batch: an expectation of 2^32 - 1 bytes or more, or null bytes");
    b->slices[i].expected = true;
    b->slices[i].expect.assign(bytes, bytes + len);
    return AVR_OK;
}

int avr_batch_run(avr_batch *b) {
    if (!b) return fail(AVR_ERR_INVALID, "cpu_batch: null batch");
    if (getenv("AVR_CPU_BATCH_REPORT")) fprintf(stderr, "[cpu_batch] %zu slices, %zu bins\n", b->slices.size(), b->bins);
    const bool k1 = b->kind == AVR_KIND_CABAC_CODES, keys = b->kind == AVR_KIND_RANGE_KEYS;
    if (b->verify && k1) return fail(AVR_ERR_INVALID, "cpu_batch: verification exists for the compress direction only: not for a K1 batch");
    if (b->verify_k1 && b->kind >= 0 && !k1) return fail(AVR_ERR_INVALID, "cpu_batch: K1 verification exists for the decompress direction only: not for a K2 batch");
    const faults &f = fault_points();
    const size_t n = b->slices.size();
    b->verify_ms = b->verify_est_ms = b->restore_ms = 0;
    for (slice &s : b->slices) { s.status = AVR_SLICE_OK; s.first_bad = s.first_bad_est = s.first_diff = AVR_VERIFY_NONE; }
    if (keys) {
        resolve_groups(b);
        if (b->verify && f.est_flip && f.est_flip <= n) {
            slice &s = b->slices[f.est_flip - 1];
            if (s.status == AVR_SLICE_OK && f.est_flip_bin < s.recs.size()) s.recs[f.est_flip_bin] += 0x100u;
        }
    }
    for (slice &s : b->slices) {
        if (s.status != AVR_SLICE_OK) { s.out.clear(); continue; }
        int status = 0;
        size_t len;
        if (!k1) {                                       // arithmetic_code<uint64_t, uint8_t>: a byte a renormalisation and the finish
            s.out.assign(s.recs.size() * 2 + 64, 0);
            len = avr_oracle_range_encode(s.recs.data(), s.recs.size(), s.out.data(), s.out.size(), &status);
        } else {                                         // cabac::encoder: at most 16 bits of output per bin in this coder's form
            s.out.assign(s.codes.size() * 2 + 64, 0);
            len = avr_oracle_cabac_encode_codes(s.codes.data(), s.codes.size(), s.out.data(), s.out.size(), &status);
        }
        s.status = status;                               // AVR_ORACLE_ERR_* and AVR_SLICE_* share their values
        s.out.resize(status == AVR_ORACLE_OK ? len : 0);
    }
    if (const char *path = getenv("AVR_CPU_BATCH_DUMP")) dump(b, path);
    if (b->verify && !k1 && n) {
        const auto t0 = std::chrono::steady_clock::now();
        flip(b, f.verify_flip);
        for (slice &s : b->slices) {
            if (s.status != AVR_SLICE_OK || s.recs.empty()) continue;
            std::vector<uint8_t> bins(s.recs.size()), bytes(s.out);
            bytes.push_back(0);                          // (never null for the decoder)
            avr_oracle_range_decode(bytes.data(), s.out.size(), s.recs.data(), s.recs.size(), bins.data());
            for (size_t j = 0; j < bins.size() && s.first_bad == AVR_VERIFY_NONE; j++)
                if (bins[j] != (s.recs[j] & 1u)) s.first_bad = uint32_t(j);
            if (s.first_bad != AVR_VERIFY_NONE) s.status = AVR_SLICE_VERIFY_FAILED;
        }
        b->verify_ms = ms_since(t0);
        if (keys) {
            const auto t1 = std::chrono::steady_clock::now();
            check_estimators(b);
            b->verify_est_ms = ms_since(t1);
        }
    }
    if (b->verify_k1 && k1 && n) {
        const auto t0 = std::chrono::steady_clock::now();
        flip(b, f.verify_flip);
        for (slice &s : b->slices) {
            if (s.status != AVR_SLICE_OK || s.codes.empty()) continue;
            std::vector<uint8_t> bins(s.codes.size()), bytes(s.out);
            bytes.push_back(0);
            avr_spec_cabac_decode_codes(bytes.data(), s.out.size(), s.codes.data(), s.codes.size(), bins.data());
            for (size_t j = 0; j < bins.size() && s.first_bad == AVR_VERIFY_NONE; j++)
                if (bins[j] != (s.codes[j] & 1u)) s.first_bad = uint32_t(j);
            if (s.first_bad != AVR_VERIFY_NONE) s.status = AVR_SLICE_VERIFY_FAILED;
        }
        b->verify_ms = ms_since(t0);
    }
    bool restored = false;
    for (const slice &s : b->slices) restored = restored || s.expected;
    if (restored) {
        const auto t0 = std::chrono::steady_clock::now();
        flip(b, f.restore_flip);
        for (slice &s : b->slices) {
            if (!s.expected || (s.status != AVR_SLICE_OK && s.status != AVR_SLICE_VERIFY_FAILED)) continue;
            s.first_diff = restore_first_diff(s);
            if (s.first_diff != AVR_VERIFY_NONE) s.status = AVR_SLICE_VERIFY_FAILED;
        }
        b->restore_ms = ms_since(t0);
    }
    b->ran = true;
    return AVR_OK;
}

int avr_batch_get(avr_batch *b, size_t i, const uint8_t **bytes, size_t *len, int *status) {
    if (!b || !b->ran) return fail(AVR_ERR_INVALID, "cpu_batch: avr_batch_get before avr_batch_run");
    if (i >= b->slices.size()) return fail(AVR_ERR_INVALID, "cpu_batch: slice index out of range");
    if (bytes) *bytes = b->slices[i].out.data();
    if (len) *len = b->slices[i].out.size();
    if (status) *status = b->slices[i].status;
    return AVR_OK;
}

#define CPU_BATCH_ANSWER(name, field)                                                                       \
    int name(avr_batch *b, size_t i, uint32_t *v) {                                                         \
        if (!b || !b->ran) return fail(AVR_ERR_INVALID, "cpu_batch: " #name " before avr_batch_run");       \
        if (i >= b->slices.size()) return fail(AVR_ERR_INVALID, "cpu_batch: slice index out of range");     \
        if (v) *v = b->slices[i].field;                                                                     \
        return AVR_OK;                                                                                      \
    }
CPU_BATCH_ANSWER(avr_batch_get_verify, first_bad)
CPU_BATCH_ANSWER(avr_batch_get_verify_est, first_bad_est)
CPU_BATCH_ANSWER(avr_batch_get_restore, first_diff)
int avr_batch_verify_ms(avr_batch *b, float *ms) { if (ms) *ms = b ? b->verify_ms : 0; return AVR_OK; }
int avr_batch_verify_est_ms(avr_batch *b, float *ms) { if (ms) *ms = b ? b->verify_est_ms : 0; return AVR_OK; }
int avr_batch_restore_ms(avr_batch *b, float *ms) { if (ms) *ms = b ? b->restore_ms : 0; return AVR_OK; }

size_t avr_drop_stop_byte(const uint8_t *buf, size_t len) { return avr_oracle_drop_stop_byte(buf, len); }
size_t avr_tail_patch(uint8_t *buf, size_t len, int length_parity, uint8_t last_byte) { return avr_oracle_tail_patch(buf, len, length_parity, last_byte); }

}  // extern "C"
