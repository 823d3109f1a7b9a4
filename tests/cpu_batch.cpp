// TEST INFRASTRUCTURE: a CPU stand-in for the part of the C ABI (include/avrecode_ms_amd.h) that the host side of the command line
// (csrc/host/avr_recode.h, csrc/host/recode_main.cpp) calls, with the oracle (oracle/) as the coder.  Linked with recode_main.cpp it
// gives a `recode` that runs both directions on a machine without a GPU: the plain reference of the whole command, which the product
// is compared against (tests/test_gpu_damaged_recode.py), and the build the damaged-container corpus runs under ASan + UBSan
// (tests/test_damaged_recode.py).  No HIP, no product library.
//
// THE DEFAULT ROUTE ONLY.  Slices of range records (avr_batch_add_slice_range) are coded by avr_oracle_range_encode, slices of
// resolved codes (avr_batch_add_slice_codes) by avr_oracle_cabac_encode_codes; statuses are the oracle's (a bin after a
// put_terminate(1): AVR_SLICE_BAD_RECORD, as on the device).  Key records (avr_batch_begin_group, avr_batch_add_slice_range_keys),
// the verify switches (avr_batch_set_verify, avr_batch_set_verify_k1) and avr_batch_expect are refused with AVR_ERR_INVALID and a
// message: AVR_DEVICE_ESTIMATORS, AVR_VERIFY, AVR_VERIFY_K1 and AVR_VERIFY_RESTORE end a run of this build with that message.
// AVR_CPU_BATCH_REPORT=1: avr_batch_run says on stderr how many slices and bins it was given (what a run had pending when it got
// as far as the coder).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/avrecode_ms_amd.h"
#include "../oracle/avr_oracle.h"

namespace {

thread_local std::string g_error;
int fail(int rc, const std::string &what) { g_error = what; return rc; }

struct slice {
    int kind;
    std::vector<uint16_t> recs;
    std::vector<uint8_t> codes, out;
    int status = AVR_SLICE_OK;
};

}  // namespace

struct avr_batch {
    size_t max_slices, max_bins, bins = 0;
    int kind = -1;
    bool ran = false;
    std::vector<slice> slices;
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

int not_here(const char *what) { return fail(AVR_ERR_INVALID, std::string("cpu_batch: ") + what + " is not part of the CPU stand-in (default route only)"); }

}  // namespace

extern "C" {

const char *avr_last_error(void) { return g_error.c_str(); }

avr_batch *avr_batch_create(int, size_t max_slices, size_t max_bins) {
    avr_batch *b = new avr_batch();
    b->max_slices = max_slices;
    b->max_bins = max_bins;
    return b;
}
void avr_batch_destroy(avr_batch *b) { delete b; }
int avr_batch_reset(avr_batch *b) {
    if (!b) return fail(AVR_ERR_INVALID, "cpu_batch: null batch");
    b->slices.clear();
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
int avr_batch_begin_group(avr_batch *, const uint8_t *) { return not_here("avr_batch_begin_group (key records)"); }
int avr_batch_add_slice_range_keys(avr_batch *, const uint16_t *, size_t) { return not_here("avr_batch_add_slice_range_keys (key records)"); }
int avr_batch_set_verify(avr_batch *, int on) { return on ? not_here("avr_batch_set_verify") : AVR_OK; }
int avr_batch_set_verify_k1(avr_batch *, int on) { return on ? not_here("avr_batch_set_verify_k1") : AVR_OK; }
int avr_batch_expect(avr_batch *, size_t, const uint8_t *, size_t) { return not_here("avr_batch_expect (the restore check)"); }

int avr_batch_run(avr_batch *b) {
    if (!b) return fail(AVR_ERR_INVALID, "cpu_batch: null batch");
    if (getenv("AVR_CPU_BATCH_REPORT")) fprintf(stderr, "[cpu_batch] %zu slices, %zu bins\n", b->slices.size(), b->bins);
    for (slice &s : b->slices) {
        int status = 0;
        size_t len;
        if (s.kind == AVR_KIND_RANGE) {                  // arithmetic_code<uint64_t, uint8_t>: a byte a renormalisation and the finish
            s.out.assign(s.recs.size() * 2 + 64, 0);
            len = avr_oracle_range_encode(s.recs.data(), s.recs.size(), s.out.data(), s.out.size(), &status);
        } else {                                         // cabac::encoder: at most 16 bits of output per bin in this coder's form
            s.out.assign(s.codes.size() * 2 + 64, 0);
            len = avr_oracle_cabac_encode_codes(s.codes.data(), s.codes.size(), s.out.data(), s.out.size(), &status);
        }
        s.status = status;                               // AVR_ORACLE_ERR_* and AVR_SLICE_* share their values
        s.out.resize(status == AVR_ORACLE_OK ? len : 0);
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

// nothing verifies here: the answers of a run with the switches off
int avr_batch_get_verify(avr_batch *, size_t, uint32_t *first_bad) { if (first_bad) *first_bad = AVR_VERIFY_NONE; return AVR_OK; }
int avr_batch_get_verify_est(avr_batch *, size_t, uint32_t *first_bad) { if (first_bad) *first_bad = AVR_VERIFY_NONE; return AVR_OK; }
int avr_batch_get_restore(avr_batch *, size_t, uint32_t *first_diff) { if (first_diff) *first_diff = AVR_VERIFY_NONE; return AVR_OK; }
int avr_batch_verify_ms(avr_batch *, float *ms) { if (ms) *ms = 0; return AVR_OK; }
int avr_batch_verify_est_ms(avr_batch *, float *ms) { if (ms) *ms = 0; return AVR_OK; }
int avr_batch_restore_ms(avr_batch *, float *ms) { if (ms) *ms = 0; return AVR_OK; }

size_t avr_drop_stop_byte(const uint8_t *buf, size_t len) { return avr_oracle_drop_stop_byte(buf, len); }
size_t avr_tail_patch(uint8_t *buf, size_t len, int length_parity, uint8_t last_byte) { return avr_oracle_tail_patch(buf, len, length_parity, last_byte); }

}  // extern "C"
