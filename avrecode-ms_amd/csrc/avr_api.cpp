// C ABI of the MI355X arithmetic re-encode path (include/avrecode_ms_amd.h).
//
// The batch object is the build's counterpart of the reference's per-slice coder objects
// (compressor::cabac_decoder::encoder, recode.cpp:1270; decompressor::cabac_decoder::
// cabac_encoder, recode.cpp:1525): the hook adapter records bins, a batch codes them.
// There is no CPU coding path in this library: without a HIP device every run fails with
// AVR_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "avr_cabac_verify.h"
#include "avr_internal.h"
#include "avr_multi.h"
#include "avr_plan.h"
#include "avr_plan_dev.h"
#include "avr_synth.h"
#include "avr_tables.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(AVR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

#define AVR_HIP(call)                                            \
    do {                                                         \
        hipError_t e_ = (call);                                  \
        if (e_ != hipSuccess) return hip_fail(e_, #call);        \
    } while (0)

constexpr avr::CabacTables kTables = avr::make_cabac_tables();

int select_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(AVR_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU coding path");
    if (device < 0 || device >= n) return fail(AVR_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
    AVR_HIP(hipSetDevice(device));
    return AVR_OK;
}

// Memory of the device (DevBuf) or pinned memory of the host (PinBuf) that grows and never shrinks; reserve keeps nothing of what
// the buffer held.  A buffer owns its memory: it moves, it is not copied, and whoever holds it need not release it.
template <class T, bool Pinned>
struct Buf {
    T *p = nullptr;
    size_t cap = 0;       // elements
    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Buf() { release(); }
    int reserve(size_t n) {
        if (n <= cap) return AVR_OK;
        release();
        size_t want = n + n / 8 + 64;
        hipError_t e = Pinned ? hipHostMalloc(reinterpret_cast<void **>(&p), want * sizeof(T), hipHostMallocDefault)
                              : hipMalloc(reinterpret_cast<void **>(&p), want * sizeof(T));
        if (e != hipSuccess) return fail(AVR_ERR_NOMEM, "%s(%zu bytes): %s", Pinned ? "hipHostMalloc" : "hipMalloc", want * sizeof(T), hipGetErrorString(e));
        cap = want;
        return AVR_OK;
    }
    void release() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinBuf = Buf<T, true>;

// N timing events, made together or not at all: a create that fails leaves none behind, and the next one tries again.
template <int N>
struct Events {
    hipEvent_t e[N] = {};
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() { clear(); }
    void clear() { for (auto &x : e) { if (x) (void)hipEventDestroy(x); x = nullptr; } }
    hipError_t create() {                                        // (the caller has selected the device)
        if (e[0]) return hipSuccess;
        for (auto &x : e)
            if (hipError_t err = hipEventCreate(&x); err != hipSuccess) { clear(); return err; }
        return hipSuccess;
    }
    hipEvent_t operator[](int i) const { return e[i]; }
};

// A batch's stream.  Declared in front of everything that may have work on it, so destroyed behind all of that.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) { avr::forget_part_streams(s); avr::forget_stream(s); (void)hipStreamDestroy(s); } }
    operator hipStream_t() const { return s; }
};

int check_states8(size_t n_states) {
    if (n_states > AVR_MAX_STATES8)
        return fail(AVR_ERR_INVALID, "n_states %zu > %d: one-byte records name at most %d contexts", n_states, AVR_MAX_STATES8, AVR_MAX_STATES8);
    return AVR_OK;
}

// A check behind the encode of a run.  A batch has three: the verifier of its kind, the estimator checker, the restore check.  Which
// settings arm one, which kernel it launches and what else that kernel reads stay with the check; this is what the three share.
// Off by default, and then none of this is touched: the events are made when the check is first asked for, the arrays when first armed.
struct Check {
    bool on = false;                        // the run in flight / the last run had it
    Events<2> ev;                           // its start and end, as last recorded
    float ms = 0, before = 0;               // what it took; of that, in front of K1p's second pass (where there was one)
    DevBuf<uint32_t> d_first;               // per slice: the first bin (byte) it found wrong, AVR_VERIFY_NONE for none
    PinBuf<uint32_t> h_first;

    int make_events(int device) {
        if (ev[0]) return AVR_OK;
        if (int rc = select_device(device)) return rc;
        if (hipError_t e = ev.create(); e != hipSuccess) return hip_fail(e, "hipEventCreate(&e)");
        return AVR_OK;
    }
    // at submit: whether this run has the check, and room for the answers of n slices
    int arm(bool has, size_t n) {
        on = has; before = 0;
        if (!on) return AVR_OK;
        if (int rc = d_first.reserve(n)) return rc;
        return h_first.reserve(n);
    }
    int start(hipStream_t s) { AVR_HIP(hipEventRecord(ev[0], s)); return AVR_OK; }
    int end(hipStream_t s) { AVR_HIP(hipEventRecord(ev[1], s)); return AVR_OK; }
    int fetch(hipStream_t s, size_t n) {
        if (on) AVR_HIP(hipMemcpyAsync(h_first.p, d_first.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        return AVR_OK;
    }
    uint32_t answer(size_t slice) const { return on ? h_first.p[slice] : AVR_VERIFY_NONE; }
    float span() const { float t = 0; if (on) (void)hipEventElapsedTime(&t, ev[0], ev[1]); return t; }
    void carry() { before = span(); }       // in front of a second pass, which records both events again
    void finish() { ms = before + span(); }
};

}  // namespace

struct avr_batch {
    int device = 0;
    size_t max_slices = 0, max_bins = 0, total_bins = 0;
    int kind = -1;
    bool recs8 = false;                     // the slices came as one-byte records (AVR_KIND_CABAC8); kind is AVR_KIND_CABAC
    bool keys = false;                      // the slices came as key records (AVR_KIND_RANGE_KEYS); kind is AVR_KIND_RANGE
    bool keys8 = false;                     // ... as one-byte key records (AVR_KIND_RANGE_KEYS8: keys is set too), or avr_batch_begin_group8 said they will
    size_t n_states = 0;
    bool ran = false;
    Stream stream;
    Events<5> ev;
    float ms[4] = {0, 0, 0, 0};
    // Nothing below is released by name: every buffer and event frees itself, behind this -- the device selected, the stream drained --
    // and in front of the stream's own end.
    ~avr_batch() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }

    // host side
    PinBuf<uint16_t> h_recs;
    PinBuf<uint8_t> h_states, h_out, h_final;
    PinBuf<uint32_t> h_out_len;
    PinBuf<int32_t> h_status;
    std::vector<uint64_t> rec_off;          // n+1, records, multiples of 8
    std::vector<uint32_t> n_bins;
    std::vector<uint64_t> dense_off;        // n+1, bytes in h_out

    // device side
    DevBuf<uint16_t> d_recs;
    DevBuf<uint8_t> d_recs8;                // one-byte records as they came over PCIe (what the kernels read: no two-byte copy)
    DevBuf<uint4> d_tiles;
    DevBuf<uint64_t> d_rec_off, d_tile_off, d_out_off, d_dense_off;
    DevBuf<uint32_t> d_n_bins, d_order, d_out_len;
    DevBuf<int32_t> d_status;
    DevBuf<uint8_t> d_states, d_final, d_out, d_dense;

    // intra-slice parallel path (K1p): plan arrays + workspace
    DevBuf<uint64_t> d_res_off, d_dig_off;
    DevBuf<uint32_t> d_chunk_base, d_chunk_slice, d_blk_base, d_blk_slice;
    DevBuf<uint8_t> d_workspace;
    int last_path = 0;                      // 0 = one lane per slice, 1 = chunked

    // key records: the groups (first slice of each), their start tables where the caller gave one, the tables after the run
    std::vector<uint32_t> group_first;
    std::vector<uint8_t> est_in;            // one table a group, fresh ones included
    PinBuf<uint8_t> h_est_in, h_est_out;
    // any_est_in only spares a copy: est_in holds a table for every group, {1, 1} for the fresh ones, so a run that sends it computes
    // what a run without start tables computes.  Nothing goes wrong while it is true; avr_batch_reset clears it to spare the copy again.
    bool any_est_in = false, est_out_fetched = false;
    DevBuf<uint16_t> d_keys;
    DevBuf<uint32_t> d_group_first;
    DevBuf<uint8_t> d_est_in, d_est_out, d_est_ws;

    // submit / wait: nothing the device reads may be pageable or local to a call
    PinBuf<uint8_t> h_plan;                 // the plan arrays of the run in flight
    size_t plan_used = 0;
    PinBuf<uint32_t> h_ndense;              // [0]: contexts the batch uses, read back behind the kernels
    avr::HostPlan hp;                       // of the run in flight: the output regions (out_off: n+1, bytes in d_out), the path's plan arrays
    bool in_flight = false;
    uint32_t dense_hint = 0;                // context rows the previous run of this object needed (0: no run yet)
    uint32_t hint_used = 0;                 // what the run in flight was sized by (0: it asked the device and waited)
    uint32_t info[4] = {0, 0, 0, 0};        // avr_batch_run_info
    avr_chunk_plan plan{};                  // of the run in flight (device arrays of this batch)

    // verification of a run (K2: avr_batch_set_verify, K1: avr_batch_set_verify_k1): off by default, and then none of this is touched
    bool verify = false;                    // the setting: the next submit of a K2 batch enqueues the verifier behind the encode
    bool verify_k1 = false;                 // the same for a K1 batch (avr_cabac_verify.hip)
    Check verifier;                         // armed by the setting of the batch's kind (events: made when either is first set)
    // ... and of a run of key records the estimator checker (avr_est_verify.hip) behind it
    Check est_checker;                      // armed by verify, for key records (events: made when verify is first set)
    // the restore check of a K1 run (avr_batch_expect): a batch without expectations touches none of this
    Check restorer;                         // armed by any expectation (events: made with the first one)
    std::vector<uint64_t> expect_off;       // per slice: where its expectation lies in h_expect (bytes, multiples of 8)
    std::vector<uint32_t> expect_len;       // per slice: its length, AVR_EXPECT_NONE for a slice without one
    size_t n_expect = 0, expect_used = 0;   // slices that have one; bytes of h_expect in use (a multiple of 8)
    PinBuf<uint8_t> h_expect;               // the expectations as they came, each padded to 8
    DevBuf<uint8_t> d_expect;
    DevBuf<uint64_t> d_expect_off;
    DevBuf<uint32_t> d_expect_len;
    // the three in the order they run in; the encode's slot of the timings ends where the first of them that a run has starts
    std::array<Check *, 3> checks() { return {&verifier, &est_checker, &restorer}; }

    // The arrays of the run in flight as the launchers take them (avr_internal.h), made once at submit: what its encoder read, for the
    // verifier behind it to read the same; its context states (a K1 batch of records; none otherwise); its coded output.
    avr::Slices read;
    avr::States states;
    avr::Output output;
    // the key records of a run that has them, as the resolver and the estimator checker read them
    avr::Slices key_records() const { return {d_keys.p, d_rec_off.p, d_n_bins.p, nullptr, uint32_t(n_bins.size()), false, {}, keys8 ? 1u : 2u}; }
    size_t est_keys() const { return keys8 ? AVR_EST_KEYS8 : AVR_EST_KEYS; }      // estimators to a table of this batch ...
    size_t est_table() const { return est_keys() * 2; }                           // ... and its bytes
    uint32_t est_pad() const { return keys8 ? avr::est::kKeysPad8 : avr::est::kKeysPad; }
};

// The refusals the entry points open with.  check_idle: for what changes a batch between runs; check_open: for what adds to a batch
// that has not run yet; check_ran, check_slice: for the getters (more: the caller's other pointers).
static int check_idle(const avr_batch *b) {
    if (!b) return fail(AVR_ERR_INVALID, "null batch");
    if (b->in_flight) return fail(AVR_ERR_INVALID, "batch is in flight; call avr_batch_wait first");
    return AVR_OK;
}
static int check_open(const avr_batch *b) {
    if (int rc = check_idle(b)) return rc;
    if (b->ran) return fail(AVR_ERR_INVALID, "batch already ran; call avr_batch_reset first");
    return AVR_OK;
}
static int check_ran(const avr_batch *b, bool more = true) {
    if (!b || !b->ran || !more) return fail(AVR_ERR_INVALID, "batch has not run");
    return AVR_OK;
}
static int check_slice(const avr_batch *b, size_t slice) {
    if (int rc = check_ran(b)) return rc;
    if (slice >= b->n_bins.size()) return fail(AVR_ERR_INVALID, "slice %zu out of range", slice);
    return AVR_OK;
}

// One plan array to the device through the batch's pinned arena: the copy is asynchronous for real (a copy from
// pageable memory is staged by the runtime inside the call), and the source stays put until avr_batch_wait.
template <class T>
static int stage_h2d(avr_batch *b, T *dst, const T *src, size_t n) {
    const size_t bytes = n * sizeof(T), at = (b->plan_used + 63) & ~size_t(63);
    if (at + bytes > b->h_plan.cap) return fail(AVR_ERR_NOMEM, "plan staging area too small (%zu + %zu > %zu)", at, bytes, b->h_plan.cap);
    memcpy(b->h_plan.p + at, src, bytes);
    b->plan_used = at + bytes;
    AVR_HIP(hipMemcpyAsync(dst, b->h_plan.p + at, bytes, hipMemcpyHostToDevice, b->stream));
    return AVR_OK;
}
// What an array of n elements takes of the arena (h_plan) at most: stage_h2d starts each at a multiple of 64.  A run reserves the
// sum over the arrays it stages, so an array added to a run is added to its sum; avr_batch_wait's dense_off, staged when the run's
// arrays are consumed, is no larger than the rec_off every run stages.
template <class T>
static constexpr size_t staged(size_t n) { return n * sizeof(T) + 64; }
static size_t staged_plan(const avr::HostPlan &h) { return h.staged_bytes() + 6 * 64; }

// The arrays of the run's plan (b->hp) on their way to the device, each into room of its own there; *plan: the device's view of them.
// An array the path does not read is empty and stays where it is.  res_total: of res_off, whoever staged it.
static int stage_plan(avr_batch *b, uint64_t res_total, avr_chunk_plan *plan) {
    const avr::HostPlan &h = b->hp;
    auto put = [b](auto &d, const auto &v) { const int rc = d.reserve(v.size()); return rc || v.empty() ? rc : stage_h2d(b, d.p, v.data(), v.size()); };
    int rc;
    if ((rc = put(b->d_res_off, h.res_off)) || (rc = put(b->d_dig_off, h.dig_off)) || (rc = put(b->d_chunk_base, h.chunk_base)) ||
        (rc = put(b->d_blk_base, h.blk_base)) || (rc = put(b->d_chunk_slice, h.chunk_slice)) || (rc = put(b->d_blk_slice, h.blk_slice)))
        return rc;
    const bool blocks = !h.blk_base.empty();
    *plan = {b->d_res_off.p, b->d_chunk_base.p, b->d_chunk_slice.p, blocks ? b->d_blk_base.p : nullptr, blocks ? b->d_blk_slice.p : nullptr,
             b->d_dig_off.p, res_total, avr::plan_total(h.dig_off), avr::plan_total(h.chunk_base), avr::plan_total(h.blk_base)};
    return AVR_OK;
}
// few, long slices: the intra-slice parallel kernels; many short ones: one lane per slice (avr::want_chunked, or as AVR_K1_PATH says)
static bool pick_chunked(const avr_batch *b) { return avr::k1_path() ? avr::k1_path() == 2 : avr::want_chunked(b->n_bins.size(), b->total_bins); }

namespace avr {
// the three environment switches of the library (avr_internal.h), read once
const Env &env() {
    static const Env e = [] {
        Env v{0, false, false};
        if (const char *p = getenv("AVR_K1_PATH")) v.k1_path = strcmp(p, "chunked") == 0 ? 2 : strcmp(p, "serial") == 0 ? 1 : 0;
        v.no_dense = getenv("AVR_NO_DENSE") != nullptr;
        v.no_hint = getenv("AVR_BATCH_NO_HINT") != nullptr;
        return v;
    }();
    return e;
}
#ifdef AVR_TEST_HOOKS
TestHooks &test_hooks() { static TestHooks h{}; return h; }
#endif
}  // namespace avr

extern "C" {

#ifdef AVR_TEST_HOOKS
// Test build only (libavrecode_hip_hooks.so): set a hook by name; returns AVR_ERR_INVALID for an unknown name.
int avr_test_hook_set(const char *name, uint32_t value) {
    static const struct { const char *name; uint32_t avr::TestHooks::*field; } kHooks[] = {
#define AVR_HOOK(f) {#f, &avr::TestHooks::f}
        AVR_HOOK(k1p_force_retry_every), AVR_HOOK(census_stride),
        AVR_HOOK(k1_path), AVR_HOOK(no_dense), AVR_HOOK(no_hint), AVR_HOOK(k2p_seg_len), AVR_HOOK(local_waves), AVR_HOOK(k2p_wave),
        AVR_HOOK(k1p_keep_retry), AVR_HOOK(chain_nsegs), AVR_HOOK(chain_whole),
        AVR_HOOK(chain_segments), AVR_HOOK(chain_force_redo), AVR_HOOK(verify_flip), AVR_HOOK(est_flip), AVR_HOOK(est_flip_bin),
        AVR_HOOK(restore_flip),
#undef AVR_HOOK
    };
    avr::TestHooks &h = avr::test_hooks();
    if (!name) return fail(AVR_ERR_INVALID, "null hook name");
    if (!strcmp(name, "reset")) { h = avr::TestHooks{}; return AVR_OK; }
    for (const auto &k : kHooks)
        if (!strcmp(name, k.name)) { h.*k.field = value; return AVR_OK; }
    return fail(AVR_ERR_INVALID, "unknown test hook %s", name);
}
#endif

const char *avr_last_error(void) { return g_err; }
const char *avr_version(void) { return "avrecode-ms_amd 0.1 (gfx950)"; }

int avr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const uint8_t *avr_cabac_lps_range_table(void) { return kTables.lps_range; }
const uint8_t *avr_cabac_mlps_state_table(void) { return kTables.mlps_state; }

// ------------------------------------------------------------------ batch API

avr_batch *avr_batch_create(int device, size_t max_slices, size_t max_bins) {
    if (max_slices == 0 || max_slices > 0x7fffffffu) { fail(AVR_ERR_INVALID, "max_slices out of range"); return nullptr; }
    if (select_device(device) != AVR_OK) return nullptr;
    avr_batch *b = new (std::nothrow) avr_batch;
    if (!b) { fail(AVR_ERR_NOMEM, "out of host memory"); return nullptr; }
    b->device = device;
    b->max_slices = max_slices;
    b->max_bins = max_bins;
    const bool ok = hipStreamCreateWithFlags(&b->stream.s, hipStreamNonBlocking) == hipSuccess && b->ev.create() == hipSuccess &&
                    b->h_recs.reserve(max_bins + 16 * max_slices) == AVR_OK;   // records: n + 7 per slice; codes (bytes): n + 31
    if (!ok) {
        if (!g_err[0]) fail(AVR_ERR_HIP, "stream/event creation failed");
        avr_batch_destroy(b);
        return nullptr;
    }
    b->rec_off.reserve(max_slices + 1);
    b->n_bins.reserve(max_slices);
    b->rec_off.push_back(0);
    return b;
}

void avr_batch_destroy(avr_batch *b) { delete b; }

int avr_batch_reset(avr_batch *b) {
    if (int rc = check_idle(b)) return rc;
    b->kind = -1; b->recs8 = false; b->keys = false; b->keys8 = false; b->n_states = 0; b->ran = false; b->total_bins = 0;
    b->group_first.clear(); b->est_in.clear(); b->any_est_in = false; b->est_out_fetched = false;
    b->rec_off.assign(1, 0);
    b->n_bins.clear();
    b->dense_off.clear();
    b->expect_off.clear(); b->expect_len.clear(); b->n_expect = 0; b->expect_used = 0;    // the expectations go with the slices
    return AVR_OK;
}

// avr_batch_begin_group (keys8 false) and avr_batch_begin_group8 (true): the first group of a batch without slices fixes which of
// the two forms of key records the batch holds
static int begin_group(avr_batch *b, const uint8_t *est_in, bool keys8) {
    if (int rc = check_open(b)) return rc;
    if (b->kind >= 0 && !b->keys) return fail(AVR_ERR_INVALID, "a batch holds slices of one kind only: groups belong to key records");
    if ((b->kind >= 0 || !b->group_first.empty()) && b->keys8 != keys8)
        return fail(AVR_ERR_INVALID, keys8 ? "avr_batch_begin_group8 on a batch of two-byte key records: a batch holds slices of one kind only"
                                           : "avr_batch_begin_group on a batch of one-byte key records (avr_batch_begin_group8): a batch holds slices of one kind only");
    if (b->group_first.size() >= b->max_slices) return fail(AVR_ERR_CAPACITY, "batch holds max_slices=%zu groups", b->max_slices);
    const size_t n_keys = keys8 ? AVR_EST_KEYS8 : AVR_EST_KEYS, table_bytes = 2 * n_keys;
    for (size_t k = 0; est_in && k < n_keys; k++) {
        const unsigned pos = est_in[2 * k], neg = est_in[2 * k + 1];
        if (pos < 1 || neg < 1 || pos + neg > 0x60)
            return fail(AVR_ERR_INVALID, "start table entry %zu = {%u, %u}: need pos >= 1, neg >= 1, pos + neg <= 0x60", k, pos, neg);
    }
    const size_t g = b->group_first.size();
    b->keys8 = keys8;
    b->est_in.resize((g + 1) * table_bytes);
    uint8_t *dst = b->est_in.data() + g * table_bytes;
    if (est_in) memcpy(dst, est_in, table_bytes); else memset(dst, 1, table_bytes);    // fresh: {1, 1}
    b->any_est_in |= est_in != nullptr;
    b->group_first.push_back(uint32_t(b->n_bins.size()));
    return int(g);
}
int avr_batch_begin_group(avr_batch *b, const uint8_t *est_in) { return begin_group(b, est_in, false); }
int avr_batch_begin_group8(avr_batch *b, const uint8_t *est_in) { return begin_group(b, est_in, true); }

// Room for one more slice in the pinned staging buffer (padding written); *where = its first element.
static int reserve_slice(avr_batch *b, int kind, size_t n, const uint8_t *init_states, size_t n_states, void **where) {
    if (int rc = check_open(b)) return rc;
    if (kind != AVR_KIND_CABAC && kind != AVR_KIND_RANGE && kind != AVR_KIND_CABAC_CODES && kind != AVR_KIND_CABAC8 &&
        kind != AVR_KIND_RANGE_KEYS && kind != AVR_KIND_RANGE_KEYS8)
        return fail(AVR_ERR_INVALID, "unknown kind %d", kind);
    // key records are K2 records before their estimators are resolved: the batch is an AVR_KIND_RANGE batch whose records the device makes
    const bool keys8 = kind == AVR_KIND_RANGE_KEYS8;
    const bool keys = kind == AVR_KIND_RANGE_KEYS || keys8;
    if (keys) kind = AVR_KIND_RANGE;
    // one-byte records are K1 records in another width: the batch is an AVR_KIND_CABAC batch whose staging buffer holds bytes
    const bool recs8 = kind == AVR_KIND_CABAC8;
    if (recs8) {
        if (int rc = check_states8(n_states)) return rc;
        kind = AVR_KIND_CABAC;
    }
    if ((b->kind >= 0 && (b->kind != kind || b->recs8 != recs8 || b->keys != keys)) || (!keys && !b->group_first.empty()) ||
        ((b->kind >= 0 || !b->group_first.empty()) && b->keys8 != keys8))    // (a group begun says which form of key records)
        return fail(AVR_ERR_INVALID, "a batch holds slices of one kind only");
    if (n > 0xfffffff0u) return fail(AVR_ERR_INVALID, "slice too long");
    if (b->n_bins.size() >= b->max_slices) return fail(AVR_ERR_CAPACITY, "batch holds max_slices=%zu slices", b->max_slices);
    if (b->total_bins + n > b->max_bins) return fail(AVR_ERR_CAPACITY, "batch holds max_bins=%zu records", b->max_bins);
    const size_t idx = b->n_bins.size();
    if (keys && b->group_first.empty()) {                        // no group begun: a fresh one
        if (int rc = begin_group(b, nullptr, keys8); rc < 0) return rc;
    }
    if (kind == AVR_KIND_CABAC) {
        if (n_states > AVR_MAX_STATES) return fail(AVR_ERR_INVALID, "n_states %zu > %d", n_states, AVR_MAX_STATES);
        if (!init_states && n_states) return fail(AVR_ERR_INVALID, "null init_states");
        if (idx && n_states != b->n_states) return fail(AVR_ERR_INVALID, "all slices of a batch use the same n_states");
        for (size_t i = 0; i < n_states; i++)
            if (init_states[i] > 127) return fail(AVR_ERR_INVALID, "state byte %zu = %u is not 2*pStateIdx+valMPS", i, init_states[i]);
        if (int rc = b->h_states.reserve(b->max_slices * std::max<size_t>(n_states, 1))) return rc;
        b->n_states = n_states;
        if (n_states) memcpy(b->h_states.p + idx * n_states, init_states, n_states);
    }
    const uint64_t off = b->rec_off.back();
    if (kind == AVR_KIND_CABAC_CODES) {
        // Resolved codes live in the same pinned buffer as records would, as bytes: slice i at byte code_off[i] (the
        // res_off of the chunk plan: 16-byte aligned, padded with a group of its own)
        const uint64_t padded = avr::slice_work_bytes(n);
        if (off + padded > (b->max_bins + 16 * b->max_slices) * sizeof(uint16_t))
            return fail(AVR_ERR_CAPACITY, "batch code buffer full (%zu slices)", b->n_bins.size());
        uint8_t *dst = reinterpret_cast<uint8_t *>(b->h_recs.p) + off;
        memset(dst + n, AVR_CODE_BYPASS(0), padded - n);         // the padding value of a resolved stream (bypass 0, never coded)
        b->rec_off.push_back(off + padded);
        *where = dst;
    } else if (recs8 || keys8) {
        // one byte per record in the same pinned buffer, slice i at BYTE rec_off[i], a multiple of 16 (the one-byte kernels read
        // 16-byte groups); what lies between a slice's last record and the next multiple of 16 is told apart by its index there
        const uint64_t padded = (uint64_t(n) + 15) & ~uint64_t(15);
        uint8_t *dst = reinterpret_cast<uint8_t *>(b->h_recs.p) + off;
        memset(dst + n, 0, padded - n);
        b->rec_off.push_back(off + padded);
        *where = dst;
    } else {
        const uint64_t padded = (uint64_t(n) + 7) & ~uint64_t(7);
        for (uint64_t i = n; i < padded; i++) b->h_recs.p[off + i] = kind == AVR_KIND_CABAC ? AVR_NOP_CABAC : AVR_NOP_RANGE;
        b->rec_off.push_back(off + padded);
        *where = b->h_recs.p + off;
    }
    b->total_bins += n;
    b->n_bins.push_back(uint32_t(n));
    b->kind = kind;
    b->recs8 = recs8;
    b->keys = keys;
    b->keys8 = keys8;
    return int(idx);
}

int avr_batch_reserve_slice(avr_batch *b, int kind, size_t n, const uint8_t *init_states, size_t n_states, void **buffer) {
    if (!buffer) return fail(AVR_ERR_INVALID, "null buffer pointer");
    return reserve_slice(b, kind, n, init_states, n_states, buffer);
}

// one slice copied in: `elem` bytes a record (code) of `src`
static int add_slice(avr_batch *b, int kind, const void *src, size_t n, size_t elem, const uint8_t *init_states, size_t n_states) {
    if (!src && n) return fail(AVR_ERR_INVALID, kind == AVR_KIND_CABAC_CODES ? "null codes" : "null records");
    void *dst = nullptr;
    const int idx = reserve_slice(b, kind, n, init_states, n_states, &dst);
    if (idx >= 0 && n) memcpy(dst, src, n * elem);
    return idx;
}

int avr_batch_add_slice_cabac(avr_batch *b, const uint16_t *recs, size_t n, const uint8_t *init_states, size_t n_states) {
    return add_slice(b, AVR_KIND_CABAC, recs, n, 2, init_states, n_states);
}
int avr_batch_add_slice_range(avr_batch *b, const uint16_t *recs, size_t n) { return add_slice(b, AVR_KIND_RANGE, recs, n, 2, nullptr, 0); }
int avr_batch_add_slice_range_keys(avr_batch *b, const uint16_t *recs, size_t n) { return add_slice(b, AVR_KIND_RANGE_KEYS, recs, n, 2, nullptr, 0); }
int avr_batch_add_slice_range_keys8(avr_batch *b, const uint8_t *recs8, size_t n) { return add_slice(b, AVR_KIND_RANGE_KEYS8, recs8, n, 1, nullptr, 0); }
int avr_batch_add_slice_cabac8(avr_batch *b, const uint8_t *recs8, size_t n, const uint8_t *init_states, size_t n_states) {
    return add_slice(b, AVR_KIND_CABAC8, recs8, n, 1, init_states, n_states);
}
int avr_batch_add_slice_codes(avr_batch *b, const uint8_t *codes, size_t n) { return add_slice(b, AVR_KIND_CABAC_CODES, codes, n, 1, nullptr, 0); }

#define AVR_STAGE(dst, src, n) do { if (int rc_ = stage_h2d(b, dst, src, n)) return rc_; } while (0)

// The restore check's expectations.  staged_restore: what their offsets and lengths take of the arena; reserve_restore: decides whether
// the run has the check (iff a slice has an expectation) and makes room; stage_restore: the expectations with their offsets and
// lengths on their way to the device, among the run's other H2D copies.
static size_t staged_restore(const avr_batch *b, size_t n) { return b->n_expect ? staged<uint64_t>(n) + staged<uint32_t>(n) : 0; }

static int reserve_restore(avr_batch *b, size_t n) {
    int rc = b->restorer.arm(b->n_expect > 0, n);
    if (rc || !b->restorer.on) return rc;
    b->expect_off.resize(n, 0);
    b->expect_len.resize(n, AVR_EXPECT_NONE);
    if ((rc = b->d_expect.reserve(b->expect_used + 8)) || (rc = b->d_expect_off.reserve(n)) || (rc = b->d_expect_len.reserve(n))) return rc;
    return AVR_OK;
}

static int stage_restore(avr_batch *b, size_t n) {
    if (!b->restorer.on) return AVR_OK;
    if (b->expect_used) AVR_HIP(hipMemcpyAsync(b->d_expect.p, b->h_expect.p, b->expect_used, hipMemcpyHostToDevice, b->stream));
    AVR_STAGE(b->d_expect_off.p, b->expect_off.data(), n);
    AVR_STAGE(b->d_expect_len.p, b->expect_len.data(), n);
    return AVR_OK;
}

// What every run begins with: room for what every path has (`arena`: what the path stages of its own), which checks the run has
// and room for their answers, the arena empty.
static int begin_run(avr_batch *b, size_t n, size_t arena) {
    int rc;
    if ((rc = b->d_out_off.reserve(n + 1)) || (rc = b->d_dense_off.reserve(n + 1)) || (rc = b->d_n_bins.reserve(n)) ||
        (rc = b->d_order.reserve(n)) || (rc = b->d_out_len.reserve(n)) || (rc = b->d_status.reserve(n)) ||
        (rc = b->d_out.reserve(b->hp.out_off.back())) || (rc = b->h_out_len.reserve(n)) || (rc = b->h_status.reserve(n)) ||
        (rc = b->h_plan.reserve(arena + staged_plan(b->hp) + staged_restore(b, n))))
        return rc;
    const bool verify = b->kind == AVR_KIND_RANGE ? b->verify : b->verify_k1;
    if ((rc = b->verifier.arm(verify, n)) || (rc = b->est_checker.arm(verify && b->keys, n)) || (rc = reserve_restore(b, n))) return rc;
    b->plan_used = 0;
    b->output = {b->d_out.p, b->d_out_off.p, b->d_out_len.p, b->d_status.p};
    return AVR_OK;
}

// lengths, statuses, final states and the checks' answers on their way to the host behind the kernels
static int enqueue_lengths(avr_batch *b, uint32_t n32) {
    const size_t n = n32, ns = b->n_states;
    const bool with_states = b->kind == AVR_KIND_CABAC && ns;
    hipStream_t s = b->stream;
    AVR_HIP(hipEventRecord(b->ev[3], s));
    AVR_HIP(hipMemcpyAsync(b->h_out_len.p, b->output.out_len, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    AVR_HIP(hipMemcpyAsync(b->h_status.p, b->output.status, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (with_states) AVR_HIP(hipMemcpyAsync(b->h_final.p, b->d_final.p, n * ns, hipMemcpyDeviceToHost, s));
    for (Check *c : b->checks())
        if (int rc = c->fetch(s, n)) return rc;
    return AVR_OK;
}

// What follows the encode kernels of every path, in this order: the verifier of the batch's kind, the estimator checker, the restore
// check -- each that the run has, between its two events -- and the lengths.
// The verifier reads what that path's encoder read (b->read).  K2: the range decoder over tiles or slice-major records.  K1: the
// CABAC decoder over whatever form the records or codes have, with the encoder's final states where the kind has states (b->states).
// The estimator checker holds the resolver's records to the key records and the tables, in the resolver's workspace (it is done with
// it, and the checker's is no larger).
// again: behind K1p's second pass at avr_batch_wait, over the same bytes.  The test build's hooks (verify_flip, restore_flip: a byte
// of a slice's output complemented in front of a check's start event) have had their turn then.
static int enqueue_checks(avr_batch *b, uint32_t n32, bool again = false) {
    hipStream_t s = b->stream;
    int rc;
    if (b->verifier.on) {
#ifdef AVR_TEST_HOOKS
        if (const uint32_t k = avr::test_hooks().verify_flip; k && k <= n32 && !again) AVR_HIP(avr::launch_verify_flip(s, b->output, k - 1));
#endif
        if ((rc = b->verifier.start(s))) return rc;
        if (b->kind == AVR_KIND_RANGE) AVR_HIP(avr::launch_range_verify(s, b->read, b->output, b->verifier.d_first.p));
        else AVR_HIP(avr::launch_cabac_verify(s, b->read, b->states, b->output, b->verifier.d_first.p));
        if ((rc = b->verifier.end(s))) return rc;
    }
    if (b->est_checker.on) {
        if ((rc = b->est_checker.start(s))) return rc;
        AVR_HIP(avr::launch_est_verify(s, b->key_records(), b->d_recs.p, b->d_group_first.p, uint32_t(b->group_first.size()),
                                       b->any_est_in ? b->d_est_in.p : nullptr, b->d_est_out.p, &b->plan, avr::align256(b->d_est_ws.p),
                                       b->output.status, b->est_checker.d_first.p));
        if ((rc = b->est_checker.end(s))) return rc;
    }
    if (b->restorer.on) {                                        // (K1 only: a K2 batch takes no expectations)
#ifdef AVR_TEST_HOOKS
        if (const uint32_t k = avr::test_hooks().restore_flip; k && k <= n32 && !again) AVR_HIP(avr::launch_verify_flip(s, b->output, k - 1));
#endif
        if ((rc = b->restorer.start(s))) return rc;
        AVR_HIP(avr::launch_restore_check(s, b->output, n32, b->d_expect.p, b->d_expect_off.p, b->d_expect_len.p, b->restorer.d_first.p));
        if ((rc = b->restorer.end(s))) return rc;
    }
    return enqueue_lengths(b, n32);
}

// A batch of resolved codes: H2D of one byte per bin, K1p phases B-D (or the one-lane-per-slice coder), lengths back.
static int submit_codes(avr_batch *b, uint32_t n32) {
    const size_t n = n32;
    avr::fill_plan(b->hp, b->n_bins.data(), n, avr::PlanFor::Codes);
    const bool chunked = pick_chunked(b);                        // (same rule as for records)
    std::vector<uint32_t> order;
    if (!chunked) {
        std::vector<uint64_t> tile_off;
        avr::plan_tiles(b->n_bins, order, tile_off);             // longest first: the lanes of a wave finish together
    }
    const uint64_t total_codes = b->rec_off.back();
    int rc;
    if ((rc = b->d_recs.reserve((total_codes + 64) / 2 + 1)) || (rc = b->d_res_off.reserve(n + 1)) ||
        (rc = begin_run(b, n, staged<uint64_t>(n + 1) * 2 + staged<uint32_t>(n) * 2)))                   // rec_off, out_off, n_bins, order
        return rc;
    hipStream_t s = b->stream;
    b->hint_used = 0;
    AVR_HIP(hipEventRecord(b->ev[0], s));
    AVR_HIP(hipMemcpyAsync(b->d_recs.p, b->h_recs.p, total_codes, hipMemcpyHostToDevice, s));
    AVR_STAGE(b->d_res_off.p, b->rec_off.data(), n + 1);
    avr_chunk_plan plan;                                         // the codes lie as the caller's records would: res_off is rec_off
    if ((rc = stage_plan(b, total_codes, &plan)) || (rc = b->d_workspace.reserve(avr::code_layout(n, &plan).total + 256))) return rc;
    AVR_STAGE(b->d_out_off.p, b->hp.out_off.data(), n + 1);
    AVR_STAGE(b->d_n_bins.p, b->n_bins.data(), n);
    if (!chunked) AVR_STAGE(b->d_order.p, order.data(), n);
    if ((rc = stage_restore(b, n))) return rc;
    AVR_HIP(hipMemsetAsync(b->d_status.p, 0, n * sizeof(int32_t), s));
    AVR_HIP(hipEventRecord(b->ev[1], s));
    AVR_HIP(hipEventRecord(b->ev[2], s));
    b->read = {b->d_recs.p, b->d_res_off.p, b->d_n_bins.p, chunked ? nullptr : b->d_order.p, n32, false, avr::cabac_verify::kCodes};
    b->states = {};                                              // codes carry their states
    if (chunked) AVR_HIP(avr::launch_k1p_code(s, b->read, &plan, avr::align256(b->d_workspace.p), b->output));
    else AVR_HIP(avr::launch_cabac_encode_codes(s, b->read, b->output));
    b->last_path = chunked;
    return enqueue_checks(b, n32);
}

// A batch of key records: the estimators of every group resolved on the device, d_keys -> d_recs (K2 range records with their
// padding), the groups' tables after the run left in d_est_out.  Enqueues and returns.
static int resolve_keys(avr_batch *b, uint32_t n32) {
    const size_t n = n32, n_groups = b->group_first.size(), table_bytes = b->est_table();
    std::vector<uint32_t> group_first(b->group_first);
    group_first.push_back(n32);
    int rc;
    if ((rc = b->d_group_first.reserve(n_groups + 1)) || (rc = b->d_est_ws.reserve(avr::est_layout(n, n_groups, b->plan.total_chunks, b->est_pad()).total + 256)) ||
        (rc = b->d_est_out.reserve(n_groups * table_bytes)) || (b->any_est_in && (rc = b->d_est_in.reserve(n_groups * table_bytes))))
        return rc;
    hipStream_t s = b->stream;
    AVR_STAGE(b->d_group_first.p, group_first.data(), n_groups + 1);
    if (b->any_est_in) {                                         // through pinned memory: the copy must not read pageable memory after the call
        if ((rc = b->h_est_in.reserve(n_groups * table_bytes))) return rc;
        memcpy(b->h_est_in.p, b->est_in.data(), n_groups * table_bytes);
        AVR_HIP(hipMemcpyAsync(b->d_est_in.p, b->h_est_in.p, n_groups * table_bytes, hipMemcpyHostToDevice, s));
    }
    b->est_out_fetched = false;
    AVR_HIP(avr::launch_est_resolve(s, b->key_records(), b->d_group_first.p, uint32_t(n_groups), b->any_est_in ? b->d_est_in.p : nullptr,
                                    b->d_est_out.p, &b->plan, avr::align256(b->d_est_ws.p), b->d_recs.p, b->output.status));
#ifdef AVR_TEST_HOOKS
    if (const uint32_t k = avr::test_hooks().est_flip; k && k <= n32 && b->verifier.on)
        AVR_HIP(avr::launch_est_flip(s, b->d_recs.p, b->d_rec_off.p, b->d_n_bins.p, k - 1, avr::test_hooks().est_flip_bin));
#endif
    return AVR_OK;
}

// Everything of a run up to the lengths on their way back.  `use_hint`: size the kernels by the context count of this
// object's previous run instead of asking the device and waiting (avr::DenseHint); avr_batch_wait checks the guess.
static int submit_impl(avr_batch *b, bool use_hint) {
    const size_t n = b->n_bins.size();
    const uint32_t n32 = uint32_t(n);
    if (b->kind == AVR_KIND_CABAC_CODES) return submit_codes(b, n32);
    const size_t ns = b->n_states;
    const bool cabac = b->kind == AVR_KIND_CABAC;
    const bool chunked = pick_chunked(b);
    b->last_path = chunked;
    std::vector<uint32_t> order;
    std::vector<uint64_t> tile_off(1, 0);
    if (!chunked) avr::plan_tiles(b->n_bins, order, tile_off, b->recs8 ? 16 : 8);     // one-byte records: one-byte tiles (the chunked path has no tiles)
    // the chunk arrays once, whichever of the resolver and K2p reads them
    avr::fill_plan(b->hp, b->n_bins.data(), n,
                   chunked && cabac ? avr::PlanFor::K1p : chunked || b->keys ? avr::PlanFor::Chunks : avr::PlanFor::Serial);
    const uint64_t total_recs = b->rec_off.back(), total_chunks = tile_off.back(), total_out = b->hp.out_off.back();
    const size_t n_tiles = tile_off.size() - 1;

    int rc;
    if ((b->recs8 ? (rc = b->d_recs8.reserve(total_recs + 16)) : (rc = b->d_recs.reserve(total_recs))) ||
        (!chunked && ((rc = b->d_tiles.reserve(total_chunks)) || (rc = b->d_tile_off.reserve(n_tiles + 1)))) ||
        (rc = b->d_rec_off.reserve(n + 1)) || (rc = b->h_ndense.reserve(16)) || (b->keys && (rc = b->d_keys.reserve(b->keys8 ? total_recs / 2 + 16 : total_recs))))      // (elements of two bytes)
        return rc;
    if (cabac && ((rc = b->d_states.reserve(n * std::max<size_t>(ns, 1))) || (rc = b->d_final.reserve(n * std::max<size_t>(ns, 1))) ||
                  (rc = b->h_final.reserve(n * std::max<size_t>(ns, 1)))))
        return rc;
    // rec_off, out_off, n_bins; tile_off, order; group_first
    if ((rc = begin_run(b, n, staged<uint64_t>(n + 1) * 2 + staged<uint32_t>(n) + (chunked ? 0 : staged<uint64_t>(n_tiles + 1) + staged<uint32_t>(n)) +
                                  (b->keys ? staged<uint32_t>(b->group_first.size() + 1) : 0)))) return rc;

    hipStream_t s = b->stream;
    const avr::DenseHint hint{use_hint ? std::min<uint32_t>(b->dense_hint, uint32_t(ns)) : 0u, b->h_ndense.p, b->h_ndense.p + 1};
    b->hint_used = hint.rows;
    b->h_ndense.p[0] = b->h_ndense.p[1] = 0;
    if (b->recs8) {                                              // neither one-byte path needs a guess: the contexts are the slices' n_states
        b->hint_used = 0;
        b->h_ndense.p[0] = uint32_t(ns);
    }
    AVR_HIP(hipEventRecord(b->ev[0], s));
    if (b->recs8) AVR_HIP(hipMemcpyAsync(b->d_recs8.p, b->h_recs.p, total_recs, hipMemcpyHostToDevice, s));        // one byte a record
    else if (b->keys8) AVR_HIP(hipMemcpyAsync(b->d_keys.p, b->h_recs.p, total_recs, hipMemcpyHostToDevice, s));    // one byte a key record
    else AVR_HIP(hipMemcpyAsync(b->keys ? b->d_keys.p : b->d_recs.p, b->h_recs.p, total_recs * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    AVR_STAGE(b->d_rec_off.p, b->rec_off.data(), n + 1);
    AVR_STAGE(b->d_out_off.p, b->hp.out_off.data(), n + 1);
    AVR_STAGE(b->d_n_bins.p, b->n_bins.data(), n);
    if (!chunked) {
        AVR_STAGE(b->d_tile_off.p, tile_off.data(), n_tiles + 1);
        AVR_STAGE(b->d_order.p, order.data(), n);
    }
    if (cabac && ns) AVR_HIP(hipMemcpyAsync(b->d_states.p, b->h_states.p, n * ns, hipMemcpyHostToDevice, s));
    if ((rc = stage_restore(b, n))) return rc;
    AVR_HIP(hipEventRecord(b->ev[1], s));
    AVR_HIP(hipMemsetAsync(b->d_status.p, 0, n * sizeof(int32_t), s));
    // Both K1 paths renumber a two-byte batch onto the contexts it uses themselves (the intra-slice parallel kernels inside
    // their census pass, the one-lane-per-slice kernel through launch_cabac_encode): records and states go in as they are.
    // One-byte records name dense ids below n_states already: neither one-byte path counts or renumbers.
    if ((rc = stage_plan(b, avr::plan_total(b->hp.res_off), &b->plan))) return rc;
    const avr_chunk_plan *plan = &b->plan;
    if (chunked && (rc = b->d_workspace.reserve((cabac ? avr::k1p_layout(n, uint32_t(ns), plan).total
                                                       : avr::k2p_layout(n, plan->total_chunks, total_out).total) + 256))) return rc;
    if (b->keys && (rc = resolve_keys(b, n32))) return rc;       // key records: d_keys -> d_recs, inside slot [1] of the timings
    uint8_t *wsp = avr::align256(b->d_workspace.p);
    b->states = cabac ? avr::States{b->d_states.p, uint32_t(ns), b->d_final.p} : avr::States{};
    // the slice-major records as they lie on the device (the tiled paths: with the order their slices take in the tiles) ...
    const avr::Slices recs{b->recs8 ? static_cast<const void *>(b->d_recs8.p) : b->d_recs.p, b->d_rec_off.p, b->d_n_bins.p, chunked ? nullptr : b->d_order.p,
                           n32, false, b->recs8 ? avr::cabac_verify::kSlices8 : avr::cabac_verify::kSlices2};
    if (chunked) {
        // ... are what K2p and K1p read, K1p in the caller's numbering: the census, the dense map and the chains are checked with the bytes
        b->read = recs;
        AVR_HIP(hipEventRecord(b->ev[2], s));
        if (!cabac)                                              // K2 for few, long slices: the range recurrence per slice, everything else per chunk (avr_k2p.hip)
            AVR_HIP(avr::launch_k2p(s, recs, plan, total_out, wsp, b->output));
        else if (b->recs8)                                       // one-byte records: no census, no guess to check, nothing waits
            AVR_HIP(avr::launch_k1p8(s, recs, b->states, plan, wsp, b->output));
        else
            AVR_HIP(avr::launch_k1p(s, recs, b->states, plan, wsp, b->output, &hint));
    } else {
        // ... or go into the tiles the one-lane-per-slice coders read (one-byte records validated and transposed in one pass, as they are)
        b->read = {b->d_tiles.p, b->d_tile_off.p, b->d_n_bins.p, b->d_order.p, n32, true, b->recs8 ? avr::cabac_verify::kTiles8 : avr::cabac_verify::kTiles2};
        if (b->recs8) AVR_HIP(avr::launch_pack_tiles8_narrow(s, uint32_t(ns), recs, b->d_tile_off.p, b->d_tiles.p, b->output.status));
        else AVR_HIP(avr::launch_pack_tiles(s, b->kind, uint32_t(ns), recs, b->d_tile_off.p, b->d_tiles.p, b->output.status));
        AVR_HIP(hipEventRecord(b->ev[2], s));
        if (b->recs8) AVR_HIP(avr::launch_cabac8_encode(s, b->read, b->states, b->output));      // no census, no guess, nothing waits
        else if (cabac) AVR_HIP(avr::launch_cabac_encode(s, b->read, b->states, b->output, &hint));
        else AVR_HIP(avr::launch_range_encode(s, b->read, b->output));
    }
    return enqueue_checks(b, n32);
}

int avr_batch_submit(avr_batch *b) {
    if (int rc = check_idle(b)) return rc;
    if (int rc = select_device(b->device)) return rc;
    b->ran = false;                                              // a batch may be submitted again after avr_batch_wait: same slices, coded anew
    const size_t n = b->n_bins.size();
    b->dense_off.assign(n + 1, 0);
    if (b->verify && b->kind >= 0 && b->kind != AVR_KIND_RANGE)
        return fail(AVR_ERR_INVALID, "verification exists for the compress direction only: not for a K1 batch");
    if (b->verify_k1 && b->kind == AVR_KIND_RANGE)
        return fail(AVR_ERR_INVALID, "K1 verification exists for the decompress direction only: not for a K2 batch");
    for (Check *c : b->checks()) (void)c->arm(false, 0);
    if (n == 0) { b->in_flight = true; return AVR_OK; }
    const bool use_hint = b->dense_hint > 0 && !avr::no_hint();
    if (int rc = submit_impl(b, use_hint)) { (void)hipStreamSynchronize(b->stream); return rc; }
    b->in_flight = true;
    return AVR_OK;
}

// Wait for the kernels, then: the coded bytes gathered densely on the device, one D2H copy.
int avr_batch_wait(avr_batch *b) {
    if (!b) return fail(AVR_ERR_INVALID, "null batch");
    if (!b->in_flight) return b->ran ? AVR_OK : fail(AVR_ERR_INVALID, "batch has not been submitted");
    if (int rc = select_device(b->device)) return rc;
    b->in_flight = false;
    const size_t n = b->n_bins.size();
    if (n == 0) {                                                // nothing ran: the run's info and times are zeros, not the previous run's
        memset(b->info, 0, sizeof b->info);
        memset(b->ms, 0, sizeof b->ms);
        for (Check *c : b->checks()) c->ms = c->before = 0;     // (avr_batch_submit has set every check off)
        b->last_path = 0;
        b->ran = true;
        return AVR_OK;
    }
    const uint32_t n32 = uint32_t(n);
    hipStream_t s = b->stream;
    int rc;
    AVR_HIP(hipStreamSynchronize(s));
    b->info[0] = uint32_t(b->last_path); b->info[1] = b->info[2] = b->info[3] = 0;
    if (b->kind == AVR_KIND_CABAC) {
        // The run was sized by a guess of the context count.  The one-lane-per-slice kernel is exact whatever the
        // guess; the intra-slice parallel kernels only if the batch needs no more rows than guessed: else once more,
        // asking the device this time.
        b->info[1] = b->hint_used; b->info[3] = 0;
        if (b->hint_used && b->last_path == 1 && b->h_ndense.p[0] > b->hint_used) {
            if ((rc = submit_impl(b, false))) { (void)hipStreamSynchronize(s); return rc; }
            AVR_HIP(hipStreamSynchronize(s));
            b->info[3] = 1;
        }
        if (b->last_path == 1 && b->h_ndense.p[1]) {             // slices with a context the sampled census missed: their second pass
            if (b->verifier.on || b->restorer.on) {
                // The verifier has run in front of this pass, and the pass treats a slice it marked AVR_SLICE_VERIFY_FAILED like one with a bad
                // record (length 0).  Such a slice goes in as AVR_SLICE_OK -- finished, so the pass leaves it alone -- and the verifier behind
                // the pass, which decodes every slice again, fails it again at the same bin.  (h_status is the device's, behind a synchronise.)
                // The same holds for the restore check and its findings.
                for (Check *c : b->checks()) c->carry();
                bool any = false;
                for (size_t i = 0; i < n; i++)
                    if (b->h_status.p[i] == AVR_SLICE_VERIFY_FAILED) { b->h_status.p[i] = AVR_SLICE_OK; any = true; }
                if (any) AVR_HIP(hipMemcpyAsync(b->d_status.p, b->h_status.p, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
            }
            AVR_HIP(avr::launch_k1p_retry(s, b->read, b->states, &b->plan, avr::align256(b->d_workspace.p), b->output));
            // the verifier and the restore check skipped the slices of this pass (their status was not AVR_SLICE_OK yet): once more behind it
            if ((rc = enqueue_checks(b, n32, true))) return rc;
            AVR_HIP(hipStreamSynchronize(s));
            b->info[3] |= 2;
        }
        b->info[2] = b->h_ndense.p[0];
        const uint32_t seen = b->h_ndense.p[0];
        if (seen) b->dense_hint = std::min<uint32_t>(uint32_t(b->n_states), seen + 8);   // a little room: the next batch of a stream rarely needs more
    }
    for (size_t i = 0; i < n; i++) {
        const uint64_t cap = b->hp.out_off[i + 1] - b->hp.out_off[i];
        b->dense_off[i + 1] = b->dense_off[i] + std::min<uint64_t>(b->h_out_len.p[i], cap);
    }
    const uint64_t dense_total = b->dense_off.back();
    if ((rc = b->d_dense.reserve(dense_total + 1)) || (rc = b->h_out.reserve(dense_total + 1))) return rc;
    b->plan_used = 0;                                            // the run's plan arrays are consumed: the arena is free again
    AVR_STAGE(b->d_dense_off.p, b->dense_off.data(), n + 1);
    AVR_HIP(avr::launch_compact(s, b->output, b->d_dense_off.p, n32, b->d_dense.p, dense_total));
    if (dense_total) AVR_HIP(hipMemcpyAsync(b->h_out.p, b->d_dense.p, dense_total, hipMemcpyDeviceToHost, s));
    AVR_HIP(hipEventRecord(b->ev[4], s));
    AVR_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&b->ms[i], b->ev[i], b->ev[i + 1]);
    // The encode's slot ends where the first check the run has starts, as last recorded.  Behind K1p's second pass (rare) that is the
    // check's second recording: the span from ev[2] then also holds the checks' first runs, taken off here, and what lay between the
    // two -- the host's wait, the status and length copies -- which stays in: on that path ms[2] is an upper bound of the encode, not
    // the encode alone.
    bool first = true;
    for (Check *c : b->checks()) {
        c->finish();
        if (!c->on) continue;
        if (first) (void)hipEventElapsedTime(&b->ms[2], b->ev[2], c->ev[0]);
        first = false;
        b->ms[2] -= c->before;
    }
    b->ran = true;                                               // only now: the getters hand out h_out / h_status
    return AVR_OK;
}

int avr_batch_run(avr_batch *b) {
    if (!b) return fail(AVR_ERR_INVALID, "null batch");
    if (b->ran) return fail(AVR_ERR_INVALID, "batch already ran");
    if (int rc = avr_batch_submit(b)) return rc;
    return avr_batch_wait(b);
}

int avr_batch_get(avr_batch *b, size_t slice, const uint8_t **bytes, size_t *len, int *status) {
    if (int rc = check_slice(b, slice)) return rc;
    if (bytes) *bytes = b->h_out.p + b->dense_off[slice];
    if (len) *len = size_t(b->dense_off[slice + 1] - b->dense_off[slice]);
    if (status) *status = b->h_status.p[slice];
    return AVR_OK;
}

int avr_batch_get_states(avr_batch *b, size_t slice, const uint8_t **states, size_t *n_states) {
    if (int rc = check_ran(b)) return rc;
    if (b->kind != AVR_KIND_CABAC) return fail(AVR_ERR_INVALID, "not a CABAC batch");
    if (int rc = check_slice(b, slice)) return rc;
    if (states) *states = b->h_final.p + slice * b->n_states;
    if (n_states) *n_states = b->n_states;
    return AVR_OK;
}

int avr_batch_get_estimators(avr_batch *b, size_t group, const uint8_t **pos_neg, size_t *n_keys) {
    if (int rc = check_ran(b)) return rc;
    if (!b->keys) return fail(AVR_ERR_INVALID, "not a batch of key records");
    if (group >= b->group_first.size()) return fail(AVR_ERR_INVALID, "group %zu out of range", group);
    if (!b->est_out_fetched) {                                   // on first use: most callers want the table of a file's last batch only
        if (int rc = select_device(b->device)) return rc;
        const size_t bytes = b->group_first.size() * b->est_table();
        if (int rc = b->h_est_out.reserve(bytes)) return rc;
        AVR_HIP(hipMemcpyAsync(b->h_est_out.p, b->d_est_out.p, bytes, hipMemcpyDeviceToHost, b->stream));
        AVR_HIP(hipStreamSynchronize(b->stream));
        b->est_out_fetched = true;
    }
    if (pos_neg) *pos_neg = b->h_est_out.p + group * b->est_table();
    if (n_keys) *n_keys = b->est_keys();
    return AVR_OK;
}

int avr_batch_run_info(avr_batch *b, uint32_t info[4]) {
    if (int rc = check_ran(b, info != nullptr)) return rc;
    memcpy(info, b->info, sizeof b->info);
    return AVR_OK;
}

int avr_batch_timings(avr_batch *b, float ms[4]) {
    if (int rc = check_ran(b, ms != nullptr)) return rc;
    memcpy(ms, b->ms, sizeof b->ms);
    return AVR_OK;
}

int avr_batch_set_verify(avr_batch *b, int on) {
    int rc = check_idle(b);
    if (rc || (on && ((rc = b->verifier.make_events(b->device)) || (rc = b->est_checker.make_events(b->device))))) return rc;
    b->verify = on != 0;
    return AVR_OK;
}

int avr_batch_set_verify_k1(avr_batch *b, int on) {
    int rc = check_idle(b);
    if (rc || (on && (rc = b->verifier.make_events(b->device)))) return rc;
    b->verify_k1 = on != 0;
    return AVR_OK;
}

// a check's answer for one slice (AVR_VERIFY_NONE where the run did not have the check), and what the check took
static int check_answer(const avr_batch *b, Check avr_batch::*which, size_t slice, uint32_t *first) {
    if (int rc = check_slice(b, slice)) return rc;
    if (first) *first = (b->*which).answer(slice);
    return AVR_OK;
}
static int check_ms(const avr_batch *b, Check avr_batch::*which, float *ms) {
    if (int rc = check_ran(b, ms != nullptr)) return rc;
    *ms = (b->*which).ms;
    return AVR_OK;
}
int avr_batch_get_verify(avr_batch *b, size_t slice, uint32_t *first_bad) { return check_answer(b, &avr_batch::verifier, slice, first_bad); }
int avr_batch_verify_ms(avr_batch *b, float *ms) { return check_ms(b, &avr_batch::verifier, ms); }
int avr_batch_get_verify_est(avr_batch *b, size_t slice, uint32_t *first_bad) { return check_answer(b, &avr_batch::est_checker, slice, first_bad); }
int avr_batch_verify_est_ms(avr_batch *b, float *ms) { return check_ms(b, &avr_batch::est_checker, ms); }
int avr_batch_get_restore(avr_batch *b, size_t slice, uint32_t *first_diff) { return check_answer(b, &avr_batch::restorer, slice, first_diff); }
int avr_batch_restore_ms(avr_batch *b, float *ms) { return check_ms(b, &avr_batch::restorer, ms); }

int avr_batch_expect(avr_batch *b, size_t slice, const uint8_t *bytes, size_t len) {
    if (int rc = check_open(b)) return rc;
    if (b->kind == AVR_KIND_RANGE) return fail(AVR_ERR_INVALID, "the restore check exists for K1 batches only: not for a K2 batch");
    if (slice >= b->n_bins.size()) return fail(AVR_ERR_INVALID, "slice %zu has not been added", slice);
    if (len >= 0xffffffffull) return fail(AVR_ERR_INVALID, "expectation too long");
    if (!bytes && len) return fail(AVR_ERR_INVALID, "null bytes");
    if (slice < b->expect_len.size() && b->expect_len[slice] != AVR_EXPECT_NONE)
        return fail(AVR_ERR_INVALID, "slice %zu has an expectation already", slice);
    if (int rc = b->restorer.make_events(b->device)) return rc;
    const size_t padded = (len + 7) & ~size_t(7), need = b->expect_used + padded;
    if (need > b->h_expect.cap) {                                // grown with what it holds (reserve keeps nothing)
        PinBuf<uint8_t> grown;
        if (int rc = grown.reserve(std::max(need, 2 * b->h_expect.cap))) return rc;
        if (b->expect_used) memcpy(grown.p, b->h_expect.p, b->expect_used);
        b->h_expect = std::move(grown);
    }
    uint8_t *dst = b->h_expect.p + b->expect_used;
    if (len) memcpy(dst, bytes, len);
    memset(dst + len, 0, padded - len);
    b->expect_off.resize(b->n_bins.size(), 0);
    b->expect_len.resize(b->n_bins.size(), AVR_EXPECT_NONE);
    b->expect_off[slice] = b->expect_used;
    b->expect_len[slice] = uint32_t(len);
    b->expect_used = need;
    b->n_expect++;
    return AVR_OK;
}

// ------------------------------------------------------------------ one batch over several GPUs
// avr_multi lives in avr_multi.cpp, on the public batch calls alone; these are the two things it needs from here (avr_multi.h).
}  // extern "C"
namespace avr {
int multi_set_error(int code, const char *text) { return fail(code, "%s", text); }
int multi_check_device(int device) { return select_device(device); }
}  // namespace avr
extern "C" {

// ------------------------------------------------------------------ device-resident API

// Every entry point below packs its arguments into the launchers' structs (avr_internal.h), runs its checks -- on the caller's size_t
// counts: the structs' are 32 bits wide -- and launches.  Which pointers a call checks is the call's own; the header says so per call.
using avr::Output;
using avr::OutputView;
using avr::Slices;
using avr::States;
using avr::StatesView;
static hipStream_t hip(void *stream) { return static_cast<hipStream_t>(stream); }

static int check_common(const void *a, const void *b, const void *c, size_t n_slices) {
    if (n_slices > 0x7fffffffu) return fail(AVR_ERR_INVALID, "n_slices out of range");
    if (n_slices && (!a || !b || !c)) return fail(AVR_ERR_INVALID, "null device pointer");
    return AVR_OK;
}
static int check_states(size_t n_states) {
    if (n_states > AVR_MAX_STATES) return fail(AVR_ERR_INVALID, "n_states %zu > %d", n_states, AVR_MAX_STATES);
    return AVR_OK;
}

int avr_pack_tiles_device(int device, void *stream, int kind, size_t n_states, const uint16_t *recs, const uint64_t *rec_off,
                          const uint32_t *n_bins, const uint32_t *order, size_t n_slices, const uint64_t *tile_off, void *tiles,
                          int32_t *status) {
    if (int rc = check_common(rec_off, n_bins, tile_off, n_slices)) return rc;
    if (kind != AVR_KIND_CABAC && kind != AVR_KIND_RANGE) return fail(AVR_ERR_INVALID, "kind %d", kind);
    if (int rc = check_states(n_states)) return rc;
    if (n_slices && !status) return fail(AVR_ERR_INVALID, "null status");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_pack_tiles(hip(stream), kind, uint32_t(n_states), Slices{recs, rec_off, n_bins, order, uint32_t(n_slices)}, tile_off, tiles, status));
    return AVR_OK;
}

// one-byte records: what the host can check of the layout -- the base 16-byte aligned, the offsets' array 8-byte aligned (the offsets
// themselves live on the device, where the kernels flag a slice whose offset is not a multiple of 16)
static int check_recs8(const void *recs8, const uint64_t *rec_off, size_t n_states) {
    if (int rc = check_states8(n_states)) return rc;
    if (reinterpret_cast<uintptr_t>(recs8) & 15) return fail(AVR_ERR_INVALID, "recs8 is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(rec_off) & 7) return fail(AVR_ERR_INVALID, "rec_off is not 8-byte aligned");
    return AVR_OK;
}

// the two packers of one-byte records: the narrow one holds its one-byte tiles to their alignment as well
static int pack_tiles8_device(bool narrow, int device, void *stream, size_t n_states, const Slices &in, size_t n_slices, const uint64_t *tile_off,
                              void *tiles, int32_t *status) {
    if (int rc = check_common(in.off, in.n_bins, tile_off, n_slices)) return rc;
    if (int rc = check_recs8(in.recs, in.off, n_states)) return rc;
    if (n_slices && (!in.recs || !tiles || !status)) return fail(AVR_ERR_INVALID, "null device pointer");
    if (narrow && (reinterpret_cast<uintptr_t>(tiles) & 15)) return fail(AVR_ERR_INVALID, "tiles is not 16-byte aligned");
    if (int rc = select_device(device)) return rc;
    AVR_HIP((narrow ? avr::launch_pack_tiles8_narrow : avr::launch_pack_tiles8)(hip(stream), uint32_t(n_states), in, tile_off, tiles, status));
    return AVR_OK;
}
int avr_pack_tiles8_device(int device, void *stream, size_t n_states, const uint8_t *recs8, const uint64_t *rec_off,
                           const uint32_t *n_bins, const uint32_t *order, size_t n_slices, const uint64_t *tile_off, void *tiles,
                           int32_t *status) {
    return pack_tiles8_device(false, device, stream, n_states, Slices{recs8, rec_off, n_bins, order, uint32_t(n_slices)}, n_slices, tile_off, tiles, status);
}
int avr_pack_tiles8_narrow_device(int device, void *stream, size_t n_states, const uint8_t *recs8, const uint64_t *rec_off,
                                  const uint32_t *n_bins, const uint32_t *order, size_t n_slices, const uint64_t *tile_off, void *tiles,
                                  int32_t *status) {
    return pack_tiles8_device(true, device, stream, n_states, Slices{recs8, rec_off, n_bins, order, uint32_t(n_slices)}, n_slices, tile_off, tiles, status);
}

int avr_cabac8_encode_tiles_device(int device, void *stream, const void *tiles, const uint64_t *tile_off, const uint32_t *n_bins,
                                   const uint32_t *order, size_t n_slices, const uint8_t *init_states, size_t n_states,
                                   uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int32_t *status, uint8_t *final_states) {
    if (int rc = check_common(tile_off, n_bins, out_off, n_slices)) return rc;
    if (int rc = check_states8(n_states)) return rc;
    if (n_slices && (!tiles || !out || !out_len || !status || (n_states && !init_states))) return fail(AVR_ERR_INVALID, "null device pointer");
    if (reinterpret_cast<uintptr_t>(tiles) & 15) return fail(AVR_ERR_INVALID, "tiles is not 16-byte aligned");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_cabac8_encode(hip(stream), Slices{tiles, tile_off, n_bins, order, uint32_t(n_slices), true},
                                      States{init_states, uint32_t(n_states), final_states}, Output{out, out_off, out_len, status}));
    return AVR_OK;
}

// the one-lane-per-slice K1 coder over two-byte tiles or slice-major records, sized by the device's count or (counts: the hinted form)
// by the caller's guess
static int cabac_encode_device(int device, void *stream, const Slices &in, size_t n_slices, const States &st, size_t n_states, const Output &o,
                               uint32_t *counts = nullptr, uint32_t rows_hint = 0) {
    if (int rc = check_common(in.off, in.n_bins, o.out_off, n_slices)) return rc;
    if (int rc = check_states(n_states)) return rc;
    if (int rc = select_device(device)) return rc;
    if (!counts) {
        AVR_HIP(avr::launch_cabac_encode(hip(stream), in, st, o));
        return AVR_OK;
    }
    counts[0] = counts[1] = 0;
    const avr::DenseHint hint{std::min<uint32_t>(rows_hint, uint32_t(n_states)), counts, nullptr};
    AVR_HIP(avr::launch_cabac_encode(hip(stream), in, st, o, &hint));
    return AVR_OK;
}
int avr_cabac_encode_tiles_device(int device, void *stream, const void *tiles, const uint64_t *tile_off, const uint32_t *n_bins,
                                  const uint32_t *order, size_t n_slices, const uint8_t *init_states, size_t n_states,
                                  uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int32_t *status, uint8_t *final_states) {
    return cabac_encode_device(device, stream, Slices{tiles, tile_off, n_bins, order, uint32_t(n_slices), true}, n_slices,
                               States{init_states, uint32_t(n_states), final_states}, n_states, Output{out, out_off, out_len, status});
}
int avr_cabac_encode_slices_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                                   const uint32_t *order, size_t n_slices, const uint8_t *init_states, size_t n_states,
                                   uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int32_t *status, uint8_t *final_states) {
    return cabac_encode_device(device, stream, Slices{recs, rec_off, n_bins, order, uint32_t(n_slices)}, n_slices,
                               States{init_states, uint32_t(n_states), final_states}, n_states, Output{out, out_off, out_len, status});
}
int avr_cabac_encode_tiles_device_hinted(int device, void *stream, const void *tiles, const uint64_t *tile_off, const uint32_t *n_bins,
                                         const uint32_t *order, size_t n_slices, const uint8_t *init_states, size_t n_states,
                                         uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int32_t *status, uint8_t *final_states,
                                         uint32_t rows_hint, uint32_t *counts) {
    if (!counts) return fail(AVR_ERR_INVALID, "null counts");
    return cabac_encode_device(device, stream, Slices{tiles, tile_off, n_bins, order, uint32_t(n_slices), true}, n_slices,
                               States{init_states, uint32_t(n_states), final_states}, n_states, Output{out, out_off, out_len, status}, counts, rows_hint);
}

// the K2 coder and its verifier, over tiles or slice-major records
static int range_encode_device(int device, void *stream, const Slices &in, size_t n_slices, const Output &o) {
    if (int rc = check_common(in.off, in.n_bins, o.out_off, n_slices)) return rc;
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_range_encode(hip(stream), in, o));
    return AVR_OK;
}
int avr_range_encode_tiles_device(int device, void *stream, const void *tiles, const uint64_t *tile_off, const uint32_t *n_bins,
                                  const uint32_t *order, size_t n_slices, uint8_t *out, const uint64_t *out_off,
                                  uint32_t *out_len, int32_t *status) {
    return range_encode_device(device, stream, Slices{tiles, tile_off, n_bins, order, uint32_t(n_slices), true}, n_slices, Output{out, out_off, out_len, status});
}
int avr_range_encode_slices_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                                   const uint32_t *order, size_t n_slices, uint8_t *out, const uint64_t *out_off,
                                   uint32_t *out_len, int32_t *status) {
    return range_encode_device(device, stream, Slices{recs, rec_off, n_bins, order, uint32_t(n_slices)}, n_slices, Output{out, out_off, out_len, status});
}

static int range_verify_device(int device, void *stream, const Slices &in, size_t n_slices, const OutputView &o, uint32_t *first_bad, bool need_first_bad) {
    if (int rc = check_common(in.off, in.n_bins, o.out_off, n_slices)) return rc;
    if (n_slices && (!in.recs || !o.out || !o.out_len || !o.status || (need_first_bad && !first_bad))) return fail(AVR_ERR_INVALID, "null device pointer");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_range_verify(hip(stream), in, o, first_bad));
    return AVR_OK;
}
int avr_range_verify_tiles_device(int device, void *stream, const void *tiles, const uint64_t *tile_off, const uint32_t *n_bins,
                                  const uint32_t *order, size_t n_slices, const uint8_t *out, const uint64_t *out_off,
                                  const uint32_t *out_len, int32_t *status, uint32_t *first_bad) {
    return range_verify_device(device, stream, Slices{tiles, tile_off, n_bins, order, uint32_t(n_slices), true}, n_slices,
                               OutputView{out, out_off, out_len, status}, first_bad, false);
}
int avr_range_verify_slices_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                                   const uint32_t *order, size_t n_slices, const uint8_t *out, const uint64_t *out_off,
                                   const uint32_t *out_len, int32_t *status, uint32_t *first_bad) {
    return range_verify_device(device, stream, Slices{recs, rec_off, n_bins, order, uint32_t(n_slices)}, n_slices,
                               OutputView{out, out_off, out_len, status}, first_bad, true);
}

static int check_plan(const avr_chunk_plan *plan, size_t n_slices, bool need_blocks) {
    if (!plan || (n_slices && (!plan->res_off || !plan->chunk_base || !plan->chunk_slice || !plan->dig_off ||
                               (need_blocks && (!plan->blk_base || !plan->blk_slice)))))
        return fail(AVR_ERR_INVALID, "null plan pointer");
    return AVR_OK;
}

// The refusals of the chunked K1 family.  The one-byte form (recs8) has its own limit on n_states, holds its records to their
// alignment, checks more of the caller's pointers and reads no blocks of the plan; the rest is the same.
static int check_chunked(const Slices &in, size_t n_slices, const States &st, size_t n_states, const avr_chunk_plan *plan, void *workspace,
                         size_t workspace_bytes, const Output &o, bool recs8 = false) {
    if (int rc = check_common(in.off, in.n_bins, o.out_off, n_slices)) return rc;
    if (int rc = recs8 ? check_recs8(in.recs, in.off, n_states) : check_states(n_states)) return rc;
    if (recs8 && n_slices && (!in.recs || !o.out || !o.out_len || (n_states && !st.init_states))) return fail(AVR_ERR_INVALID, "null device pointer");
    if (int rc = check_plan(plan, n_slices, !recs8)) return rc;
    if (n_slices && (!workspace || !o.status)) return fail(AVR_ERR_INVALID, "null plan pointer");
    if (workspace_bytes < avr::k1p_layout(n_slices, uint32_t(n_states), plan).total)
        return fail(AVR_ERR_CAPACITY, "workspace of %zu bytes is smaller than %s_chunked_workspace_bytes()", workspace_bytes, recs8 ? "avr_cabac8" : "avr_cabac");
    return AVR_OK;
}

size_t avr_cabac_chunked_workspace_bytes(size_t n_slices, size_t n_states, const avr_chunk_plan *plan) {
    if (!plan || n_states > AVR_MAX_STATES) return 0;
    return avr::k1p_layout(n_slices, uint32_t(n_states), plan).total;
}
size_t avr_cabac8_chunked_workspace_bytes(size_t n_slices, size_t n_states, const avr_chunk_plan *plan) {
    if (!plan || n_states > AVR_MAX_STATES8) return 0;
    return avr::k1p_layout(n_slices, uint32_t(n_states), plan).total;
}

int avr_cabac_encode_chunked_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                                    size_t n_slices, const uint8_t *init_states, size_t n_states, const avr_chunk_plan *plan,
                                    void *workspace, size_t workspace_bytes, uint8_t *out, const uint64_t *out_off,
                                    uint32_t *out_len, int32_t *status, uint8_t *final_states) {
    const Slices in{recs, rec_off, n_bins, nullptr, uint32_t(n_slices)};
    const States st{init_states, uint32_t(n_states), final_states};
    const Output o{out, out_off, out_len, status};
    if (int rc = check_chunked(in, n_slices, st, n_states, plan, workspace, workspace_bytes, o)) return rc;
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_k1p(hip(stream), in, st, plan, workspace, o));
    return AVR_OK;
}

int avr_cabac8_encode_chunked_device(int device, void *stream, const uint8_t *recs8, const uint64_t *rec_off, const uint32_t *n_bins,
                                     size_t n_slices, const uint8_t *init_states, size_t n_states, const avr_chunk_plan *plan,
                                     void *workspace, size_t workspace_bytes, uint8_t *out, const uint64_t *out_off,
                                     uint32_t *out_len, int32_t *status, uint8_t *final_states) {
    const Slices in{recs8, rec_off, n_bins, nullptr, uint32_t(n_slices)};
    const States st{init_states, uint32_t(n_states), final_states};
    const Output o{out, out_off, out_len, status};
    if (int rc = check_chunked(in, n_slices, st, n_states, plan, workspace, workspace_bytes, o, true)) return rc;
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_k1p8(hip(stream), in, st, plan, workspace, o));
    return AVR_OK;
}

int avr_cabac_encode_chunked_device_hinted(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                                           size_t n_slices, const uint8_t *init_states, size_t n_states, const avr_chunk_plan *plan,
                                           void *workspace, size_t workspace_bytes, uint8_t *out, const uint64_t *out_off,
                                           uint32_t *out_len, int32_t *status, uint8_t *final_states, uint32_t rows_hint, uint32_t *counts) {
    const Slices in{recs, rec_off, n_bins, nullptr, uint32_t(n_slices)};
    const States st{init_states, uint32_t(n_states), final_states};
    const Output o{out, out_off, out_len, status};
    if (!counts) return fail(AVR_ERR_INVALID, "null counts");
    if (int rc = check_chunked(in, n_slices, st, n_states, plan, workspace, workspace_bytes, o)) return rc;
    if (int rc = select_device(device)) return rc;
    counts[0] = counts[1] = 0;
    if (n_slices == 0) return AVR_OK;
    const avr::DenseHint hint{std::min<uint32_t>(rows_hint, uint32_t(n_states)), counts, counts + 1};
    AVR_HIP(avr::launch_k1p(hip(stream), in, st, plan, workspace, o, &hint));
    return AVR_OK;
}

int avr_cabac_encode_chunked_second_pass_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                                                size_t n_slices, const uint8_t *init_states, size_t n_states, const avr_chunk_plan *plan,
                                                void *workspace, size_t workspace_bytes, uint8_t *out, const uint64_t *out_off,
                                                uint32_t *out_len, int32_t *status, uint8_t *final_states) {
    const Slices in{recs, rec_off, n_bins, nullptr, uint32_t(n_slices)};
    const States st{init_states, uint32_t(n_states), final_states};
    const Output o{out, out_off, out_len, status};
    if (int rc = check_chunked(in, n_slices, st, n_states, plan, workspace, workspace_bytes, o)) return rc;
    if (int rc = select_device(device)) return rc;
    if (n_slices == 0) return AVR_OK;
    AVR_HIP(avr::launch_k1p_retry(hip(stream), in, st, plan, workspace, o));
    return AVR_OK;
}

extern "C++" {
// The streams the parts of avr_cabac_encode_chunked_device_parts run on, with their events: one set per (device, caller's stream), made on
// first use and kept (work on the caller's stream is ordered, so consecutive calls share it); released by avr::forget_part_streams.
namespace {
struct PartStreams { hipStream_t side[AVR_MAX_PARTS - 1]; hipEvent_t fork, done[AVR_MAX_PARTS - 1]; };
avr::StreamPool<PartStreams> g_parts;
hipError_t part_streams(hipStream_t s, PartStreams **out) {
    return g_parts.get(s, out, [](PartStreams &x) {              // (what was made of one that fails is left to the process's end: an out-of-resources path)
        hipError_t e = hipEventCreateWithFlags(&x.fork, hipEventDisableTiming);
        for (int i = 0; i < AVR_MAX_PARTS - 1 && e == hipSuccess; i++) {
            e = hipStreamCreateWithFlags(&x.side[i], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&x.done[i], hipEventDisableTiming);
        }
        return e;
    });
}
}  // namespace
namespace avr {
void forget_part_streams(hipStream_t s) {
    g_parts.forget(s, [](PartStreams &x) {
        for (int k = 0; k < AVR_MAX_PARTS - 1; k++) {
            (void)hipStreamSynchronize(x.side[k]);
            avr::forget_stream(x.side[k]);                       // the library's own per-stream scratch of that stream
            (void)hipEventDestroy(x.done[k]);
            (void)hipStreamDestroy(x.side[k]);
        }
        (void)hipEventDestroy(x.fork);
    });
}
}  // namespace avr
}  // extern "C++"

// a part's arrays, with what the parts share
static Slices part_slices(const uint16_t *recs, const avr_chunked_part &q) { return {recs, q.rec_off, q.n_bins, nullptr, uint32_t(q.n_slices)}; }
static States part_states(size_t n_states, const avr_chunked_part &q) { return {q.init_states, uint32_t(n_states), q.final_states}; }
static Output part_output(uint8_t *out, const avr_chunked_part &q) { return {out, q.out_off, q.out_len, q.status}; }

int avr_cabac_encode_chunked_device_parts(int device, void *stream, const uint16_t *recs, size_t n_states, uint8_t *out,
                                          const avr_chunked_part *parts, size_t n_parts) {
    if (!parts || n_parts == 0 || n_parts > AVR_MAX_PARTS) return fail(AVR_ERR_INVALID, "1 .. %d parts", AVR_MAX_PARTS);
    for (size_t i = 0; i < n_parts; i++) {
        const avr_chunked_part &q = parts[i];
        if (!q.counts) return fail(AVR_ERR_INVALID, "part %zu: null counts", i);
        if (int rc = check_chunked(part_slices(recs, q), q.n_slices, part_states(n_states, q), n_states, q.plan, q.workspace, q.workspace_bytes,
                                   part_output(out, q)))
            return rc;
    }
    if (int rc = select_device(device)) return rc;
    hipStream_t main = hip(stream);
    PartStreams *ps = nullptr;
    if (n_parts > 1) {
        AVR_HIP(part_streams(main, &ps));
        AVR_HIP(hipEventRecord(ps->fork, main));
    }
    for (size_t i = 0; i < n_parts; i++) {                       // part 0 on the caller's stream, the others beside it
        const avr_chunked_part &q = parts[i];
        hipStream_t s = i == 0 ? main : ps->side[i - 1];
        if (i) AVR_HIP(hipStreamWaitEvent(s, ps->fork, 0));
        q.counts[0] = q.counts[1] = 0;
        if (q.n_slices) {
            const avr::DenseHint hint{std::min<uint32_t>(q.rows_hint, uint32_t(n_states)), q.counts, q.counts + 1, uint32_t(n_parts)};
            AVR_HIP(avr::launch_k1p(s, part_slices(recs, q), part_states(n_states, q), q.plan, q.workspace, part_output(out, q), &hint));
        }
        if (i) AVR_HIP(hipEventRecord(ps->done[i - 1], s));
    }
    for (size_t i = 1; i < n_parts; i++) AVR_HIP(hipStreamWaitEvent(main, ps->done[i - 1], 0));
    return AVR_OK;
}

size_t avr_range_chunked_workspace_bytes(size_t n_slices, const avr_chunk_plan *plan, uint64_t out_total) {
    if (!plan) return 0;
    return avr::k2p_layout(n_slices, plan->total_chunks, out_total).total;
}

int avr_range_encode_chunked_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                                    size_t n_slices, const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                                    uint8_t *out, const uint64_t *out_off, uint64_t out_total, uint32_t *out_len, int32_t *status) {
    if (int rc = check_common(rec_off, n_bins, out_off, n_slices)) return rc;
    if (!plan || (n_slices && (!plan->chunk_base || !plan->chunk_slice || !workspace || !status || !out || !out_len)))
        return fail(AVR_ERR_INVALID, "null plan / workspace / output pointer");
    if (workspace_bytes < avr::k2p_layout(n_slices, plan->total_chunks, out_total).total)
        return fail(AVR_ERR_CAPACITY, "workspace of %zu bytes is smaller than avr_range_chunked_workspace_bytes()", workspace_bytes);
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_k2p(hip(stream), Slices{recs, rec_off, n_bins, nullptr, uint32_t(n_slices)}, plan, out_total, workspace,
                            Output{out, out_off, out_len, status}));
    return AVR_OK;
}

size_t avr_range_resolve_workspace_bytes(size_t n_slices, size_t n_groups, const avr_chunk_plan *plan) {
    if (!plan) return 0;
    return avr::est_layout(n_slices, n_groups, plan->total_chunks).total;
}
size_t avr_range_keys_verify_workspace_bytes(size_t n_slices, size_t n_groups, const avr_chunk_plan *plan) {
    (void)n_groups;
    if (!plan) return 0;
    return avr::est_verify_layout(n_slices, plan->total_chunks).total;
}

// The refusals of the estimator resolver and of its checker.  other: the call's second array of records, `name` in the header;
// rest: whether the call's remaining pointers are there; quote: what sizes the call's workspace.
static int check_est(const Slices &keys, size_t n_slices, const void *other, const char *name, const uint32_t *group_first, size_t n_groups,
                     const uint8_t *est_in, const uint8_t *est_out, const avr_chunk_plan *plan, const void *workspace, size_t workspace_bytes,
                     bool rest, size_t (*quote)(size_t, size_t, const avr_chunk_plan *), const char *quote_name) {
    if (int rc = check_common(keys.off, keys.n_bins, keys.recs, n_slices)) return rc;
    if (n_groups > 0x7fffffffu) return fail(AVR_ERR_INVALID, "n_groups out of range");
    if (n_slices && (n_groups == 0 || n_groups > n_slices))
        return fail(AVR_ERR_INVALID, "n_groups %zu: a batch of %zu slices has between 1 and %zu groups", n_groups, n_slices, n_slices);
    if (n_slices && (!group_first || !other || !rest)) return fail(AVR_ERR_INVALID, "null device pointer");
    if (!plan || (n_slices && (!plan->chunk_base || !plan->chunk_slice))) return fail(AVR_ERR_INVALID, "null plan pointer");
    if (n_slices && !workspace) return fail(AVR_ERR_INVALID, "null workspace");
    if (workspace_bytes < quote(n_slices, n_groups, plan))
        return fail(AVR_ERR_INVALID, "workspace of %zu bytes is smaller than %s()", workspace_bytes, quote_name);
    const char *keys_name = keys.rec_bytes == 1 ? "keys8" : "keys";
    if (n_slices && other == keys.recs) return fail(AVR_ERR_INVALID, "%s must not alias %s", name, keys_name);
    if ((reinterpret_cast<uintptr_t>(keys.recs) | reinterpret_cast<uintptr_t>(other)) & 15)
        return fail(AVR_ERR_INVALID, "%s / %s not 16-byte aligned", keys_name, name);
    if ((reinterpret_cast<uintptr_t>(est_in) | reinterpret_cast<uintptr_t>(est_out)) & 1)
        return fail(AVR_ERR_INVALID, "est_in / est_out not 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(AVR_ERR_INVALID, "workspace not 256-byte aligned");
    return AVR_OK;
}

int avr_range_resolve_device(int device, void *stream, const uint16_t *keys, const uint64_t *rec_off, const uint32_t *n_bins,
                             size_t n_slices, const uint32_t *group_first, size_t n_groups, const uint8_t *est_in, uint8_t *est_out,
                             const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes, uint16_t *recs_out, int32_t *status) {
    const Slices in{keys, rec_off, n_bins, nullptr, uint32_t(n_slices)};
    if (int rc = check_est(in, n_slices, recs_out, "recs_out", group_first, n_groups, est_in, est_out, plan, workspace, workspace_bytes, status != nullptr,
                           avr_range_resolve_workspace_bytes, "avr_range_resolve_workspace_bytes"))
        return rc;
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_est_resolve(hip(stream), in, group_first, uint32_t(n_groups), est_in, est_out, plan, workspace, recs_out, status));
    return AVR_OK;
}

int avr_range_keys_verify_device(int device, void *stream, const uint16_t *keys, const uint16_t *recs, const uint64_t *rec_off,
                                 const uint32_t *n_bins, size_t n_slices, const uint32_t *group_first, size_t n_groups,
                                 const uint8_t *est_in, const uint8_t *est_out, const avr_chunk_plan *plan, void *workspace,
                                 size_t workspace_bytes, int32_t *status, uint32_t *first_bad) {
    const Slices in{keys, rec_off, n_bins, nullptr, uint32_t(n_slices)};
    if (int rc = check_est(in, n_slices, recs, "recs", group_first, n_groups, est_in, est_out, plan, workspace, workspace_bytes, status && first_bad,
                           avr_range_keys_verify_workspace_bytes, "avr_range_keys_verify_workspace_bytes"))
        return rc;
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_est_verify(hip(stream), in, recs, group_first, uint32_t(n_groups), est_in, est_out, plan, workspace, status, first_bad));
    return AVR_OK;
}

// the same two calls for one-byte key records (AVR_KIND_RANGE_KEYS8): Slices::rec_bytes = 1 picks the kernels' other width
size_t avr_range_resolve8_workspace_bytes(size_t n_slices, size_t n_groups, const avr_chunk_plan *plan) {
    if (!plan) return 0;
    return avr::est_layout(n_slices, n_groups, plan->total_chunks, avr::est::kKeysPad8).total;
}
size_t avr_range_keys8_verify_workspace_bytes(size_t n_slices, size_t n_groups, const avr_chunk_plan *plan) {
    (void)n_groups;
    if (!plan) return 0;
    return avr::est_verify_layout(n_slices, plan->total_chunks, avr::estv::kTabStride8).total;
}

int avr_range_resolve8_device(int device, void *stream, const uint8_t *keys8, const uint64_t *rec_off, const uint32_t *n_bins,
                              size_t n_slices, const uint32_t *group_first, size_t n_groups, const uint8_t *est_in, uint8_t *est_out,
                              const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes, uint16_t *recs_out, int32_t *status) {
    const Slices in{keys8, rec_off, n_bins, nullptr, uint32_t(n_slices), false, {}, 1};
    if (int rc = check_est(in, n_slices, recs_out, "recs_out", group_first, n_groups, est_in, est_out, plan, workspace, workspace_bytes, status != nullptr,
                           avr_range_resolve8_workspace_bytes, "avr_range_resolve8_workspace_bytes"))
        return rc;
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_est_resolve(hip(stream), in, group_first, uint32_t(n_groups), est_in, est_out, plan, workspace, recs_out, status));
    return AVR_OK;
}

int avr_range_keys8_verify_device(int device, void *stream, const uint8_t *keys8, const uint16_t *recs, const uint64_t *rec_off,
                                  const uint32_t *n_bins, size_t n_slices, const uint32_t *group_first, size_t n_groups,
                                  const uint8_t *est_in, const uint8_t *est_out, const avr_chunk_plan *plan, void *workspace,
                                  size_t workspace_bytes, int32_t *status, uint32_t *first_bad) {
    const Slices in{keys8, rec_off, n_bins, nullptr, uint32_t(n_slices), false, {}, 1};
    if (int rc = check_est(in, n_slices, recs, "recs", group_first, n_groups, est_in, est_out, plan, workspace, workspace_bytes, status && first_bad,
                           avr_range_keys8_verify_workspace_bytes, "avr_range_keys8_verify_workspace_bytes"))
        return rc;
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_est_verify(hip(stream), in, recs, group_first, uint32_t(n_groups), est_in, est_out, plan, workspace, status, first_bad));
    return AVR_OK;
}

size_t avr_cabac_resolve_workspace_bytes(size_t n_slices, size_t n_states, const avr_chunk_plan *plan) {
    if (!plan || n_states > AVR_MAX_STATES) return 0;
    return avr::resolve_layout(n_slices, uint32_t(n_states), plan).total;
}

int avr_cabac_resolve_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                             size_t n_slices, const uint8_t *init_states, size_t n_states, const avr_chunk_plan *plan,
                             void *workspace, size_t workspace_bytes, uint8_t *codes, int32_t *status, uint8_t *final_states) {
    if (int rc = check_common(rec_off, n_bins, codes, n_slices)) return rc;
    if (int rc = check_states(n_states)) return rc;
    if (int rc = check_plan(plan, n_slices, true)) return rc;
    if (n_slices && (!workspace || !status)) return fail(AVR_ERR_INVALID, "null workspace / status");
    if (workspace_bytes < avr::resolve_layout(n_slices, uint32_t(n_states), plan).total)
        return fail(AVR_ERR_CAPACITY, "workspace smaller than avr_cabac_resolve_workspace_bytes()");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_k1p_resolve(hip(stream), Slices{recs, rec_off, n_bins, nullptr, uint32_t(n_slices)},
                                    States{init_states, uint32_t(n_states), final_states}, plan, workspace, codes, status));
    return AVR_OK;
}

size_t avr_cabac_resolved_workspace_bytes(size_t n_slices, const avr_chunk_plan *plan) {
    return plan ? avr::code_layout(n_slices, plan).total : 0;
}

int avr_cabac_encode_resolved_device(int device, void *stream, const uint8_t *codes, const uint32_t *n_bins, size_t n_slices,
                                     const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes, uint8_t *out,
                                     const uint64_t *out_off, uint32_t *out_len, int32_t *status) {
    if (int rc = check_common(codes, n_bins, out_off, n_slices)) return rc;
    if (int rc = check_plan(plan, n_slices, false)) return rc;
    if (n_slices && (!workspace || !status)) return fail(AVR_ERR_INVALID, "null workspace / status");
    if (workspace_bytes < avr::code_layout(n_slices, plan).total)
        return fail(AVR_ERR_CAPACITY, "workspace smaller than avr_cabac_resolved_workspace_bytes()");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_k1p_code(hip(stream), Slices{codes, plan->res_off, n_bins, nullptr, uint32_t(n_slices)}, plan, workspace,
                                 Output{out, out_off, out_len, status}));
    return AVR_OK;
}

int avr_cabac_encode_codes_device(int device, void *stream, const uint8_t *codes, const uint64_t *res_off, const uint32_t *n_bins,
                                  const uint32_t *order, size_t n_slices, uint8_t *out, const uint64_t *out_off,
                                  uint32_t *out_len, int32_t *status) {
    if (int rc = check_common(codes, n_bins, out_off, n_slices)) return rc;
    if (n_slices && (!res_off || !status || !out_len)) return fail(AVR_ERR_INVALID, "null device pointer");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_cabac_encode_codes(hip(stream), Slices{codes, res_off, n_bins, order, uint32_t(n_slices)}, Output{out, out_off, out_len, status}));
    return AVR_OK;
}

// The K1 verifier's five forms (avr_cabac_verify.hip).  One body: the checks that need no device, then the launch.
static int cabac_verify_device(int device, void *stream, const Slices &in, size_t n_slices, const StatesView &st, size_t n_states, const OutputView &o,
                               uint32_t *first_bad, bool need_first_bad) {
    if (int rc = check_common(in.off, in.n_bins, o.out_off, n_slices)) return rc;
    const size_t limit = avr::cabac_verify::form_max_states(in.form);
    if (n_states > limit) return fail(AVR_ERR_INVALID, "n_states %zu > %zu", n_states, limit);
    if (n_slices && (!in.recs || !o.out || !o.out_len || !o.status || (need_first_bad && !first_bad) || (n_states && !st.init_states)))
        return fail(AVR_ERR_INVALID, "null device pointer");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_cabac_verify(hip(stream), in, st, o, first_bad));
    return AVR_OK;
}

int avr_cabac_verify_tiles_device(int device, void *stream, const void *tiles, const uint64_t *tile_off, const uint32_t *n_bins,
                                  const uint32_t *order, size_t n_slices, const uint8_t *init_states, size_t n_states,
                                  const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, const uint8_t *final_states,
                                  int32_t *status, uint32_t *first_bad) {
    return cabac_verify_device(device, stream, Slices{tiles, tile_off, n_bins, order, uint32_t(n_slices), true, avr::cabac_verify::kTiles2}, n_slices,
                               StatesView{init_states, uint32_t(n_states), final_states}, n_states, OutputView{out, out_off, out_len, status}, first_bad, false);
}

int avr_cabac_verify_slices_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                                   const uint32_t *order, size_t n_slices, const uint8_t *init_states, size_t n_states,
                                   const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, const uint8_t *final_states,
                                   int32_t *status, uint32_t *first_bad) {
    return cabac_verify_device(device, stream, Slices{recs, rec_off, n_bins, order, uint32_t(n_slices), false, avr::cabac_verify::kSlices2}, n_slices,
                               StatesView{init_states, uint32_t(n_states), final_states}, n_states, OutputView{out, out_off, out_len, status}, first_bad, true);
}

int avr_cabac8_verify_tiles_device(int device, void *stream, const void *tiles, const uint64_t *tile_off, const uint32_t *n_bins,
                                   const uint32_t *order, size_t n_slices, const uint8_t *init_states, size_t n_states,
                                   const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, const uint8_t *final_states,
                                   int32_t *status, uint32_t *first_bad) {
    return cabac_verify_device(device, stream, Slices{tiles, tile_off, n_bins, order, uint32_t(n_slices), true, avr::cabac_verify::kTiles8}, n_slices,
                               StatesView{init_states, uint32_t(n_states), final_states}, n_states, OutputView{out, out_off, out_len, status}, first_bad, false);
}

int avr_cabac8_verify_slices_device(int device, void *stream, const uint8_t *recs8, const uint64_t *rec_off, const uint32_t *n_bins,
                                    const uint32_t *order, size_t n_slices, const uint8_t *init_states, size_t n_states,
                                    const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, const uint8_t *final_states,
                                    int32_t *status, uint32_t *first_bad) {
    return cabac_verify_device(device, stream, Slices{recs8, rec_off, n_bins, order, uint32_t(n_slices), false, avr::cabac_verify::kSlices8}, n_slices,
                               StatesView{init_states, uint32_t(n_states), final_states}, n_states, OutputView{out, out_off, out_len, status}, first_bad, true);
}

int avr_cabac_verify_codes_device(int device, void *stream, const uint8_t *codes, const uint64_t *res_off, const uint32_t *n_bins,
                                  const uint32_t *order, size_t n_slices, const uint8_t *out, const uint64_t *out_off,
                                  const uint32_t *out_len, int32_t *status, uint32_t *first_bad) {
    return cabac_verify_device(device, stream, Slices{codes, res_off, n_bins, order, uint32_t(n_slices), false, avr::cabac_verify::kCodes}, n_slices,
                               StatesView{}, 0, OutputView{out, out_off, out_len, status}, first_bad, true);
}

// The restore check (avr_restore.hip): the checks that need no device, then the launch.
int avr_restore_check_device(int device, void *stream, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, size_t n_slices,
                             const uint8_t *expect, const uint64_t *expect_off, const uint32_t *expect_len, int32_t *status,
                             uint32_t *first_diff) {
    if (n_slices > 0x7fffffffu) return fail(AVR_ERR_INVALID, "n_slices %zu out of range", n_slices);
    if (n_slices && (!out || !out_off || !out_len || !expect || !expect_off || !expect_len || !status || !first_diff))
        return fail(AVR_ERR_INVALID, "null device pointer");
    if (reinterpret_cast<uintptr_t>(expect) & 7) return fail(AVR_ERR_INVALID, "expect is not 8-byte aligned");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_restore_check(hip(stream), OutputView{out, out_off, out_len, status}, uint32_t(n_slices), expect, expect_off, expect_len, first_diff));
    return AVR_OK;
}

// ------------------------------------------------------------------ the plan and the compaction on the device (avr_plan_dev.hip)

void avr_plan_bounds(size_t n_slices, uint64_t max_total_bins, uint64_t *cap_chunks, uint64_t *cap_blocks) {
    avr::plan_dev::bounds(n_slices, max_total_bins, cap_chunks, cap_blocks);
}

size_t avr_plan_workspace_bytes(size_t n_slices) { return size_t(avr::plan_dev::workspace_bytes(n_slices)); }

// what the three calls ask of n_slices, their workspace and an array's alignment: no device needed
static int check_plan_call(size_t n_slices, const void *workspace, size_t workspace_bytes) {
    if (n_slices > 0x7fffffffu) return fail(AVR_ERR_INVALID, "n_slices %zu out of range", n_slices);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255)) return fail(AVR_ERR_INVALID, "workspace null or not 256-byte aligned");
    if (workspace_bytes < avr_plan_workspace_bytes(n_slices))
        return fail(AVR_ERR_INVALID, "workspace of %zu bytes, avr_plan_workspace_bytes says %zu", workspace_bytes, avr_plan_workspace_bytes(n_slices));
    return AVR_OK;
}
static bool misaligned(const void *p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

int avr_plan_chunks_device(int device, void *stream, const uint32_t *n_bins, size_t n_slices, int level, const avr_plan_arrays *arrays,
                           void *workspace, size_t workspace_bytes, avr_plan_totals *totals) {
    if (!arrays || !totals) return fail(AVR_ERR_INVALID, "null arrays or totals");
    if (level < AVR_PLAN_SERIAL || level > AVR_PLAN_K1P) return fail(AVR_ERR_INVALID, "level %d: expected 0..3 (AVR_PLAN_*)", level);
    if (int rc = check_plan_call(n_slices, workspace, workspace_bytes)) return rc;
    const avr_plan_arrays &a = *arrays;
    if (a.rec_round != 8 && a.rec_round != 16) return fail(AVR_ERR_INVALID, "rec_round %u: expected 8 or 16", a.rec_round);
    // the n + 1 arrays are written even for an empty batch (their single zero); chunk_slice / blk_slice only with slices
    if (!a.out_off || (level >= AVR_PLAN_CHUNKS && !a.chunk_base) || (level >= AVR_PLAN_CODES && !a.dig_off) ||
        (level >= AVR_PLAN_K1P && (!a.res_off || !a.blk_base)))
        return fail(AVR_ERR_INVALID, "null array that level %d writes", level);
    if (n_slices && (!n_bins || (level >= AVR_PLAN_CHUNKS && !a.chunk_slice) || (level >= AVR_PLAN_K1P && !a.blk_slice)))
        return fail(AVR_ERR_INVALID, "null array that level %d needs", level);
    if (misaligned(n_bins, 4) || misaligned(totals, 8) || misaligned(a.out_off, 8) || misaligned(a.rec_off, 8) ||
        (level >= AVR_PLAN_CHUNKS && (misaligned(a.chunk_base, 4) || misaligned(a.chunk_slice, 4))) || (level >= AVR_PLAN_CODES && misaligned(a.dig_off, 8)) ||
        (level >= AVR_PLAN_K1P && (misaligned(a.res_off, 8) || misaligned(a.blk_base, 4) || misaligned(a.blk_slice, 4))))
        return fail(AVR_ERR_INVALID, "misaligned array");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_plan_chunks(hip(stream), n_bins, uint32_t(n_slices), level, a, workspace, totals));
    return AVR_OK;
}

int avr_plan_tiles_device(int device, void *stream, const uint32_t *n_bins, size_t n_slices, uint32_t records_per_chunk, uint32_t *order,
                          uint64_t *tile_off, void *workspace, size_t workspace_bytes, avr_plan_totals *totals) {
    if (!totals || !tile_off) return fail(AVR_ERR_INVALID, "null totals or tile_off");
    if (records_per_chunk != 8 && records_per_chunk != 16) return fail(AVR_ERR_INVALID, "records_per_chunk %u: expected 8 or 16", records_per_chunk);
    if (int rc = check_plan_call(n_slices, workspace, workspace_bytes)) return rc;
    if (n_slices && (!n_bins || !order)) return fail(AVR_ERR_INVALID, "null device pointer");
    if (misaligned(n_bins, 4) || misaligned(order, 4) || misaligned(tile_off, 8) || misaligned(totals, 8)) return fail(AVR_ERR_INVALID, "misaligned array");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_plan_tiles(hip(stream), n_bins, uint32_t(n_slices), records_per_chunk, order, tile_off, workspace, totals));
    return AVR_OK;
}

int avr_chunk_plan_from(const avr_plan_arrays *arrays, const avr_plan_totals *totals, avr_chunk_plan *plan) {
    if (!arrays || !totals || !plan) return fail(AVR_ERR_INVALID, "null pointer");
    if (totals->total_chunks > arrays->cap_chunks || totals->total_blocks > arrays->cap_blocks)
        return fail(AVR_ERR_CAPACITY, "%llu chunks and %llu blocks, room for %llu and %llu: the bound on the bins did not hold",
                    (unsigned long long)totals->total_chunks, (unsigned long long)totals->total_blocks, (unsigned long long)arrays->cap_chunks,
                    (unsigned long long)arrays->cap_blocks);
    if ((totals->total_chunks >> 32) || (totals->total_blocks >> 32)) return fail(AVR_ERR_CAPACITY, "2^32 chunks or blocks and more: chunk_base / blk_base have wrapped");
    *plan = avr_chunk_plan{arrays->res_off, arrays->chunk_base, arrays->chunk_slice, arrays->blk_base, arrays->blk_slice, arrays->dig_off,
                           totals->res_total, totals->dig_total, uint32_t(totals->total_chunks), uint32_t(totals->total_blocks)};
    return AVR_OK;
}

int avr_compact_device(int device, void *stream, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, size_t n_slices,
                       uint8_t *dense, uint64_t dense_capacity, uint64_t *dense_off, void *workspace, size_t workspace_bytes) {
    if (!dense_off) return fail(AVR_ERR_INVALID, "null dense_off");
    if (int rc = check_plan_call(n_slices, workspace, workspace_bytes)) return rc;
    if (n_slices && (!out || !out_off || !out_len || (!dense && dense_capacity))) return fail(AVR_ERR_INVALID, "null device pointer");
    if (misaligned(out_off, 8) || misaligned(out_len, 4) || misaligned(dense_off, 8)) return fail(AVR_ERR_INVALID, "misaligned array");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_compact_wide(hip(stream), out, out_off, out_len, uint32_t(n_slices), dense, dense_capacity, dense_off, workspace));
    return AVR_OK;
}

// ------------------------------------------------------------------ the epilogue on the device (avr_plan_dev.hip, avr_finish.h)

size_t avr_finish_workspace_bytes(size_t n_slices) { return size_t(avr::plan_dev::finish_layout(n_slices).total); }

int avr_finish_device(int device, void *stream, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, const int32_t *status,
                      size_t n_slices, const uint32_t *finish, uint8_t *dense, uint64_t dense_capacity, uint64_t *dense_off, void *workspace,
                      size_t workspace_bytes) {
    if (!dense_off) return fail(AVR_ERR_INVALID, "null dense_off");
    if (n_slices > 0x7fffffffu) return fail(AVR_ERR_INVALID, "n_slices %zu out of range", n_slices);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255)) return fail(AVR_ERR_INVALID, "workspace null or not 256-byte aligned");
    if (workspace_bytes < avr_finish_workspace_bytes(n_slices))
        return fail(AVR_ERR_INVALID, "workspace of %zu bytes, avr_finish_workspace_bytes says %zu", workspace_bytes, avr_finish_workspace_bytes(n_slices));
    if (n_slices && (!out || !out_off || !out_len || !finish || (!dense && dense_capacity))) return fail(AVR_ERR_INVALID, "null device pointer");
    if (misaligned(out_off, 8) || misaligned(out_len, 4) || misaligned(status, 4) || misaligned(finish, 4) || misaligned(dense_off, 8))
        return fail(AVR_ERR_INVALID, "misaligned array");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_finish(hip(stream), out, out_off, out_len, status, uint32_t(n_slices), finish, dense, dense_capacity, dense_off, workspace));
    return AVR_OK;
}

// ------------------------------------------------------------------ dense context ids

int avr_context_census_device(int device, void *stream, const uint16_t *recs, uint64_t n_records, uint32_t *bitmap) {
    if ((n_records && !recs) || !bitmap || (n_records & 7)) return fail(AVR_ERR_INVALID, "bad argument (n_records must be a multiple of 8)");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_context_census(hip(stream), recs, n_records, bitmap));
    return AVR_OK;
}

int avr_context_remap_device(int device, void *stream, uint16_t *recs, uint64_t n_records, const uint16_t *table) {
    if ((n_records && !recs) || !table || (n_records & 7)) return fail(AVR_ERR_INVALID, "bad argument (n_records must be a multiple of 8)");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_context_remap(hip(stream), recs, n_records, table));
    return AVR_OK;
}

int avr_states_permute_device(int device, void *stream, const uint8_t *src, size_t n_src, uint8_t *dst, size_t n_dst,
                              const uint16_t *index, size_t n_index, size_t n_slices, int scatter) {
    if (n_slices && n_index && (!src || !dst || !index)) return fail(AVR_ERR_INVALID, "null pointer");
    if (n_src > AVR_MAX_STATES || n_dst > AVR_MAX_STATES || n_index > AVR_MAX_STATES) return fail(AVR_ERR_INVALID, "more than %d states", AVR_MAX_STATES);
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_states_permute(hip(stream), src, uint32_t(n_src), dst, uint32_t(n_dst), index,
                                       uint32_t(n_index), n_slices, scatter));
    return AVR_OK;
}

// ------------------------------------------------------------------ synthetic streams

int avr_synth_config_init(avr_synth_config *cfg, int workload, uint32_t scale_permille, uint64_t first_slice) {
    if (!cfg) return fail(AVR_ERR_INVALID, "null config");
    if (workload < 2 || workload > 5) return fail(AVR_ERR_INVALID, "workload %d: expected 2..5 (BASELINE.json configs)", workload);
    if (scale_permille == 0) return fail(AVR_ERR_INVALID, "scale_permille must be > 0");
    cfg->workload = workload;
    cfg->scale_permille = scale_permille;
    cfg->seed = 0x5EED0000ull + uint64_t(workload);     // SURVEY.md 8(d) seeds
    cfg->first_slice = first_slice;
    cfg->n_states = avr::synth_shape(workload, scale_permille, cfg->seed, 0).n_states;
    return AVR_OK;
}

namespace {
struct HostRecordSink {
    uint16_t *dst;
    uint32_t n = 0;
    void put_record(uint16_t r) { dst[n++] = r; }
};
}  // namespace

int avr_synth_count_host(const avr_synth_config *cfg, int kind, size_t n_slices, uint32_t *n_bins) {
    if (!cfg || (!n_bins && n_slices)) return fail(AVR_ERR_INVALID, "null argument");
    (void)kind;
    for (size_t i = 0; i < n_slices; i++) {
        avr::CountSink cs;
        avr::CabacSink<avr::CountSink> sink(cs);
        avr::synth_slice(cfg->workload, cfg->scale_permille, cfg->seed, cfg->first_slice + i, sink);
        n_bins[i] = cs.n;
    }
    return AVR_OK;
}

int avr_synth_generate_host(const avr_synth_config *cfg, int kind, size_t n_slices, const uint64_t *rec_off, uint16_t *recs,
                            uint8_t *init_states) {
    if (!cfg || ((!rec_off || !recs) && n_slices)) return fail(AVR_ERR_INVALID, "null argument");
    for (size_t i = 0; i < n_slices; i++) {
        HostRecordSink rs{recs + rec_off[i]};
        if (kind == AVR_KIND_CABAC) {
            avr::CabacSink<HostRecordSink> sink(rs);
            avr::synth_slice(cfg->workload, cfg->scale_permille, cfg->seed, cfg->first_slice + i, sink);
            if (init_states)
                for (uint32_t c = 0; c < cfg->n_states; c++)
                    init_states[i * cfg->n_states + c] = avr::synth_init_state(c, cfg->seed, cfg->first_slice + i);
        } else {
            avr::ModelSink<HostRecordSink> sink(rs);
            avr::synth_slice(cfg->workload, cfg->scale_permille, cfg->seed, cfg->first_slice + i, sink);
        }
    }
    return AVR_OK;
}

int avr_synth_count_device(int device, void *stream, const avr_synth_config *cfg, int kind, size_t n_slices, uint32_t *n_bins) {
    if (!cfg || (!n_bins && n_slices) || n_slices > 0x7fffffffu) return fail(AVR_ERR_INVALID, "bad argument");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_synth_count(hip(stream), cfg->workload, cfg->scale_permille, cfg->seed, cfg->first_slice,
                                    kind, uint32_t(n_slices), n_bins));
    return AVR_OK;
}

int avr_synth_generate_slices_device(int device, void *stream, const avr_synth_config *cfg, int kind, size_t n_slices,
                                     const uint64_t *rec_off, uint16_t *recs, uint8_t *init_states) {
    if (!cfg || ((!rec_off || !recs) && n_slices) || n_slices > 0x7fffffffu) return fail(AVR_ERR_INVALID, "bad argument");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_synth_slices(hip(stream), cfg->workload, cfg->scale_permille, cfg->seed, cfg->first_slice,
                                     kind, uint32_t(n_slices), rec_off, recs, init_states, cfg->n_states));
    return AVR_OK;
}

int avr_synth_generate_tiles_device(int device, void *stream, const avr_synth_config *cfg, int kind, size_t n_slices,
                                    const uint32_t *order, const uint64_t *tile_off, void *tiles, uint8_t *init_states) {
    if (!cfg || ((!tile_off || !tiles) && n_slices) || n_slices > 0x7fffffffu) return fail(AVR_ERR_INVALID, "bad argument");
    if (int rc = select_device(device)) return rc;
    AVR_HIP(avr::launch_synth_tiles(hip(stream), cfg->workload, cfg->scale_permille, cfg->seed, cfg->first_slice,
                                    kind, uint32_t(n_slices), order, tile_off, tiles, init_states, cfg->n_states));
    return AVR_OK;
}

// ------------------------------------------------------------------ host epilogue helpers

size_t avr_drop_stop_byte(const uint8_t *buf, size_t len) {
    // decompressor::cabac_decoder::finish, recode.cpp:1508-1512
    return (len > 0 && buf[len - 1] == 0x80) ? len - 1 : len;
}

size_t avr_tail_patch(uint8_t *buf, size_t len, int length_parity, uint8_t last_byte) {
    // decompressor::run, recode.cpp:1354-1360
    if (length_parity == -1) return len;
    if (length_parity != int(len & 1)) { buf[len] = last_byte; return len + 1; }
    if (len > 0) buf[len - 1] = last_byte;
    return len;
}

}  // extern "C"
