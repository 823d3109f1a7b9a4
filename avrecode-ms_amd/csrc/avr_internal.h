// Internal declarations shared by avr_kernels.hip (device code + launchers) and avr_api.cpp
// (the C ABI).  Not installed; the public surface is include/avrecode_ms_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <list>
#include <mutex>

#include "../../include/avrecode_ms_amd.h"
#include "avr_layout.h"

// No-op records: what the packer and the generators pad a slice's last chunk (and a tile's
// shorter lanes) with, so the encode kernels never test a record index against n_bins.
//   K1: selector 1026, bin 0 -> r1 = 0, symbol 0: low, range and states unchanged
//   K2: pos = neg = 0 (never valid in a real record) -> skipped
#define AVR_NOP_CABAC2  (AVR_NOP_CABAC | (AVR_NOP_CABAC << 16))
// transient per-slice status, the hand-over to a serial coder in the same call: K1p's phase D declined the slice (k_cabac_encode_codes
// codes it from the resolved codes the call has made), or the renumbered launch of k_cabac_encode met a context its census missed (a
// second launch without renumbering codes it).  Never leaves a call: the coder that takes the slice writes its real status.
#define AVR_SLICE_RETRY_SERIAL 100
// transient, inside the intra-slice parallel path only: the slice has a bin in a context the sampled census of the
// batch missed (it takes the second, fully counted pass); the slice is finished and must be left alone by that pass
#define AVR_SLICE_RETRY_CENSUS 101
#define AVR_SLICE_DONE         102

namespace avr {

// Run-time switches of the library.
//   * Environment, read ONCE per process (env()), documented in include/avrecode_ms_amd.h; none of them can change a
//     coded byte -- they choose between mappings that produce the same bytes:
//       AVR_K1_PATH=serial|chunked   force one lane per slice / the intra-slice parallel kernels in the batch API
//       AVR_NO_DENSE=1               one-lane-per-slice K1 without the renumbering onto the contexts the batch uses
//       AVR_BATCH_NO_HINT=1          avr_batch_submit always asks the device for the context count (and waits)
//   * Test hooks, compiled in only with -DAVR_TEST_HOOKS (libavrecode_hip_hooks.so, which tests/ load; the product
//     library has neither the setter nor any code that reads them): force the hand-over paths that real streams
//     take once in a blue moon, so that every run of the tests proves them.  All bit-exact as well.
struct Env { int k1_path; bool no_dense, no_hint; };             // k1_path: 0 auto, 1 serial, 2 chunked
const Env &env();
struct TestHooks {
    uint32_t k1p_force_retry_every;  // k_k1p_d hands every n-th slice to the serial kernel (0 = off)
    uint32_t census_stride;          // sampling stride of both census kernels (0 = the built-in 16)
    uint32_t k1_path, no_dense, no_hint;   // the environment switches above, settable per test (non-zero wins over env())
    uint32_t chain_segments;         // K1p: the context chains in segments whatever the batch's size
    uint32_t chain_whole;            // K1p: every context chain start to end (k_k1p_ctxchain alone), no segments
    uint32_t chain_force_redo;       // K1p: the segmented chains hand every n-th (slice, context) pair to the whole-slice walk
    uint32_t k2p_seg_len;            // chunks per segment of K2p's overlapped passes (0 = by batch shape): short slices through many segments
    uint32_t local_waves;            // K1p: waves to a workgroup of k_k1p_local (0 = as many waves to a CU as its LDS takes)
    uint32_t chain_nsegs;            // K1p: segments the context chains are cut in (0 = as many as keep the launch in one round of workgroups)
    uint32_t k2p_wave;               // K2p pass 1: 1 = a wave per slice, 2 = a lane per slice, 3 = a lane per slice and a wave each for the longest (0 = by slice count)
    uint32_t verify_flip;            // batch API with verify on: k > 0 complements bit 7 of byte 0 of slice k - 1's output region between the encode and the verifier
    uint32_t est_flip, est_flip_bin; // batch API with verify on, key records: k > 0 adds one to neg of bin est_flip_bin of slice k - 1's resolved record, between the
                                     // resolver and the encode: encoder and K2 verifier agree on the wrong pair, only the estimator checker can see it
    uint32_t restore_flip;           // batch API, a run that carries the restore check: verify_flip in front of the check (behind the K1 verifier where that is on)
    uint32_t k1p_keep_retry;         // K1p (every form): the slices that leave the parallel path -- declined by the scheme, handed over by phase D -- keep
                                     // AVR_SLICE_RETRY_SERIAL (no serial kernel after it), so a test sees which slices phase D coded itself
};
#ifdef AVR_TEST_HOOKS
TestHooks &test_hooks();
#else
inline const TestHooks &test_hooks() { static const TestHooks none{}; return none; }
#endif
inline int k1_path() { return test_hooks().k1_path ? int(test_hooks().k1_path) : env().k1_path; }
inline bool no_dense() { return test_hooks().no_dense || env().no_dense; }
inline bool no_hint() { return test_hooks().no_hint || env().no_hint; }

// How many LDS rows the renumbered contexts of a batch need is known on the device after the census; the launches
// that follow are sized by it, which costs the host one 4-byte round trip per call.  A caller that has a good guess
// (the batch API: the count of its previous batch) passes it here: the launches are sized by `rows`, nothing waits,
// and the true count is copied to *host_count (pinned) behind the kernels for the caller to check afterwards:
//   * the one-lane-per-slice kernel is exact whatever the guess: contexts beyond `rows` are handed back like
//     contexts the sampled census missed;
//   * the intra-slice parallel kernels are exact iff *host_count <= rows: otherwise the caller runs the call again
//     without a hint (they never fault: a dense id >= rows is treated as "no context").
//   * with a guess the intra-slice parallel path also leaves its second pass (slices with a context the sampled
//     census missed) to the caller: *host_retry (pinned) gets the number of such slices behind the kernels, and a
//     caller that finds it non-zero calls launch_k1p_retry with the arguments of launch_k1p.
//   * sharing: how many calls like this one are in flight on the device at once (the parts of avr_cabac_encode_chunked_device_parts):
//     the context chains are cut into as many segments as keep ALL of them in one round of workgroups (0 = 1).
struct DenseHint { uint32_t rows; uint32_t *host_count; uint32_t *host_retry; uint32_t sharing = 0; };
// The rows to size by, once the census and launch_densemap have left the batch's context count in *n_dense (device) on `s`: the
// hint's guess, the count copied to *hint->host_count behind what is enqueued (nothing waits) -- or, without a guess, the count itself,
// read back (the call waits for the stream) and left in *hint->host_count too; either way no more than n_states.
hipError_t dense_rows(hipStream_t s, const uint32_t *n_dense, uint32_t n_states, const DenseHint *hint, uint32_t *rows);

// Something the library keeps per (device, stream): made on first use, under the pool's mutex, and kept -- work on one stream is
// ordered, so consecutive calls may share it -- until forget() releases what is kept for a stream that is going away.
template <class T>
class StreamPool {
    struct Slot { int dev; hipStream_t s; T x; };
    std::list<Slot> slots_;                                      // a list: the T a call got stays where it is while others are added
    std::mutex mu_;
public:
    // the T of (current device, s); a new one is filled by make(T &), and is not kept if that fails
    template <class Make>
    hipError_t get(hipStream_t s, T **out, Make make) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lock(mu_);
        for (Slot &x : slots_)
            if (x.dev == dev && x.s == s) { *out = &x.x; return hipSuccess; }
        T fresh{};
        if ((e = make(fresh)) != hipSuccess) return e;
        slots_.push_back(Slot{dev, s, fresh});
        *out = &slots_.back().x;
        return hipSuccess;
    }
    // every T kept for s, on whatever device: destroy(T &), then gone
    template <class Destroy>
    void forget(hipStream_t s, Destroy destroy) {
        std::lock_guard<std::mutex> lock(mu_);
        for (auto it = slots_.begin(); it != slots_.end();)
            if (it->s == s) { destroy(it->x); it = slots_.erase(it); } else ++it;
    }
};

// what the library keeps per (device, stream) -- the renumbering's scratch, K2p's second stream and events -- released: call before the stream is destroyed
void forget_stream(hipStream_t s);
void forget_part_streams(hipStream_t s);                      // avr_api.cpp: the streams of avr_cabac_encode_chunked_device_parts kept for s

// One run's arrays as they travel from the C ABI and the batch to the launchers: one type per role, so that a misplaced array does
// not compile.  The launchers unpack them where they launch; no kernel takes one.
namespace cabac_verify { enum Form : int; }                      // avr_cabac_verify.h
// What an encoder reads, and the verifier behind it reads again: the records (tiles, codes) of n_slices slices.
struct Slices {
    const void *recs = nullptr;              // the records (tiles, codes) ...
    const uint64_t *off = nullptr;           // ... and where each slice's (tile's) begin
    const uint32_t *n_bins = nullptr;
    const uint32_t *order = nullptr;         // the slices' order, where the path has one
    uint32_t n_slices = 0;
    bool tiled = false;                      // in tiles (one lane per slice), not slice-major
    cabac_verify::Form form{};               // K1: which of the verifier's forms that is (K2 records are two bytes wide: tiled says it all)
    uint32_t rec_bytes = 2;                  // key records (launch_est_resolve, launch_est_verify): 2, or 1 for AVR_KIND_RANGE_KEYS8
    template <class T> const T *as() const { return static_cast<const T *>(recs); }
};
// The context states of a K1 run, before and after; what only reads them (the verifier) takes the view.
struct StatesView { const uint8_t *init_states = nullptr; uint32_t n_states = 0; const uint8_t *final_states = nullptr; };
struct States {
    const uint8_t *init_states = nullptr; uint32_t n_states = 0; uint8_t *final_states = nullptr;
    operator StatesView() const { return {init_states, n_states, final_states}; }
};
// The coded bytes with their regions, lengths and statuses; the verifiers and the restore check read the bytes and write statuses only.
struct OutputView { const uint8_t *out = nullptr; const uint64_t *out_off = nullptr; const uint32_t *out_len = nullptr; int32_t *status = nullptr; };
struct Output {
    uint8_t *out = nullptr; const uint64_t *out_off = nullptr; uint32_t *out_len = nullptr; int32_t *status = nullptr;
    operator OutputView() const { return {out, out_off, out_len, status}; }
};

hipError_t launch_cabac_encode(hipStream_t s, const Slices &in, const States &st, const Output &o, const DenseHint *hint = nullptr);
// used (1024 bits) -> table[caller's context number] = dense id (0xffff: unused), index[dense id] = caller's number, *n_dense
hipError_t launch_densemap(hipStream_t s, const uint32_t *used, uint16_t *table, uint16_t *index, uint32_t *n_dense);
hipError_t launch_range_encode(hipStream_t s, const Slices &in, const Output &o);
// the K2 verifier (avr_verify.hip): decodes every AVR_SLICE_OK slice back against its records; writes status and first_bad only
hipError_t launch_range_verify(hipStream_t s, const Slices &in, const OutputView &o, uint32_t *first_bad);
// the K1 verifier (avr_cabac_verify.hip): the CABAC decoder of H.264 9.3.3.2 over every AVR_SLICE_OK slice and its records, in.form
// saying which of avr_cabac_verify.h's (kCodes: no states); st.final_states may be null; writes status and first_bad only
hipError_t launch_cabac_verify(hipStream_t s, const Slices &in, const StatesView &st, const OutputView &o, uint32_t *first_bad);
// the restore check (avr_restore.hip): every slice that is AVR_SLICE_OK or AVR_SLICE_VERIFY_FAILED and has an expectation, its coded
// bytes through the decompressor's epilogue rule against the expected payload, a wave per slice; writes status and first_diff only
hipError_t launch_restore_check(hipStream_t s, const OutputView &o, uint32_t n_slices, const uint8_t *expect, const uint64_t *expect_off,
                                const uint32_t *expect_len, uint32_t *first_diff);
#ifdef AVR_TEST_HOOKS
hipError_t launch_verify_flip(hipStream_t s, const Output &o, uint32_t slice);
#endif
// slice-major records (in.order: the slices' order in the tiles) -> tiles; in.recs: const uint16_t *
hipError_t launch_pack_tiles(hipStream_t s, int kind, uint32_t n_states, const Slices &in, const uint64_t *tile_off, void *tiles, int32_t *status);
hipError_t launch_synth_count(hipStream_t s, int workload, uint32_t scale, uint64_t seed,
                              uint64_t first_slice, int kind, uint32_t n_slices, uint32_t *n_bins);
hipError_t launch_synth_tiles(hipStream_t s, int workload, uint32_t scale, uint64_t seed,
                              uint64_t first_slice, int kind, uint32_t n_slices, const uint32_t *order,
                              const uint64_t *tile_off, void *tiles, uint8_t *init_states,
                              uint32_t n_states);

// one-byte K1 records (AVR_KIND_CABAC8, slice i at byte in.off[i], a multiple of 16) -> the two-byte tiles of launch_pack_tiles
hipError_t launch_pack_tiles8(hipStream_t s, uint32_t n_states, const Slices &in, const uint64_t *tile_off, void *tiles, int32_t *status);
// the same records -> ONE-BYTE tiles (16 records a chunk), and the one-lane-per-slice coder on them: no census, no wait
hipError_t launch_pack_tiles8_narrow(hipStream_t s, uint32_t n_states, const Slices &in, const uint64_t *tile_off, void *tiles, int32_t *status);
hipError_t launch_cabac8_encode(hipStream_t s, const Slices &in, const States &st, const Output &o);
hipError_t launch_context_census(hipStream_t s, const uint16_t *recs, uint64_t n, uint32_t *bitmap);
hipError_t launch_context_remap(hipStream_t s, uint16_t *recs, uint64_t n, const uint16_t *table);
hipError_t launch_states_permute(hipStream_t s, const uint8_t *src, uint32_t n_src, uint8_t *dst, uint32_t n_dst,
                                 const uint16_t *index, uint32_t n_index, uint64_t n_slices, int scatter);
// every slice's coded bytes to dense + dense_off[i] (avr_plan_dev.hip's wide copy on the caller's own offsets; dense_total = dense_off[n_slices])
hipError_t launch_compact(hipStream_t s, const OutputView &o, const uint64_t *dense_off, uint32_t n_slices, uint8_t *dense, uint64_t dense_total);

// The intra-slice parallel K1 path (avr_k1p.hip), slice-major records.  Workspace of the three whole-path launchers:
// k1p_layout(n_slices, n_states, pl).total bytes (avr_layout.h, as every workspace here)
hipError_t launch_k1p(hipStream_t s, const Slices &in, const States &st, const avr_chunk_plan *pl, void *workspace, const Output &o,
                      const DenseHint *hint = nullptr);
hipError_t launch_k1p_retry(hipStream_t s, const Slices &in, const States &st, const avr_chunk_plan *pl, void *workspace, const Output &o);
// the same from one-byte records (in.off in bytes, multiples of 16; n_states <= AVR_MAX_STATES8): no census, no wait; workspace as above
hipError_t launch_k1p8(hipStream_t s, const Slices &in, const States &st, const avr_chunk_plan *pl, void *workspace, const Output &o);
hipError_t launch_k1p_resolve(hipStream_t s, const Slices &in, const States &st, const avr_chunk_plan *pl, void *workspace, uint8_t *codes,
                              int32_t *status);
// resolved codes (in.recs), slice i at pl->res_off[i]
hipError_t launch_k1p_code(hipStream_t s, const Slices &in, const avr_chunk_plan *pl, void *workspace, const Output &o);
hipError_t launch_cabac_encode_codes(hipStream_t s, const Slices &in, const Output &o, int32_t want_status = AVR_SLICE_OK);
// K2 for few, long slices (avr_k2p.hip): range recurrence per slice, coding per chunk into byte sums, carries + finish
hipError_t launch_k2p(hipStream_t s, const Slices &in, const avr_chunk_plan *pl, uint64_t out_total, void *workspace, const Output &o);
// the compress direction's estimators (avr_est.hip): key records -> K2 range records, per group of slices; never waits.  keys.rec_bytes
// 1: one-byte key records, keys.off in bytes (recs_out at the same offsets in records), tables of AVR_EST_KEYS8 entries, and the
// workspace est_layout(.., est::kKeysPad8); for launch_est_verify est_verify_layout(.., estv::kTabStride8)
hipError_t launch_est_resolve(hipStream_t s, const Slices &keys, const uint32_t *group_first, uint32_t n_groups, const uint8_t *est_in,
                              uint8_t *est_out, const avr_chunk_plan *pl, void *workspace, uint16_t *recs_out, int32_t *status);
// the estimator checker (avr_est_verify.hip): resolved records held to their key records and to each other (avr_est_verify.h);
// workspace est_verify_layout(n_slices, total_chunks).total bytes; writes status and first_bad only; never waits
hipError_t launch_est_verify(hipStream_t s, const Slices &keys, const uint16_t *recs, const uint32_t *group_first, uint32_t n_groups,
                             const uint8_t *est_in, const uint8_t *est_out, const avr_chunk_plan *pl, void *workspace, int32_t *status,
                             uint32_t *first_bad);
#ifdef AVR_TEST_HOOKS
hipError_t launch_est_flip(hipStream_t s, uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins, uint32_t slice, uint32_t bin);
#endif
hipError_t launch_synth_slices(hipStream_t s, int workload, uint32_t scale, uint64_t seed, uint64_t first_slice,
                               int kind, uint32_t n_slices, const uint64_t *rec_off, uint16_t *recs,
                               uint8_t *init_states, uint32_t n_states);

}  // namespace avr
