/*
 * avrecode_ms_amd.h -- C ABI of the MI355X-native arithmetic re-encode path.
 *
 * Shared library: avrecode-ms_amd/libavrecode_hip.so (built by __graft_entry__.build()).
 * Plain C: pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * What this replaces in the reference (pbluc/avrecode-ms, paths relative to
 * /root/reference):
 *
 *   The reference codes every CABAC bin inline, inside the libavcodec hook
 *   callbacks (recode.cpp:149-171 -> Driver::cabac_decoder::get / get_bypass /
 *   get_terminate):
 *     compress    recode.cpp:1182-1199 -> h264_symbol::execute :1075-1103
 *                 -> recoded_code::encoder::put (arithmetic_code.h:106-126)
 *     decompress  recode.cpp:1442-1481
 *                 -> cabac::encoder::put / put_bypass / put_terminate (cabac_code.h:33-67)
 *   Nothing consumes the coded bytes before the end of the run
 *   (recode.cpp:1131 SerializeAsString, :1352-1363 final loop), so the build's
 *   hook adapter RECORDS one 16-bit record per bin and hands whole batches of
 *   independent slices to the device here.  The entry points are what a cgo /
 *   JNI / ctypes binding -- or the reference's own C++ -- would bind; the
 *   reference-side patch is shown in INTEGRATION.md.
 *
 * Record formats
 *   CABAC record (K1, decompress direction), uint16_t:
 *       bit 0      bin value
 *       bits 1..11 selector: 0..1023  context index = offset of the `uint8_t *state`
 *                                     handed to get() from the slice's first state
 *                                     (recode.cpp:156, context identity is the address, :325)
 *                            1024     bypass     (get_bypass,    recode.cpp:1458-1467)
 *                            1025     terminate  (get_terminate, recode.cpp:1469-1481)
 *   range record (K2, compress direction), uint16_t:
 *       bit 0      bin value
 *       bits 1..7  pos, bits 8..14 neg : the {pos,neg} estimator of the bin's model key at
 *                  the moment it is coded (recode.cpp:823-827, 1064); p(1) = (range/(pos+neg))*pos
 *   key record (compress direction before its estimators are resolved, AVR_KIND_RANGE_KEYS), uint16_t: the bits of the CABAC record
 *       bit 0      bin value
 *       bits 1..11 model key: 0..1023 a context id, AVR_SEL_BYPASS, AVR_SEL_TERMINATE -- the 1026 keys h264_model keeps in flat_[]
 *                  (residual hooks off); bits 12..15 zero.  The device looks up and updates the key's {pos, neg} estimator
 *                  (recode.cpp:823-827, 1037-1052) and makes the range record: the same two bytes feed both directions.
 *   one-byte key record (AVR_KIND_RANGE_KEYS8), uint8_t: a key is only an index into its group's table of estimators, and a real
 *   file meets at most 126 contexts, so a dense id does what the 11-bit key does in half the bytes over PCIe
 *       bit 0      bin value
 *       bits 1..7  dense key id: 0..125 the caller's model keys in a numbering the caller keeps fixed over a whole GROUP,
 *                  AVR_SEL8_BYPASS (126), AVR_SEL8_TERMINATE (127).  All 128 ids are keys: no record value is malformed.
 *   The layout is AVR_KIND_CABAC8's: slice-major, slice i at BYTE rec_off[i], a multiple of 16, readable up to the next multiple of 16;
 *   the bytes past n_bins are padding of any value, told apart by index: never counted, never matched, never validated.  A group with
 *   more than 126 keys keeps the two-byte form.
 *
 * Environment.  The library reads three variables, once per process; NONE of them can change a coded byte -- they pick
 * between mappings that produce the same bytes (tests/ run all of them against the oracle):
 *   AVR_K1_PATH=serial|chunked   batch API: force one lane per slice / the intra-slice parallel kernels (default: by batch shape)
 *   AVR_NO_DENSE=1               one-lane-per-slice K1 keeps the caller's context numbering (no renumbering onto the contexts in use)
 *   AVR_BATCH_NO_HINT=1          avr_batch_submit always asks the device for the batch's context count (and waits for it)
 * There is no switch that alters output.  The switches tests use to force rare hand-over paths exist only in a separate
 * build of the same sources with -DAVR_TEST_HOOKS (libavrecode_hip_hooks.so, avr_test_hook_set); this library has neither
 * the setter nor the code that reads them.
 *
 * Threading: one avr_batch per host thread; calls on different batches are
 * independent.  Errors: functions return AVR_OK (0) or a negative AVR_ERR_*;
 * avr_last_error() gives the message for the calling thread.  The reference
 * throws C++ exceptions through its C callbacks instead (recode.cpp:43,71,99,169,
 * arithmetic_code.h:117); the host wrapper re-throws from these codes.
 */
#ifndef AVRECODE_MS_AMD_H
#define AVRECODE_MS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVR_OK              0
#define AVR_ERR_INVALID    -1   /* bad argument / call order */
#define AVR_ERR_NO_DEVICE  -2   /* no HIP device: there is NO CPU fallback */
#define AVR_ERR_HIP        -3   /* a HIP runtime call failed */
#define AVR_ERR_NOMEM      -4
#define AVR_ERR_CAPACITY   -5   /* more slices / bins than the batch was created for */

/* per-slice status written by the kernels.
 *
 * Malformed records -- one rule for every path that validates.  A slice with a record in [0, n_bins) that no recorder writes
 * comes back AVR_SLICE_BAD_RECORD with length 0:
 *   K1, two-byte   a bit of 12..15 set; a selector neither < n_states nor bypass / terminate (the no-op selector 1026 included:
 *                  only the padding past n_bins may hold it); a put_terminate(1) that is not the slice's last bin
 *   K1, one-byte   a selector in [n_states, 126); a put_terminate(1) that is not last; a rec_off that is not a multiple of 16
 *   K2             bit 15 set, or pos + neg = 0
 *   key records    a bit of 12..15 set, or a key above AVR_SEL_TERMINATE.  The later slices of the record's GROUP have no defined
 *                  estimators, so that slice AND EVERY LATER SLICE OF ITS GROUP come back AVR_SLICE_BAD_RECORD with length 0; earlier
 *                  slices and other groups are coded.  (No rule about put_terminate(1): K2 has none.)
 *   key records,   no record value is malformed; a rec_off that is not a multiple of 16 makes its slice a bad one by the group rule
 *   one-byte       above (that slice and every later slice of its group: AVR_SLICE_BAD_RECORD, length 0).  Such a slice is read from
 *                  the multiple of 16 below its rec_off, and none of its resolved records is written.
 * Enforced by the packers (avr_pack_tiles_device, avr_pack_tiles8_device, avr_pack_tiles8_narrow_device) with the tile coders behind them, by the K1p calls
 * (avr_cabac_encode_chunked_device and its hinted, second-pass and parts forms, avr_cabac8_encode_chunked_device,
 * avr_cabac_resolve_device), by K2p (avr_range_encode_chunked_device), by avr_range_resolve_device and so by the batch API on either path: a slice's status
 * does not depend on the path.  Precedence: AVR_SLICE_BAD_RECORD wins over AVR_SLICE_ZERO_PROB, AVR_SLICE_OVERFLOW and any
 * hand-over inside a path, wherever in the slice the bad record sits.  The slice-major serial entry points
 * (avr_cabac_encode_slices_device, avr_range_encode_slices_device) trust their input.  Resolved codes have no bad value. */
#define AVR_SLICE_OK          0
#define AVR_SLICE_ZERO_PROB   1  /* arithmetic_code.h:116-118 "emitted a zero-probability symbol" */
#define AVR_SLICE_OVERFLOW    2  /* output region too small (never with the batch API's sizing) */
#define AVR_SLICE_BAD_RECORD  3  /* a record the rule above calls malformed */
/* Only ever set by a verifier (K2: avr_range_verify_*_device, avr_batch_set_verify; K1: avr_cabac_verify_*_device,
 * avr_cabac8_verify_*_device, avr_batch_set_verify_k1), and only on a slice that was AVR_SLICE_OK: the slice's coded bytes do not
 * decode back to the bins of its records (K1 also: the decoder's final context states are not the encoder's).  The slice's bytes
 * and length stay retrievable as they are. */
#define AVR_SLICE_VERIFY_FAILED 4           /* only ever set by the verifier */
#define AVR_VERIFY_NONE 0xFFFFFFFFu
/* The restore check (avr_restore_check_device, avr_batch_expect) sets AVR_SLICE_VERIFY_FAILED too, on a slice that was AVR_SLICE_OK
 * and whose coded bytes do not restore the payload the caller expects of it.  AVR_EXPECT_NONE as a slice's expect_len: this slice has
 * no expectation, the check skips it. */
#define AVR_EXPECT_NONE 0xFFFFFFFFu   /* expect_len: this slice has no expectation */

#define AVR_SEL_BYPASS     1024
#define AVR_SEL_TERMINATE  1025
#define AVR_MAX_STATES     1024  /* size of libavcodec's per-slice cabac_state[] */

/* No-op records.  Device layouts keep every slice a whole number of 8-record (16-byte)
 * chunks; the records between a slice's last bin and the chunk end are no-ops, so the encode
 * kernels never compare a record index with n_bins.  K1: selector 1026 with bin 0 (probability
 * range 0, symbol 0: low, range and states unchanged).  K2: pos = neg = 0 (never a real
 * record).  The batch API and avr_pack_tiles_device write them; callers of the slice-major
 * device entry points must. */
#define AVR_NOP_CABAC      (1026 << 1)
#define AVR_NOP_RANGE      0

#define AVR_KIND_CABAC 0         /* K1: cabac::encoder           (cabac_code.h:26-82)   */
#define AVR_KIND_RANGE 1         /* K2: recoded_code::encoder    (recode.cpp:322-323)   */
#define AVR_KIND_CABAC_CODES 2   /* K1 from resolved codes: one byte per bin, see avr_batch_add_slice_codes */
#define AVR_KIND_CABAC8 3        /* K1 from ONE-BYTE records (bin, dense selector), see avr_batch_add_slice_cabac8 */
#define AVR_KIND_RANGE_KEYS 4    /* K2 from KEY records (bin, model key): the estimators are resolved on the device, see avr_batch_begin_group */
#define AVR_EST_KEYS 1026        /* estimators to a table: keys 0 .. AVR_SEL_TERMINATE */
#define AVR_KIND_RANGE_KEYS8 5   /* K2 from ONE-BYTE key records (bin, dense key id), see avr_batch_begin_group8 */
#define AVR_EST_KEYS8 128        /* estimators to a table of one-byte key records: ids 0 .. 125, AVR_SEL8_BYPASS, AVR_SEL8_TERMINATE */

/* One-byte K1 records (AVR_KIND_CABAC8): bit 0 = the bin, bits 1..7 = a dense selector -- 0 .. 125 the slice's contexts in the
 * order the recorder met them (its ids are dense by first appearance already: INTEGRATION.md), AVR_SEL8_BYPASS, AVR_SEL8_TERMINATE.
 * What the record stands for is what the two-byte record stands for (recode.cpp:1442-1481); a stream with more than 126 contexts
 * keeps the two-byte form. */
#define AVR_SEL8_BYPASS     126
#define AVR_SEL8_TERMINATE  127
#define AVR_MAX_STATES8     126

const char *avr_last_error(void);
const char *avr_version(void);
int  avr_device_count(void);                 /* 0 when no GPU is visible */

/* The CABAC tables in the layout cabac_code.h:11-12 indexes (512 and 256 bytes). */
const uint8_t *avr_cabac_lps_range_table(void);
const uint8_t *avr_cabac_mlps_state_table(void);

/* ------------------------------------------------------------------ batch API (host memory)
 * Replaces the per-bin encoder calls of Driver::cabac_decoder (see above).  Usage:
 *   b = avr_batch_create(dev, max_slices, max_bins);
 *   per slice:  avr_batch_add_slice_cabac(...) | avr_batch_add_slice_range(...)
 *   avr_batch_run(b);                      // H2D, pack, encode kernel, D2H
 *   per slice:  avr_batch_get(b, i, &bytes, &len, &status);
 * A batch holds slices of one kind only.  Returned pointers stay valid until the next
 * avr_batch_reset / avr_batch_destroy.  K1 output is the raw encoder output: the caller
 * applies recode.cpp:1508-1512 (drop a trailing 0x80) and :1354-1360 (tail patch),
 * see avr_drop_stop_byte / avr_tail_patch. */
typedef struct avr_batch avr_batch;

avr_batch *avr_batch_create(int device, size_t max_slices, size_t max_bins);
void       avr_batch_destroy(avr_batch *b);
int        avr_batch_reset(avr_batch *b);

/* init_states: n_states bytes (2*pStateIdx+valMPS), the slice's cabac_state[] as it was
 * when the slice's first bin was requested; n_states <= AVR_MAX_STATES and all slices of a
 * batch use the same n_states.  Returns the slice index (>= 0) or an error (< 0). */
int avr_batch_add_slice_cabac(avr_batch *b, const uint16_t *recs, size_t n,
                              const uint8_t *init_states, size_t n_states);
int avr_batch_add_slice_range(avr_batch *b, const uint16_t *recs, size_t n);
/* K1 from RESOLVED CODES: one byte per bin made with AVR_CODE_CONTEXT(state, bin) -- `state` being *state
 * as it is when the bin is requested, which the adapter holds anyway (it updates it, cabac_code.h:43-47) --
 * AVR_CODE_BYPASS(bin) or AVR_CODE_TERMINATE(bin): the (symbol, *state) pairs cabac::encoder::put takes
 * (cabac_code.h:33).  Half the bytes of avr_batch_add_slice_cabac over PCIe, no state arrays, and the
 * context-state resolution on the GPU is skipped.  put_terminate(1), if present, must be the last bin.
 * A batch of few, long slices is coded by the intra-slice parallel kernels (K1p phases B-D), a batch of
 * many short ones by one lane per slice (k_cabac_encode_codes); either way every slice is coded. */
int avr_batch_add_slice_codes(avr_batch *b, const uint8_t *codes, size_t n);
/* K1 from ONE-BYTE records (AVR_KIND_CABAC8, above): the same slice as avr_batch_add_slice_cabac would take, in half the bytes
 * over PCIe -- which is what bounds the batch API end to end (2 B per bin against 0.1 B of output).  init_states: n_states <=
 * AVR_MAX_STATES8 bytes, indexed by the dense selector.  The device reads the one-byte records as they came, with no two-byte copy
 * and no widening: a batch of many short slices through avr_pack_tiles8_narrow_device and avr_cabac8_encode_tiles_device (one-byte
 * tiles, one lane per slice), a batch of few long ones through avr_cabac8_encode_chunked_device -- either way no census and no host
 * round trip, so avr_batch_submit of a one-byte batch never waits, its first run included.
 * Same bytes, final states and statuses as avr_batch_add_slice_cabac -- a selector >= n_states that is neither bypass nor
 * terminate comes back as AVR_SLICE_BAD_RECORD. */
int avr_batch_add_slice_cabac8(avr_batch *b, const uint8_t *recs8, size_t n,
                               const uint8_t *init_states, size_t n_states);
/* K2 from KEY records (AVR_KIND_RANGE_KEYS, above): the compress-direction adapter records what the decompress-direction one
 * records -- the bin and the identity of its context -- and the device resolves the adaptive {pos, neg} estimators.
 * Estimators belong to a GROUP: a run of consecutive slices, in the order they are added, that share one table of AVR_EST_KEYS
 * estimators (a file's slices).  avr_batch_begin_group: the slices added from here on form a new group, which starts from fresh
 * estimators {1, 1} (est_in NULL) or from est_in: AVR_EST_KEYS pairs of bytes {pos, neg}, each with pos >= 1, neg >= 1 and
 * pos + neg <= 0x60 (else AVR_ERR_INVALID).  Returns the group's index.  The first slice of a batch opens a fresh group if none
 * was begun; a batch of this kind holds only this kind.  avr_batch_submit runs the resolver (avr_range_resolve_device) and then the
 * K2 path it would choose for the same slices as AVR_KIND_RANGE; it does not wait.  Bytes, lengths and statuses are those of an
 * AVR_KIND_RANGE batch fed the resolved records.  avr_batch_get_estimators: the group's table after its last bin, in the layout
 * begin_group takes (valid until the next reset / destroy; undefined for a group with a malformed record).  A group split over two
 * batches -- the second begun from the first one's table -- gives the bytes and the table of the unsplit group.
 * avr_multi takes key records with the group as its unit of placement: a group's estimators are one serial table, so all slices of
 * a group go to one device (avr_multi_begin_group, below). */
int avr_batch_begin_group(avr_batch *b, const uint8_t *est_in);
int avr_batch_add_slice_range_keys(avr_batch *b, const uint16_t *recs, size_t n);
int avr_batch_get_estimators(avr_batch *b, size_t group, const uint8_t **pos_neg, size_t *n_keys);
/* K2 from ONE-BYTE key records (AVR_KIND_RANGE_KEYS8, above): the same slices in half the bytes over PCIe, for groups that meet at most
 * 126 keys.  A table (est_in, avr_batch_get_estimators: n_keys = AVR_EST_KEYS8) holds AVR_EST_KEYS8 = 128 {pos, neg} byte pairs in the
 * dense numbering.  avr_batch_begin_group8 is avr_batch_begin_group for this kind -- 128 pairs or NULL, the same validity rule, the
 * group's index returned -- and a call of its own because a group may be begun before the batch's first slice says which kind it
 * holds: it fixes the batch's kind.  avr_batch_begin_group on a batch of this kind is AVR_ERR_INVALID, and so is avr_batch_begin_group8
 * on a batch of any other kind.  Without a group begun, the first slice opens a fresh one.  avr_batch_submit stages one byte a record
 * (avr_batch_timings()[0] shows it), runs avr_range_resolve8_device into the batch's two-byte record buffer and then the K2 path an
 * AVR_KIND_RANGE_KEYS batch of the same slices takes; avr_batch_set_verify runs the K2 verifier over the resolver's output and then
 * avr_range_keys8_verify_device.  Bytes, lengths, statuses, first_bad and tables are those of an AVR_KIND_RANGE_KEYS batch given the
 * widened records (id << 1 | bin, the ids being valid two-byte keys), table entries 0..127.
 * NOT WIRED, deliberately: avr_multi and the `recode` command line take the two-byte form only.  Both are also linked against the CPU
 * stand-in of the batch calls that the tests keep (tests/cpu_batch.cpp), which knows no symbol newer than itself; INTEGRATION.md shows
 * the adapter side (numbering keys densely by first appearance over a file, choosing the form per file). */
int avr_batch_begin_group8(avr_batch *b, const uint8_t *est_in);
int avr_batch_add_slice_range_keys8(avr_batch *b, const uint8_t *recs8, size_t n);
/* Zero-copy form of the calls above: room for a slice of n elements (uint16_t records for AVR_KIND_CABAC /
 * AVR_KIND_RANGE / AVR_KIND_RANGE_KEYS, uint8_t codes for AVR_KIND_CABAC_CODES, uint8_t records for AVR_KIND_CABAC8 / AVR_KIND_RANGE_KEYS8) in the batch's pinned staging buffer, which the H2D copy
 * reads directly; the caller writes exactly n elements to *buffer before avr_batch_submit / avr_batch_run (the padding
 * after them is already in place).  init_states / n_states as for avr_batch_add_slice_cabac (copied now), ignored
 * for the other kinds.  A recorder that appends here saves one pass over its records.  Returns the slice index. */
int avr_batch_reserve_slice(avr_batch *b, int kind, size_t n, const uint8_t *init_states, size_t n_states, void **buffer);

/* avr_batch_run = avr_batch_submit + avr_batch_wait.
 * avr_batch_submit enqueues the whole run on the batch's own stream -- H2D from pinned memory, the kernels, the
 * lengths on their way back -- and returns without waiting for the device (the first two-byte CABAC-record run of a batch
 * object waits once for a 4-byte context count; later runs are sized by that count and checked in avr_batch_wait; a one-byte
 * (AVR_KIND_CABAC8) batch never waits).
 * avr_batch_wait blocks until the results are in host memory.  Between the two calls the batch must not be
 * touched (add / reset / get fail with AVR_ERR_INVALID).  Two or three batch objects used in turn keep the copy
 * engines and the kernels of consecutive batches overlapped:
 *     submit(b[0]);  for (i = 1; ; i++) { fill(b[i % 2]); submit(b[i % 2]); wait(b[(i - 1) % 2]); consume; reset; }
 * After avr_batch_wait a batch may be submitted again as it is (same slices, coded anew). */
int avr_batch_submit(avr_batch *b);
int avr_batch_wait(avr_batch *b);
int avr_batch_run(avr_batch *b);

int avr_batch_get(avr_batch *b, size_t slice, const uint8_t **bytes, size_t *len, int *status);
/* K1 only: the slice's state bytes after its last bin (what cabac_code.h:43-47 leaves in *state). */
int avr_batch_get_states(avr_batch *b, size_t slice, const uint8_t **states, size_t *n_states);
/* How the last run went: [0] 1 = intra-slice parallel kernels, 0 = one lane per slice; [1] context rows the kernels
 * were sized by from the previous run's count (0: the run asked the device and waited, or needed no count); [2] contexts the
 * batch uses (as the sampled census saw them) -- except for a one-byte (AVR_KIND_CABAC8) batch, on either path: it takes no census,
 * so [1] is 0 and [2] is the batch's declared n_states, every one of which has a row; [3] bit 0 = avr_batch_wait found the guess
 * too small and ran the batch again, bit 1 = it ran the second pass of the intra-slice parallel path (slices with a bin in a context
 * the sampled census missed).  CABAC-record batches; zeros otherwise, except that [0] is also 1 when a K2 batch ran K2p (a test of key
 * records sees through it which K2 path coded the batch).  A run of a batch without slices ran nothing: all four are 0, whatever the
 * object's previous run was. */
int avr_batch_run_info(avr_batch *b, uint32_t info[4]);
/* milliseconds of the last run: [0] H2D, [1] pack kernel (for key records: the estimator resolver and the pack kernel), [2] encode kernel, [3] D2H;
 * all 0 for a run of a batch without slices, as are avr_batch_verify_ms, avr_batch_verify_est_ms and avr_batch_restore_ms */
int avr_batch_timings(avr_batch *b, float ms[4]);

/* Verification of a K2 batch (AVR_KIND_RANGE, AVR_KIND_RANGE_KEYS, AVR_KIND_RANGE_KEYS8) on the device: off by default, and then nothing of a run differs.
 * avr_batch_set_verify(b, 1): from the next avr_batch_submit on, the verifier (avr_range_verify_tiles_device on the one-lane-per-slice
 * path, avr_range_verify_slices_device over the slice-major records on the K2p path -- for key records, the resolver's output) is
 * enqueued behind the encode kernels on the batch's stream; avr_batch_submit still does not wait.  The setting stays until it is set
 * again (avr_batch_reset keeps it); AVR_ERR_INVALID while the batch is in flight.  A slice whose bytes do not decode to its bins
 * comes back from avr_batch_get with AVR_SLICE_VERIFY_FAILED, its bytes and length as the encoder left them, and
 * avr_batch_get_verify gives the index of its first bad bin -- AVR_VERIFY_NONE for every other slice, and for every slice of a run
 * with verify off.  avr_batch_timings()[2] stays the encode alone: the verifier sits between two events of its own, and
 * avr_batch_verify_ms reports them (0 for a run with verify off).  Verification exists for the compress direction only: with verify
 * on, avr_batch_submit of a K1 batch returns AVR_ERR_INVALID.
 *   Key records (AVR_KIND_RANGE_KEYS).  The decoder above reads the resolver's output, estimators included: it shows that the bytes
 * decode with the estimators the resolver chose, not that those are the model's.  So behind it the ESTIMATOR CHECKER
 * (avr_range_keys_verify_device, below) holds every resolved record and every group's table afterwards to the key records by the
 * update rule itself, between two events of its own and with answers of its own: avr_batch_get_verify_est gives the slice's first bin
 * whose estimator does not follow the model (n_bins: its padding, or its group's table afterwards), AVR_VERIFY_NONE for a slice
 * without a finding, for batches of other kinds and for runs with verify off; avr_batch_verify_est_ms its time (0 where it did not
 * run; not part of avr_batch_verify_ms).  A slice failed by either check comes back AVR_SLICE_VERIFY_FAILED; avr_batch_get_verify
 * stays the decoder's answer, AVR_VERIFY_NONE for a slice that only the checker failed. */
int avr_batch_set_verify(avr_batch *b, int on);
int avr_batch_get_verify(avr_batch *b, size_t slice, uint32_t *first_bad);
int avr_batch_verify_ms(avr_batch *b, float *ms);
int avr_batch_get_verify_est(avr_batch *b, size_t slice, uint32_t *first_bad);
int avr_batch_verify_est_ms(avr_batch *b, float *ms);

/* Verification of a K1 batch (AVR_KIND_CABAC, AVR_KIND_CABAC8, AVR_KIND_CABAC_CODES) -- the decompress direction, whose product is the
 * user's H.264 file -- switched on by a call of its own: off by default, and then nothing of a run differs.
 * avr_batch_set_verify_k1(b, 1): from the next avr_batch_submit on, the K1 verifier (below: avr_cabac_verify_*_device) is enqueued
 * behind the encode on the batch's stream, over whatever that path's encoder read -- the two-byte or one-byte tiles on the
 * one-lane-per-slice paths, the slice-major records on K1p, the codes on both code paths -- with the encoder's final states to compare
 * where the kind has states; avr_batch_submit still does not wait.  When avr_batch_wait runs a batch a second time, or runs K1p's second
 * pass, the verifier follows again; the last answers are the ones reported.  Everything else is avr_batch_set_verify's: the setting
 * stays (avr_batch_reset keeps it), AVR_ERR_INVALID while the batch is in flight, AVR_SLICE_VERIFY_FAILED with the bytes as the encoder
 * left them, avr_batch_get_verify (the first bad bin; n_bins where only the final states differ), avr_batch_timings()[2] the encode
 * alone and avr_batch_verify_ms the verifier (one exception: where avr_batch_wait ran K1p's second pass, [2] also holds the host's wait
 * and the copies between the two runs -- an upper bound of the encode).  K1 verification exists for the decompress direction only: with it on, avr_batch_submit
 * of a K2 batch returns AVR_ERR_INVALID.  avr_batch_set_verify and its rule for K1 batches are unchanged. */
int avr_batch_set_verify_k1(avr_batch *b, int on);

/* The restore check of a K1 batch (AVR_KIND_CABAC, AVR_KIND_CABAC8, AVR_KIND_CABAC_CODES): will the decompressor's epilogue turn
 * this slice's coded bytes into the payload they were made from?  For a caller that holds the original payload -- the compressor,
 * which can run K1 from the codes its own CABAC decoder sees -- and wants to know it before the original is deleted.
 * avr_batch_expect(b, slice, bytes, len): slice `slice` (already added) is expected to restore bytes[0 .. len); the bytes are copied
 * now, into pinned staging padded to 8.  There is no switch: a run carries the check iff at least one of its slices has an
 * expectation; avr_batch_reset drops them all.  avr_batch_submit sends the expectations to the device on the batch's stream and
 * enqueues avr_restore_check_device (below) behind the encode on whichever path ran, behind the K1 verifier where that is on, between
 * two events of its own; it still does not wait.  When avr_batch_wait runs a batch a second time, or runs K1p's second pass, the check
 * follows again; the last answers are the ones reported.  A slice with a finding comes back from avr_batch_get with
 * AVR_SLICE_VERIFY_FAILED, its bytes and length as the encoder left them; avr_batch_get_restore gives the index of the first byte that
 * differs (the shorter length, where one string is the beginning of the other), AVR_VERIFY_NONE for every other slice and for a run
 * without expectations; avr_batch_restore_ms the check's time (0 where it did not run; no part of avr_batch_timings or
 * avr_batch_verify_ms).  avr_batch_get_verify stays the K1 verifier's answer.  AVR_ERR_INVALID: a K2 batch, a batch in flight or one
 * that has run, a slice index not yet added, a second expectation for one slice, len >= 2^32 - 1, null bytes with len > 0.  With no
 * expectation set, no buffer, event or launch of a run differs. */
int avr_batch_expect(avr_batch *b, size_t slice, const uint8_t *bytes, size_t len);
int avr_batch_get_restore(avr_batch *b, size_t slice, uint32_t *first_diff);
int avr_batch_restore_ms(avr_batch *b, float *ms);

/* ------------------------------------------------------------------ one batch over several GPUs
 * Slices are independent (one coder object each in the reference, recode.cpp:1270, :1525), so a batch shards
 * with no exchange between devices: avr_multi_submit sorts the units by bin count, hands them out heaviest first to
 * the entry of `devices` with the least work so far (greedy LPT, ties to the lower entry, equal weights in the caller's order),
 * fills and submits one avr_batch per entry from a host thread of its own (own stream, own pinned staging), and the getters
 * return results by the caller's slice index.  `devices` may name a device more than once (it then gets that many independent
 * sub-batches).  Same record formats, same rules (one kind per batch, one n_states) and same errors as the single-device batch.
 *
 * THE RULE.  For any sequence of the calls below, an avr_multi over any device list gives, slice by slice and group by group, what
 * ONE avr_batch on devices[0] given the same calls gives: bytes, lengths and statuses; final states; first_bad of either verifier
 * and of the estimator checker; first_diff of the restore check; every group's table afterwards.  Which entry coded a slice, and
 * which K1 / K2 path its sub-batch chose (the choice is per sub-batch, from its own share), shows in none of these.
 *
 * Units.  A unit is a slice; for key records a unit is a whole GROUP, whose weight is the sum of its slices' bins: a group's
 * estimators are one serial table, so every slice of a group goes to one entry, where the entry's groups are begun in the caller's
 * order from the tables copied at avr_multi_begin_group.  A group without slices is no unit and goes to no device;
 * avr_multi_get_estimators answers for it from the multi's own copy of its start table, for every other group from the sub-batch
 * that owned it.  avr_multi_begin_group / avr_multi_add_slice_range_keys carry avr_batch_begin_group's semantics word for word (the
 * first slice opens a fresh group if none was begun; est_in copied and validated at the call; groups only with key records), and a
 * group split over two multis -- the second begun from the first one's table -- gives the bytes and the table of the unsplit group.
 *
 * avr_multi_run = avr_multi_submit + avr_multi_wait.  avr_multi_submit places the units, fills and avr_batch_submits every entry's
 * sub-batch, joins its threads and returns without waiting for any device (the one wait of avr_batch_submit remains: the first
 * two-byte CABAC-record run of a fresh sub-batch).  avr_multi_wait runs avr_batch_wait on every entry, from threads.  Between the two,
 * add, begin_group, expect, reset, the two settings and every getter return AVR_ERR_INVALID; avr_multi_wait without a submit does too.
 * A run of a multi without slices succeeds and runs nothing.  After avr_multi_wait the getters work until avr_multi_reset /
 * avr_multi_destroy; a second submit without a reset is refused ("batch already ran").  Two multis used in turn overlap the
 * copies and kernels of consecutive batches the way two avr_batch objects do.
 * Failure: if one entry's add, submit or wait fails, every entry already submitted is waited for before the call returns -- nothing
 * stays in flight -- and the call returns that entry's code with "device entry E (device D): <its message>".  The object then
 * accepts only avr_multi_reset and avr_multi_destroy.
 *
 * avr_multi_reset drops the slices, groups, expectations, kind and n_states; it keeps the device list, both verify settings and the
 * sub-batches with their device and pinned buffers (AVR_ERR_INVALID while in flight).  On a later run an entry's sub-batch is reused
 * (avr_batch_reset) when the capacity it was created with covers the entry's share; otherwise it is replaced by one that covers the
 * larger of the two.  avr_multi_created: how many avr_batch objects the multi has created so far (a count, valid in every state).
 *
 * The checks are avr_batch's.  avr_multi_set_verify / avr_multi_set_verify_k1: kept over avr_multi_reset, applied to every sub-batch
 * at submit; a K1 kind with set_verify on, or a K2 kind with set_verify_k1 on, is AVR_ERR_INVALID from avr_multi_submit before any
 * sub-batch is touched, so the object stays usable (reset it, or switch the setting off and submit).  avr_multi_expect: the bytes are
 * copied now and go to the owning sub-batch under the slice's local index at submit; avr_batch_expect's refusals apply at the call.
 * avr_multi_get_verify / _get_verify_est / _get_restore / _get_states: the owning sub-batch's answer for the slice.
 * All getters: AVR_ERR_INVALID before a completed run and for an index out of range. */
typedef struct avr_multi avr_multi;
avr_multi *avr_multi_create(const int *devices, size_t n_devices, size_t max_slices, size_t max_bins);
void       avr_multi_destroy(avr_multi *m);
int avr_multi_reset(avr_multi *m);
int avr_multi_created(avr_multi *m);
int avr_multi_add_slice_cabac(avr_multi *m, const uint16_t *recs, size_t n, const uint8_t *init_states, size_t n_states);
int avr_multi_add_slice_range(avr_multi *m, const uint16_t *recs, size_t n);
int avr_multi_add_slice_codes(avr_multi *m, const uint8_t *codes, size_t n);
/* one-byte records, as avr_batch_add_slice_cabac8 (n_states <= AVR_MAX_STATES8) */
int avr_multi_add_slice_cabac8(avr_multi *m, const uint8_t *recs8, size_t n, const uint8_t *init_states, size_t n_states);
int avr_multi_begin_group(avr_multi *m, const uint8_t *est_in);
int avr_multi_add_slice_range_keys(avr_multi *m, const uint16_t *recs, size_t n);
int avr_multi_get_estimators(avr_multi *m, size_t group, const uint8_t **pos_neg, size_t *n_keys);
int avr_multi_set_verify(avr_multi *m, int on);
int avr_multi_set_verify_k1(avr_multi *m, int on);
int avr_multi_expect(avr_multi *m, size_t slice, const uint8_t *bytes, size_t len);
int avr_multi_submit(avr_multi *m);
int avr_multi_wait(avr_multi *m);
int avr_multi_run(avr_multi *m);
int avr_multi_get(avr_multi *m, size_t slice, const uint8_t **bytes, size_t *len, int *status);
int avr_multi_get_states(avr_multi *m, size_t slice, const uint8_t **states, size_t *n_states);
int avr_multi_get_verify(avr_multi *m, size_t slice, uint32_t *first_bad);
int avr_multi_get_verify_est(avr_multi *m, size_t slice, uint32_t *first_bad);
int avr_multi_get_restore(avr_multi *m, size_t slice, uint32_t *first_diff);
/* which entry of `devices` coded the slice, and the bins each entry was given (n_devices values): for tests and reports */
int avr_multi_placement(avr_multi *m, size_t slice);
int avr_multi_load(avr_multi *m, uint64_t *bins_per_device);
/* avr_batch_run_info of the entry's sub-batch; ms[0..3] its avr_batch_timings, ms[4] avr_batch_verify_ms, ms[5]
 * avr_batch_verify_est_ms, ms[6] avr_batch_restore_ms.  Zeros for an entry that got no slice. */
int avr_multi_entry_info(avr_multi *m, size_t entry, uint32_t info[4]);
int avr_multi_entry_ms(avr_multi *m, size_t entry, float ms[7]);

/* ------------------------------------------------------------------ device-resident API
 * All pointers below are DEVICE pointers on `device`; `stream` is a hipStream_t (NULL = the
 * null stream).  Calls enqueue work on `stream` and return, with ONE exception: the K1 entry points that take
 * two-byte (bin, selector) records -- avr_cabac_encode_tiles_device / _slices_device / _chunked_device and
 * avr_cabac_resolve_device -- size their launches by the number of contexts the batch uses, which the device counts:
 * they wait on `stream` once for that 4-byte count (the chunked forms a second time, for the 4-byte count of slices that
 * need their second pass), i.e. they block the calling thread until the stream has drained up to their census kernel.
 * A caller that must not block uses the batch API (avr_batch_submit sizes the launches by the previous batch's count and
 * checks afterwards), the same scheme on its own buffers (avr_cabac_encode_tiles_device_hinted / _chunked_device_hinted below: the
 * caller passes the count an earlier call reported and looks at what this one reports when it next synchronises), one-byte records
 * (avr_pack_tiles8_narrow_device + avr_cabac8_encode_tiles_device, avr_cabac8_encode_chunked_device: no wait, no guess), or resolved
 * codes (avr_cabac_encode_resolved_device / _codes_device and every K2 entry: no wait).  avr_cabac_encode_tiles_device blocks behind
 * avr_pack_tiles8_device's two-byte tiles as behind any other.
 * These are what the batch API is made of and what bench.py times with inputs already resident in HBM (its K1 steps: the hinted calls).
 * MEMORY: what a workspace (or a code buffer, or an output array) holds on entry is arbitrary -- no call needs it cleared, and a workspace may
 * be handed from one batch to another as it stands.  A call writes nothing outside [workspace, workspace + workspace_bytes) and the documented
 * extents of its output arrays: out[out_off[i] .. out_off[i] + out_len[i]) of every slice (nothing else of `out`, not a byte past out_off[n_slices]),
 * n_slices entries of out_len and status, n_slices * n_states final states, res_total + 32 bytes of codes, tile_off[n_tiles] * 16 bytes of tiles.
 * A region [out_off[i], out_off[i + 1]) may be any size, gaps of 2^32 bytes and more included; a slice uses at most 2^32 - 1 bytes of it.
 * A slice that a one-lane-per-slice coder gives up on while coding it (AVR_SLICE_OVERFLOW; avr_cabac8_encode_tiles_device: a put_terminate(1)
 * that is not last) may have had bytes of its own region written before -- nothing outside [out_off[i], out_off[i + 1]).
 * STREAMS: whatever a call runs on streams of its own is joined back: work enqueued on `stream` behind the call sees all of its results
 * and may overwrite its workspace (tests/test_gpu_workspace.py holds the library to all three).
 * ONE THREAD PER STREAM: the library keeps a few kilobytes of scratch (and, for the chunked K2, a second stream with its
 * events) per (device, stream); a call's kernels find them there, so two host threads must not enqueue on the same stream
 * at the same time.  What is kept for a batch's own stream is released by avr_batch_destroy.
 *
 * Slice-major layout: slice i's records are recs[rec_off[i] .. rec_off[i] + n_bins[i]);
 * rec_off[] entries are multiples of 8 records (16 bytes).
 *
 * Wave-interleaved tile layout (what the encode kernels read): slices are taken 64 at a
 * time in `order` (order[g] = slice handled by lane g%64 of tile g/64).  A tile holds
 * max-over-its-lanes ceil(n_bins/8) chunks; chunk c of lane l is the 16 bytes at
 *   tiles + (tile_off[t] + c*64 + l) * 16
 * so one wave-wide load instruction reads 1 KiB contiguous.  tile_off has n_tiles+1 entries
 * in units of 16-byte chunks. */
/* Also validates every record (it is the one place each record is read exactly once) by the rule above (AVR_SLICE_*): a bad
 * record sets status[slice] = AVR_SLICE_BAD_RECORD.  status must be zero-filled before. */
int avr_pack_tiles_device(int device, void *stream, int kind, size_t n_states,
                          const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins,
                          const uint32_t *order, size_t n_slices,
                          const uint64_t *tile_off, void *tiles, int32_t *status);

/* K1.  init_states: n_slices*n_states bytes indexed by slice; out_off: n_slices+1 byte offsets
 * into out, each a multiple of 8; out_len/status indexed by slice; final_states may be NULL.
 * status is in/out: a slice whose status is already non-zero (set by the packer) is skipped
 * with out_len 0; otherwise the kernel writes AVR_SLICE_*.  Records are trusted to be valid
 * (packer / generator output); a selector that is not a context of the slice, bypass or
 * terminate is treated as a no-op. */
/* The packer for ONE-BYTE records (AVR_KIND_CABAC8): slice i's records are recs8[rec_off[i] .. rec_off[i] + n_bins[i]), rec_off in
 * BYTES, each a multiple of 16, and readable up to the next multiple of 16 (what lies past n_bins is never coded, whatever it holds).
 * Writes the two-byte tile layout above -- what avr_cabac_encode_tiles_device and its hinted form read -- with the same checks:
 * a selector that is neither < n_states (<= AVR_MAX_STATES8) nor AVR_SEL8_BYPASS / AVR_SEL8_TERMINATE, or a rec_off value that
 * is not a multiple of 16, sets status[slice] = AVR_SLICE_BAD_RECORD.  status must be zero-filled before.  Refused before anything
 * touches a device (AVR_ERR_INVALID): n_states > AVR_MAX_STATES8, a null pointer with n_slices > 0, recs8 not 16-byte aligned,
 * rec_off not 8-byte aligned. */
int avr_pack_tiles8_device(int device, void *stream, size_t n_states,
                           const uint8_t *recs8, const uint64_t *rec_off, const uint32_t *n_bins,
                           const uint32_t *order, size_t n_slices,
                           const uint64_t *tile_off, void *tiles, int32_t *status);

int avr_cabac_encode_tiles_device(int device, void *stream,
                                  const void *tiles, const uint64_t *tile_off,
                                  const uint32_t *n_bins, const uint32_t *order, size_t n_slices,
                                  const uint8_t *init_states, size_t n_states,
                                  uint8_t *out, const uint64_t *out_off,
                                  uint32_t *out_len, int32_t *status, uint8_t *final_states);

/* ONE-BYTE tile layout (AVR_KIND_CABAC8 records as they are, no widening): the wave-interleaved layout above with SIXTEEN one-byte
 * records per 16-byte chunk.  Chunk c of lane l of tile t is the 16 bytes at
 *   tiles + (tile_off[t] + 64*c + l) * 16
 * and holds records 16c .. 16c+15 of slice order[64t + l]; a tile holds max-over-its-lanes ceil(n_bins/16) chunks (tile_off in
 * 16-byte units, as above).  The bytes of a slice's last chunk past n_bins are padding: never coded, whatever they hold -- a byte has
 * no no-op value (with n_states = 126 every selector means something), so the coder tells padding apart by its index.
 *
 * avr_pack_tiles8_narrow_device: the arguments and the slice-major input of avr_pack_tiles8_device (rec_off in bytes, multiples of 16,
 * reads starting at multiples of 16), the same validation (a selector in [n_states, 126) or a rec_off that is not a multiple of 16:
 * AVR_SLICE_BAD_RECORD for that slice alone; status zero-filled before) and the same refusals before anything touches a device,
 * tiles not 16-byte aligned among them; the records are transposed into one-byte tiles in the same pass.  A lane writes its own
 * slice's chunks only: the rest of its column of a tile is left as it was (never read).
 *
 * avr_cabac8_encode_tiles_device: the one-lane-per-slice coder on one-byte tiles -- the arguments of avr_cabac_encode_tiles_device,
 * with n_states <= AVR_MAX_STATES8, and the same bytes, final states and statuses as it gives on the same slices as two-byte records
 * (a slice whose status is already non-zero is skipped with length 0; a put_terminate(1) that is not the slice's last bin:
 * AVR_SLICE_BAD_RECORD with length 0; AVR_SLICE_OVERFLOW for a region too small).  The selectors are dense ids below n_states already,
 * so the call has nothing to count or renumber: it NEVER BLOCKS THE CALLING THREAD -- no census, no read-back, no guess, no second
 * launch, no allocation; every kernel is enqueued on `stream` and the call returns.  Refused before anything touches a device
 * (AVR_ERR_INVALID): n_states > AVR_MAX_STATES8, a null pointer with n_slices > 0 (init_states may be null when n_states is 0;
 * final_states may be null), tiles not 16-byte aligned. */
int avr_pack_tiles8_narrow_device(int device, void *stream, size_t n_states,
                                  const uint8_t *recs8, const uint64_t *rec_off, const uint32_t *n_bins,
                                  const uint32_t *order, size_t n_slices,
                                  const uint64_t *tile_off, void *tiles, int32_t *status);
int avr_cabac8_encode_tiles_device(int device, void *stream,
                                   const void *tiles, const uint64_t *tile_off,
                                   const uint32_t *n_bins, const uint32_t *order, size_t n_slices,
                                   const uint8_t *init_states, size_t n_states,
                                   uint8_t *out, const uint64_t *out_off,
                                   uint32_t *out_len, int32_t *status, uint8_t *final_states);

/* K2. */
int avr_range_encode_tiles_device(int device, void *stream,
                                  const void *tiles, const uint64_t *tile_off,
                                  const uint32_t *n_bins, const uint32_t *order, size_t n_slices,
                                  uint8_t *out, const uint64_t *out_off,
                                  uint32_t *out_len, int32_t *status);

/* K2 verifier: the decoder of the recoded coder (arithmetic_code.h:209-298) over slices whose records are known, one lane per slice
 * -- what the encoder was given, (range / (pos + neg)) * pos from each record, the decoder is given too, and the bin it decodes is
 * compared with the record's.  It shares nothing with the encoders' carry handling or finish(), so it checks all three K2 paths.
 * Layouts, `order`, out_off and out_len as for avr_range_encode_tiles_device / avr_range_encode_slices_device (padding records must
 * be no-ops); run it behind the encode on the same stream.  status is in/out:
 *   a slice whose status is not AVR_SLICE_OK on entry is skipped: its status stays, first_bad[slice] = AVR_VERIFY_NONE;
 *   an AVR_SLICE_OK slice has its n_bins records decoded in order from out[out_off[i] .. out_off[i] + min(out_len[i], capacity));
 *   at the first bin that decodes to another value the lane stops: first_bad[slice] = that bin's index, status[slice] =
 *   AVR_SLICE_VERIFY_FAILED; otherwise first_bad[slice] = AVR_VERIFY_NONE and the status stays AVR_SLICE_OK.
 * first_bad may be NULL in the tiles call (the status alone is wanted).  Nothing else is written: not out, out_len, records or tiles.
 * Bytes at or past a slice's length read as zero whatever the region holds there, and nothing outside a slice's region is read.
 * The calls enqueue on `stream` and return: they never block, allocate or use a workspace.  Refused before anything touches a
 * device (AVR_ERR_INVALID): a null pointer with n_slices > 0 (order may be NULL in the slices call). */
int avr_range_verify_tiles_device(int device, void *stream, const void *tiles, const uint64_t *tile_off,
                                  const uint32_t *n_bins, const uint32_t *order, size_t n_slices,
                                  const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
                                  int32_t *status, uint32_t *first_bad /* may be NULL */);
int avr_range_verify_slices_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off,
                                   const uint32_t *n_bins, const uint32_t *order /* may be NULL */, size_t n_slices,
                                   const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
                                   int32_t *status, uint32_t *first_bad);

/* K1 verifier: the arithmetic decoder of ITU-T H.264 (9.3.1.2; 9.3.3.2: DecodeDecision, DecodeBypass, DecodeTerminate) over slices
 * whose records are known, one lane per slice.  A K1 slice's output is a standard CABAC stream and every bin's context is known from the
 * records, so the decoder is handed the context of each bin, decodes the bin and compares it with the record's.  It is written from
 * the standard, has no carries, no deferred digits and no finish(), and works the context states out itself by the sequential rule of
 * Figure 9-3 in the CALLER's numbering (no dense renumbering): it is independent of the encoders -- the one-lane kernels, K1p's
 * speculative replay, census, dense map, chains and phase D, the one-byte and the code forms -- except for one thing it shares with
 * them, rangeTabLPS and the state transitions (avr_cabac_lps_range_table / avr_cabac_mlps_state_table hold the same values).
 * WHAT IT COSTS: one lane per slice is a slice's whole serial chain, so on batches of few, long slices (K1p's shapes) it takes a
 * multiple of the encode; a chunk-parallel verifier would start from the encoder's own per-chunk states and would not be independent.
 * Five record forms behind the same walk:
 *   avr_cabac_verify_tiles_device    two-byte tiles, as avr_cabac_encode_tiles_device reads them; n_states <= AVR_MAX_STATES
 *   avr_cabac_verify_slices_device   two-byte records, slice-major (rec_off in records, multiples of 8; padding never decoded)
 *   avr_cabac8_verify_tiles_device   one-byte tiles, the layout of avr_pack_tiles8_narrow_device; n_states <= AVR_MAX_STATES8
 *   avr_cabac8_verify_slices_device  one-byte records, slice-major (rec_off in bytes, multiples of 16, readable to the next multiple of 16)
 *   avr_cabac_verify_codes_device    resolved codes (AVR_CODE_*) at res_off[i] (bytes, multiples of 16, readable to the next multiple
 *                                    of 16): each code is the (symbol, *state) pair itself, so no states are kept -- code < 252 is a
 *                                    context bin at state code >> 1, 252 / 253 bypass, 254 / 255 a decision at pStateIdx 63 (LPS range 2
 *                                    in every quarter), which for a slice's last bin is DecodeTerminate
 * init_states: n_slices * n_states bytes, as the encoder was given; final_states: the encoder's, or NULL.  status is in/out:
 *   a slice whose status is not AVR_SLICE_OK on entry is skipped: its status stays, first_bad[slice] = AVR_VERIFY_NONE;
 *   an AVR_SLICE_OK slice has bins 0 .. n_bins - 1 decoded in order from out[out_off[i] .. out_off[i] + min(out_len[i], capacity));
 *   at the first bin that decodes to another value (or whose selector is no context of the slice, bypass or terminate) the lane stops
 *   with its chunk: first_bad[slice] = that bin's index, status[slice] = AVR_SLICE_VERIFY_FAILED;
 *   where every bin decoded right and final_states is given, the decoder's own states are compared with it, all n_states bytes:
 *   a difference is first_bad[slice] = n_bins (no bin has that index) with AVR_SLICE_VERIFY_FAILED;
 *   otherwise first_bad[slice] = AVR_VERIFY_NONE and the status stays AVR_SLICE_OK.
 * Records at an index >= n_bins are never decoded, whatever they hold.  first_bad may be NULL in the tiles calls.  Nothing else is
 * written: not out, out_len, records, tiles or states.  Bits at or past a slice's length read as zero whatever the region holds there,
 * and nothing outside a slice's region is read.  The calls enqueue on `stream` and return: they never block, allocate or use a
 * workspace.  Refused before anything touches a device (AVR_ERR_INVALID): a null pointer with n_slices > 0 (order may be NULL in the
 * slices and codes calls, init_states when n_states is 0), n_slices >= 2^31, n_states above the form's limit. */
int avr_cabac_verify_tiles_device(int device, void *stream, const void *tiles, const uint64_t *tile_off,
                                  const uint32_t *n_bins, const uint32_t *order, size_t n_slices,
                                  const uint8_t *init_states, size_t n_states,
                                  const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
                                  const uint8_t *final_states /* may be NULL */, int32_t *status, uint32_t *first_bad /* may be NULL */);
int avr_cabac_verify_slices_device(int device, void *stream, const uint16_t *recs, const uint64_t *rec_off,
                                   const uint32_t *n_bins, const uint32_t *order /* may be NULL */, size_t n_slices,
                                   const uint8_t *init_states, size_t n_states,
                                   const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
                                   const uint8_t *final_states /* may be NULL */, int32_t *status, uint32_t *first_bad);
int avr_cabac8_verify_tiles_device(int device, void *stream, const void *tiles, const uint64_t *tile_off,
                                   const uint32_t *n_bins, const uint32_t *order, size_t n_slices,
                                   const uint8_t *init_states, size_t n_states,
                                   const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
                                   const uint8_t *final_states /* may be NULL */, int32_t *status, uint32_t *first_bad /* may be NULL */);
int avr_cabac8_verify_slices_device(int device, void *stream, const uint8_t *recs8, const uint64_t *rec_off,
                                    const uint32_t *n_bins, const uint32_t *order /* may be NULL */, size_t n_slices,
                                    const uint8_t *init_states, size_t n_states,
                                    const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
                                    const uint8_t *final_states /* may be NULL */, int32_t *status, uint32_t *first_bad);
int avr_cabac_verify_codes_device(int device, void *stream, const uint8_t *codes, const uint64_t *res_off,
                                  const uint32_t *n_bins, const uint32_t *order /* may be NULL */, size_t n_slices,
                                  const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
                                  int32_t *status, uint32_t *first_bad);

/* Restore check: the decompressor's epilogue applied to coded K1 slices where they lie, a wave per slice, and the result compared with
 * the payload the caller expects (avrecode-ms_amd/csrc/avr_restore.h holds the rule, avr_restore.hip the kernel).  For slice i with
 * coded bytes out[out_off[i] .. + L), L = min(out_len[i], capacity), and expectation expect[expect_off[i] .. + E), E = expect_len[i]:
 *   finish       L1 = L - 1 if L > 0 and the last coded byte is 0x80, else L (avr_drop_stop_byte: one byte, never two);
 *   tail patch   with what the compressor writes into the container, parity E & 1 and last byte expect[E - 1], both for E >= 2 only
 *                (for E < 2 nothing is patched and R = L1): if (L1 & 1) != (E & 1) the restored bytes are the L1 coded bytes and the
 *                last byte behind them, R = L1 + 1; otherwise the L1 coded bytes with the last of them replaced by the last byte (where
 *                L1 > 0), R = L1 (avr_tail_patch);
 *   answer       first_diff[i] = the smallest j < min(R, E) at which the restored bytes differ from the expectation; else min(R, E)
 *                if R != E; else AVR_VERIFY_NONE.
 * expect_off: n_slices entries, multiples of 8, and each expectation readable to the next multiple of 8; `expect` itself 8-byte aligned;
 * out_off as everywhere (n_slices + 1 entries, multiples of 8).  expect_len[i] == AVR_EXPECT_NONE: no expectation.  status is in/out:
 *   a slice takes part when it comes in as AVR_SLICE_OK or AVR_SLICE_VERIFY_FAILED (a verifier may have run before) and has an
 *   expectation; every other slice is skipped: first_diff[i] = AVR_VERIFY_NONE, its status left as it was;
 *   a finding turns AVR_SLICE_OK into AVR_SLICE_VERIFY_FAILED.
 * Nothing else is written: not out, out_len or expect.  No word of `out` that starts at or past L is read, whatever the region holds
 * there, and nothing outside [out_off[i], out_off[i + 1]) and the padded expectation.  The call enqueues on `stream` and returns: it
 * never blocks, allocates or uses a workspace.  It shares NOTHING with the encoders -- no table, no carry rule, no finish() -- and with
 * avr_drop_stop_byte / avr_tail_patch the rule, written a second time and held equal by the tests.  What it proves: K1, finish, the
 * tail patch and the container's two fields give back the real payload.  What it does not: the host range decoder (K3) and the host
 * parser's agreement with itself on the way back.  Refused before anything touches a device (AVR_ERR_INVALID): a null pointer with
 * n_slices > 0, n_slices >= 2^31, `expect` not 8-byte aligned. */
int avr_restore_check_device(int device, void *stream,
                             const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, size_t n_slices,
                             const uint8_t *expect, const uint64_t *expect_off /* n_slices entries, multiples of 8 */,
                             const uint32_t *expect_len, int32_t *status, uint32_t *first_diff);

/* K1, intra-slice parallel form ("K1p", avrecode-ms_amd/csrc/avr_k1p.h): the same bytes as
 * avr_cabac_encode_tiles_device, produced by many lanes per slice -- for batches of few, long
 * slices (a 1-slice-per-frame clip), where one lane per slice leaves the chip idle.  Input is the
 * slice-major layout (padding records must be no-ops).  Everything runs per chunk of AVR_CHUNK_BINS bins:
 * context states are resolved by a counting sort of each chunk's bins by context (one lane per chunk) and one
 * state chain per (slice, context) over the sorted chunks; the arithmetic coding per chunk follows.  The call
 * renumbers the batch onto the contexts it uses by itself (a census pass over blocks of AVR_SORT_BLOCK_BINS
 * bins, which also validates every record).  The caller supplies the plan (device arrays, n = n_slices):
 *   res_off[i]     byte offset of slice i in the per-bin work arrays, multiple of 16,
 *                  res_off[i+1] - res_off[i] >= roundup16(n_bins[i]) + 16;      res_total = res_off[n]
 *   chunk_base[i]  first global chunk of slice i; it has max(1, ceil(n_bins[i]/AVR_CHUNK_BINS))
 *                  chunks; total_chunks = chunk_base[n]; chunk_slice[c] = slice of global chunk c
 *   blk_base[i], blk_slice[b], total_blocks: the same for blocks of AVR_SORT_BLOCK_BINS bins (the census grid)
 *   dig_off[i]     first 32-bit digit sum of slice i, dig_off[i+1] - dig_off[i] >= n_bins[i]/2 + 8;
 *                  dig_total = dig_off[n]
 * workspace: avr_cabac_chunked_workspace_bytes(...) bytes of device memory, 256-byte aligned.
 * status is in/out as for the tile kernels; this path validates every record itself.  A slice the
 * scheme declines (no coded LPS for 16 consecutive chunks) is coded by the serial kernel in the
 * same call. */
#define AVR_CHUNK_BINS       1024
#define AVR_SORT_BLOCK_BINS  4096
typedef struct {
    const uint64_t *res_off;
    const uint32_t *chunk_base;
    const uint32_t *chunk_slice;
    const uint32_t *blk_base;
    const uint32_t *blk_slice;
    const uint64_t *dig_off;
    uint64_t res_total;
    uint64_t dig_total;
    uint32_t total_chunks;
    uint32_t total_blocks;
} avr_chunk_plan;

size_t avr_cabac_chunked_workspace_bytes(size_t n_slices, size_t n_states, const avr_chunk_plan *plan);
int avr_cabac_encode_chunked_device(int device, void *stream,
                                    const uint16_t *recs, const uint64_t *rec_off,
                                    const uint32_t *n_bins, size_t n_slices,
                                    const uint8_t *init_states, size_t n_states,
                                    const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                                    uint8_t *out, const uint64_t *out_off,
                                    uint32_t *out_len, int32_t *status, uint8_t *final_states);

/* K1p from ONE-BYTE records (AVR_KIND_CABAC8; layout as for avr_pack_tiles8_device: rec_off in bytes, multiples of 16, the bytes
 * past n_bins in a slice's last 16 are padding of any value).  The same bytes, final states and statuses as
 * avr_cabac_encode_chunked_device on the same slices as two-byte records, the same plan (blk_base / blk_slice are not read: there is
 * no census), workspace avr_cabac8_chunked_workspace_bytes(...).  The selectors are dense ids below n_states <= AVR_MAX_STATES8
 * already, so the call has nothing to count or renumber: it NEVER BLOCKS THE CALLING THREAD -- every kernel is enqueued on `stream`
 * and the call returns, with no read-back of a context count, no guess to check afterwards and no second pass (what the two-byte
 * call and its hinted form need).  Validation is as strict as the two-byte call's: a selector in [n_states, 126), a
 * put_terminate(1) that is not the slice's last bin, or a rec_off value that is not a multiple of 16 sets AVR_SLICE_BAD_RECORD for
 * that slice alone.  Refused before anything touches a device: as avr_pack_tiles8_device, and a workspace too small (AVR_ERR_CAPACITY). */
size_t avr_cabac8_chunked_workspace_bytes(size_t n_slices, size_t n_states, const avr_chunk_plan *plan);
int avr_cabac8_encode_chunked_device(int device, void *stream,
                                     const uint8_t *recs8, const uint64_t *rec_off,
                                     const uint32_t *n_bins, size_t n_slices,
                                     const uint8_t *init_states, size_t n_states,
                                     const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                                     uint8_t *out, const uint64_t *out_off,
                                     uint32_t *out_len, int32_t *status, uint8_t *final_states);

/* The K1 device calls SIZED BY THE CALLER'S GUESS of how many contexts the batch uses (r4) -- the count an earlier call reported,
 * which is how avr_batch runs from its second batch on -- so that the call enqueues everything and returns: the calls above read
 * that count back from the device before they can size their launches (avr_cabac_encode_chunked_device: two host round trips a
 * call, 70 us of config 2's 1.55 ms; the tiles call: one).
 *   rows_hint  0 = no guess: ask the device and wait, as the calls above do (the counts are reported all the same).
 *   counts     two words of PINNED host memory, valid once the caller has synchronised `stream`: counts[0] = context rows the
 *              batch needs, counts[1] = slices left for a second pass (chunked call only: slices with a bin in a context the
 *              sampled census missed).
 * What the caller does once it has synchronised.  Tiles call: nothing, it is exact whatever the guess (a slice the guess did not
 * fit was coded by the call's second launch).  Chunked call: counts[0] > rows_hint -- the outputs are NOT valid: restore `status`
 * to what it held before the call and call again with rows_hint = 0; else counts[1] > 0 --
 * avr_cabac_encode_chunked_second_pass_device with the same arguments codes the slices that were left. */
int avr_cabac_encode_tiles_device_hinted(int device, void *stream,
                                         const void *tiles, const uint64_t *tile_off,
                                         const uint32_t *n_bins, const uint32_t *order, size_t n_slices,
                                         const uint8_t *init_states, size_t n_states,
                                         uint8_t *out, const uint64_t *out_off,
                                         uint32_t *out_len, int32_t *status, uint8_t *final_states,
                                         uint32_t rows_hint, uint32_t *counts);
int avr_cabac_encode_chunked_device_hinted(int device, void *stream,
                                           const uint16_t *recs, const uint64_t *rec_off,
                                           const uint32_t *n_bins, size_t n_slices,
                                           const uint8_t *init_states, size_t n_states,
                                           const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                                           uint8_t *out, const uint64_t *out_off,
                                           uint32_t *out_len, int32_t *status, uint8_t *final_states,
                                           uint32_t rows_hint, uint32_t *counts);
int avr_cabac_encode_chunked_second_pass_device(int device, void *stream,
                                                const uint16_t *recs, const uint64_t *rec_off,
                                                const uint32_t *n_bins, size_t n_slices,
                                                const uint8_t *init_states, size_t n_states,
                                                const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                                                uint8_t *out, const uint64_t *out_off,
                                                uint32_t *out_len, int32_t *status, uint8_t *final_states);

/* A batch as several parts at once (r4).  The kernels of the intra-slice parallel path are launched over a part's chunks in rounds of
 * workgroups, and the last round of each is part empty -- for a batch the size of config 2 (4 736 waves against the 2 048 and 3 072 its
 * two longest kernels hold at a time) a third of one kernel and half of another.  Slices are independent, so a batch cut into parts of
 * consecutive slices, each part with a plan and a workspace of its own and run on a stream of its own, fills those rounds with the
 * other parts' kernels: config 2 in three parts 1.41 -> 1.32 ms.  This call is that: part i is avr_cabac_encode_chunked_device_hinted on
 * its own arguments (pointers of the whole batch's arrays moved to the part's first slice; rec_off / out_off values stay offsets into
 * the shared recs / out), on a stream the library keeps for (device, stream); the parts start when `stream` has reached the call and
 * `stream` continues when all are done.  What the caller does about each part's counts: as for the hinted call. */
typedef struct {
    const uint64_t *rec_off;  const uint32_t *n_bins;  size_t n_slices;
    const uint8_t *init_states;
    const avr_chunk_plan *plan;  void *workspace;  size_t workspace_bytes;
    const uint64_t *out_off;  uint32_t *out_len;  int32_t *status;  uint8_t *final_states;
    uint32_t rows_hint;  uint32_t *counts;
} avr_chunked_part;
#define AVR_MAX_PARTS 8
int avr_cabac_encode_chunked_device_parts(int device, void *stream, const uint16_t *recs, size_t n_states, uint8_t *out,
                                          const avr_chunked_part *parts, size_t n_parts);

/* K2, intra-slice parallel form ("K2p", avrecode-ms_amd/csrc/avr_k2p.h): the same bytes as avr_range_encode_slices_device for
 * batches of few, long slices.  The range recurrence of arithmetic_code<uint64_t, uint8_t> (recode.cpp:322-323, 823-827) is
 * walked by one lane per slice -- it is exact 63-bit arithmetic on its own previous value and does not decompose --
 * while low, the output bytes, the carries and finish() (arithmetic_code.h:128-144) are done per chunk of AVR_CHUNK_BINS
 * bins and per slice.  Of the plan only chunk_base, chunk_slice and total_chunks are used; out_total = out_off[n_slices];
 * out_off as for the other entry points (capacity n_bins + 16 per slice at least).  Input is the slice-major layout; every record
 * in [0, n_bins) is validated by the rule above (AVR_SLICE_*), the padding past it must be AVR_NOP_RANGE. */
size_t avr_range_chunked_workspace_bytes(size_t n_slices, const avr_chunk_plan *plan, uint64_t out_total);
int avr_range_encode_chunked_device(int device, void *stream,
                                    const uint16_t *recs, const uint64_t *rec_off,
                                    const uint32_t *n_bins, size_t n_slices,
                                    const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                                    uint8_t *out, const uint64_t *out_off, uint64_t out_total,
                                    uint32_t *out_len, int32_t *status);

/* The compress direction's estimators on the device (avrecode-ms_amd/csrc/avr_est.h): KEY records in, K2 range records out.
 * keys / recs_out: the slice-major layout above with the same rec_off (16-byte aligned, recs_out must not alias keys).  recs_out
 * gets bin | pos << 1 | neg << 8 for [0, n_bins) of every slice and AVR_NOP_RANGE from there to the slice's next multiple of 8 records
 * (what lies between that and the next slice's rec_off is not touched), so it goes straight into
 * avr_pack_tiles_device(AVR_KIND_RANGE) + avr_range_encode_tiles_device or into avr_range_encode_chunked_device.
 *   group_first   n_groups + 1 entries on the DEVICE, group g = slices [group_first[g], group_first[g + 1]), group_first[0] = 0,
 *                 non-decreasing, group_first[n_groups] = n_slices; trusted like rec_off.  1 <= n_groups <= n_slices.
 *   est_in        n_groups tables of AVR_EST_KEYS byte pairs {pos, neg} (2-byte aligned; trusted: pos, neg >= 1, pos + neg <= 0x60),
 *                 or NULL: every group starts fresh {1, 1}
 *   est_out       the same layout, every group's table after its last bin, or NULL: not wanted
 *   plan          chunk_base, chunk_slice and total_chunks are used
 *   workspace     avr_range_resolve_workspace_bytes(...) bytes, 256-byte aligned:
 *                 align256(4 n_slices) + align256(4 n_groups) + 2 ceil(total_chunks / 16) * 6168
 *   status        in/out, zero-filled before (or a packer's / an earlier call's): a malformed record (rule above) sets
 *                 AVR_SLICE_BAD_RECORD for its slice and every later slice of the group; the records of such slices are undefined
 * The call enqueues on `stream` and returns: it never waits for the device, whatever the shape -- groups of one short slice each and
 * one group of all slices run through the same kernels (a group inside one window of 16 chunks is resolved by one wave start to end;
 * a longer one in rows of a window each, with one short chain per key over the rows).  Refused before anything touches a device
 * (AVR_ERR_INVALID): a null pointer with n_slices > 0, n_groups of 0 or above n_slices, a null plan, a workspace smaller than
 * avr_range_resolve_workspace_bytes, recs_out == keys, misaligned keys / recs_out / est_in / est_out / workspace. */
size_t avr_range_resolve_workspace_bytes(size_t n_slices, size_t n_groups, const avr_chunk_plan *plan);
int avr_range_resolve_device(int device, void *stream,
                             const uint16_t *keys, const uint64_t *rec_off, const uint32_t *n_bins, size_t n_slices,
                             const uint32_t *group_first, size_t n_groups,
                             const uint8_t *est_in, uint8_t *est_out,
                             const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                             uint16_t *recs_out, int32_t *status);

/* The estimator checker (avrecode-ms_amd/csrc/avr_est_verify.h): are `recs` the K2 records the model's update rule gives for `keys`?
 * A check of avr_range_resolve_device's output that shares nothing with it.  step(e, b): pos += b, neg += 1 - b, and both halved
 * rounding up if pos + neg > 0x60.  Over each group's bins in stream order: (1) bit 0 of a record is bit 0 of its well-formed key
 * record; (2) a key's first bin in the group carries est_in[group][key], {1, 1} without est_in; (3) every other bin carries step of
 * the RECORDED pair and the bin of the key's previous bin; (4) the records from n_bins to the slice's next multiple of 8 are
 * AVR_NOP_RANGE; (5) est_out[group][key], where est_out is given, is step of the key's last recorded pair and bin, or the start entry
 * of a key the group never met.  The arguments are avr_range_resolve_device's, `recs` being its recs_out and est_out read only.
 *   workspace     avr_range_keys_verify_workspace_bytes(...) bytes, 256-byte aligned:
 *                 align256(4 n_slices) + 2 ceil(total_chunks / 16) * 4112
 *                 -- never more than avr_range_resolve_workspace_bytes for the same batch: the resolver's may be handed on as it stands
 *   status        in/out.  A slice that comes in as AVR_SLICE_BAD_RECORD takes no part, nor (the resolver's rule, relied on) any later
 *                 slice of its group: first_bad = AVR_VERIFY_NONE, and (5) is not checked for that group.  Every other slice takes
 *                 part whatever its status; one with a finding goes from AVR_SLICE_OK to AVR_SLICE_VERIFY_FAILED, any other status stays.
 *   first_bad     per slice: the smallest bin index that violates (1), (2) or (3); n_bins for (4), and for (5) on the group's last
 *                 slice, unless a smaller index is noted; else AVR_VERIFY_NONE.  The same from run to run.
 * Nothing else is written; nothing is read between a slice's padded records and the next rec_off.  The call enqueues on `stream` and
 * returns: it neither waits nor allocates.  A group inside one span of 16 chunks is checked by one wave; a longer one also gets, per
 * span and key, the estimator its next bin must carry and from those the table at every span's start.  Refused before anything
 * touches a device (AVR_ERR_INVALID): a null pointer with n_slices > 0, n_groups of 0 or above n_slices, a null plan, recs == keys,
 * misaligned keys / recs / est_in / est_out / workspace, a workspace below the quoted size, n_slices >= 2^31. */
size_t avr_range_keys_verify_workspace_bytes(size_t n_slices, size_t n_groups, const avr_chunk_plan *plan);
int avr_range_keys_verify_device(int device, void *stream,
                                 const uint16_t *keys, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins, size_t n_slices,
                                 const uint32_t *group_first, size_t n_groups,
                                 const uint8_t *est_in /* may be NULL */, const uint8_t *est_out /* may be NULL */,
                                 const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                                 int32_t *status, uint32_t *first_bad);

/* The two stages of K1p on their own.
 *
 * Stage 1, avr_cabac_resolve_device: context-state resolution (phase A).  Writes one RESOLVED CODE
 * per bin, slice i at codes + res_off[i] (codes must hold res_total + 32 bytes, 256-byte aligned):
 *     (state << 1) | bin   context bin met in state = 2*pStateIdx + valMPS <= 125
 *     252 | bin            bypass bin
 *     255 - bin            put_terminate(bin) (and a context bin at pStateIdx 63 with symbol bin)
 * i.e. exactly the inputs cabac::encoder::put takes -- (symbol, *state) -- per bin (cabac_code.h:33).
 *
 * Stage 2, avr_cabac_encode_resolved_device: the arithmetic coding (phases B-D) from resolved codes.
 * A hook adapter that tracks *state itself -- it has to keep libavcodec's state bytes current anyway,
 * cabac_code.h:43-47 -- can record resolved codes directly with the AVR_CODE_* macros and skip stage 1.
 * The plan is the one of avr_cabac_encode_chunked_device (blk_* unused by stage 2).  A slice whose digit
 * sums phase D does not resolve in parallel (a carry of two or more into a 33-digit segment of the form
 * ffff ... fffe) is coded by the serial kernel below in the same call: every slice comes back coded.
 *
 * avr_cabac_encode_codes_device: the serial form, one lane per slice straight from the codes (no plan, no
 * workspace): for batches of many short slices.  order may be NULL (else: slices taken longest first). */
#define AVR_CODE_CONTEXT(state, bin)  ((state) >= 126 ? 255 - (((bin) ^ (state)) & 1) : (((state) << 1) | (bin)))
#define AVR_CODE_BYPASS(bin)          (252 | (bin))
#define AVR_CODE_TERMINATE(bin)       (255 - (bin))
size_t avr_cabac_resolve_workspace_bytes(size_t n_slices, size_t n_states, const avr_chunk_plan *plan);
int avr_cabac_resolve_device(int device, void *stream,
                             const uint16_t *recs, const uint64_t *rec_off,
                             const uint32_t *n_bins, size_t n_slices,
                             const uint8_t *init_states, size_t n_states,
                             const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                             uint8_t *codes, int32_t *status, uint8_t *final_states);
size_t avr_cabac_resolved_workspace_bytes(size_t n_slices, const avr_chunk_plan *plan);
int avr_cabac_encode_resolved_device(int device, void *stream,
                                     const uint8_t *codes, const uint32_t *n_bins, size_t n_slices,
                                     const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                                     uint8_t *out, const uint64_t *out_off,
                                     uint32_t *out_len, int32_t *status);

int avr_cabac_encode_codes_device(int device, void *stream,
                                  const uint8_t *codes, const uint64_t *res_off, const uint32_t *n_bins,
                                  const uint32_t *order, size_t n_slices,
                                  uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int32_t *status);

/* Variants that read the slice-major layout directly (one 16-byte load per lane per 8 bins,
 * uncoalesced across lanes); kept for the layout comparison in DESIGN.md and for tests.  The
 * padding records up to each slice's next multiple of 8 must be no-op records. */
int avr_cabac_encode_slices_device(int device, void *stream,
                                   const uint16_t *recs, const uint64_t *rec_off,
                                   const uint32_t *n_bins, const uint32_t *order, size_t n_slices,
                                   const uint8_t *init_states, size_t n_states,
                                   uint8_t *out, const uint64_t *out_off,
                                   uint32_t *out_len, int32_t *status, uint8_t *final_states);
int avr_range_encode_slices_device(int device, void *stream,
                                   const uint16_t *recs, const uint64_t *rec_off,
                                   const uint32_t *n_bins, const uint32_t *order, size_t n_slices,
                                   uint8_t *out, const uint64_t *out_off,
                                   uint32_t *out_len, int32_t *status);

/* ------------------------------------------------------------------ the plan, and the way back, on the device
 * Every device-resident call above takes a plan: out_off and the arrays of an avr_chunk_plan for the intra-slice parallel paths, the
 * estimator resolver and checker; `order` and tile_off for the packers and the one-lane-per-slice coders.  A caller whose lengths
 * (n_bins) lie in HBM makes them here, from the rules the batch API applies on the host (avrecode-ms_amd/csrc/avr_plan.h; the kernels
 * in avr_plan_dev.hip call the same per-slice functions), and gets its coded bytes back dense without the lengths leaving the device.
 * All three device calls enqueue on `stream` and return: they never wait or allocate, and write nothing outside
 * [workspace, workspace + workspace_bytes), `totals` and the extents given below (MEMORY and STREAMS above hold for them as they stand).
 *   workspace   avr_plan_workspace_bytes(n_slices) bytes of device memory, 256-byte aligned: one quote that covers each of the three
 *               calls (about 16 bytes a slice and a megabyte), arbitrary on entry, free again once the call's work has run
 *   totals      DEVICE or PINNED HOST memory, 8-byte aligned, valid once the caller has synchronised `stream` (the scheme of `counts`
 *               of the hinted calls).  A plan call fills only its own fields: avr_plan_chunks_device all but tile_chunks,
 *               avr_plan_tiles_device tile_chunks alone -- both may be handed the same struct.
 * The sequence of a device-resident caller: avr_plan_bounds sizes chunk_slice / blk_slice from an upper bound on the
 * bins that the caller, who allocated the records, knows; the plan calls; ONE synchronisation; avr_chunk_plan_from makes the struct the
 * existing calls take and says whether the bound held; the *_workspace_bytes quotes follow from it.
 *
 * avr_plan_bounds (host): cap_chunks = max_total_bins / AVR_CHUNK_BINS + n_slices, cap_blocks = max_total_bins / AVR_SORT_BLOCK_BINS +
 * n_slices -- a slice has at most n_bins / 1024 + 1 chunks, an empty one has one; no list of n_slices lengths with that sum has more.
 *
 * avr_plan_chunks_device: element for element what the host plan holds for the same lengths.  `level` says which arrays are written
 * (each level those of the levels before it); the others, and their caps, are ignored:
 *   AVR_PLAN_SERIAL   out_off[n + 1]: slice i may write roundup8(n_bins[i] + 16) bytes; and rec_off[n + 1] unless NULL: the slice-major
 *                     record offsets, slice i taking roundup(n_bins[i], rec_round) -- rec_round 8: two-byte records, offsets in
 *                     records; 16: one-byte records, offsets in bytes
 *   AVR_PLAN_CHUNKS   chunk_base[n + 1], chunk_slice[total_chunks]                  (K2p, the estimator resolver and checker)
 *   AVR_PLAN_CODES    dig_off[n + 1]                                                (K1p from resolved codes)
 *   AVR_PLAN_K1P      res_off[n + 1], blk_base[n + 1], blk_slice[total_blocks]      (the whole of K1p)
 * chunk_base and blk_base are 32 bits wide as in avr_chunk_plan; the totals are 64.  chunk_slice[k] is never written for k >= cap_chunks,
 * nor blk_slice[k] for k >= cap_blocks, whatever n_bins holds: a bound that did not hold costs the plan (avr_chunk_plan_from refuses
 * it), not memory.  A total of a level above `level` is 0, rec_total is 0 without rec_off.
 *
 * avr_chunk_plan_from (host, after the synchronisation): AVR_ERR_CAPACITY when total_chunks > cap_chunks or total_blocks > cap_blocks,
 * or when either is 2^32 or more (the 32-bit arrays have wrapped); else *plan points at `arrays` with the totals filled in.
 *
 * avr_plan_tiles_device: order[n] = the slices by n_bins descending over the full 32-bit range, equal lengths in the caller's order
 * (a stable sort); tile_off[n_tiles + 1], n_tiles = ceil(n / 64): tile t holds 64 * ceil(n_bins[order[64 t]] / records_per_chunk)
 * 16-byte chunks (8: two-byte records; 16: one-byte tiles); totals->tile_chunks = tile_off[n_tiles], the tile buffer's size in chunks.
 *
 * avr_compact_device: dense_off[n + 1] = the exclusive prefix sum of min(out_len[i], out_off[i + 1] - out_off[i]) with the total
 * appended -- what avr_batch_wait works out on the host -- and slice i's bytes copied to dense + dense_off[i], in 8-byte words over an
 * aligned body, if they end at or before dense_capacity.  No byte at or past dense_capacity is written; dense_off is complete either
 * way, so an overflow shows as dense_off[n] > dense_capacity (that slice and all later ones were not copied).  out_off: multiples of 8
 * as everywhere, gaps of any size; all offsets 64 bits wide.  Run it behind the encode on the same stream.
 *
 * Refused before anything touches a device (AVR_ERR_INVALID): a null array that the level needs, or a null n_bins / order / tile_off /
 * out / out_off / out_len / dense / dense_off, with n_slices > 0; null arrays, totals or (with a quote above 0) workspace; a level
 * outside 0..3; rec_round or records_per_chunk neither 8 nor 16; an array not aligned to its element, a workspace not 256-byte aligned;
 * a workspace below the quote; n_slices >= 2^31.  n_slices == 0 writes the single zero of each n + 1 array and zero totals. */
/* AVR_NOWAIT marks a call that enqueues on `stream` and returns whatever its arguments: no wait, no allocation, no stream of its own.
 * (It also sets the three calls apart for tests/device_api_refusals.py, whose table is made from the parameter names of the unmarked
 * *_device declarations and cannot describe a struct of arrays with caps; tests/test_plan_bounds.py holds these three to their refusals,
 * tests/test_finish_bounds.py avr_finish_device below to its own.) */
#define AVR_NOWAIT
#define AVR_PLAN_SERIAL 0   /* out_off (+ rec_off)                                  */
#define AVR_PLAN_CHUNKS 1   /* + chunk_base, chunk_slice      (K2p, resolver)       */
#define AVR_PLAN_CODES  2   /* + dig_off                      (K1p from codes)      */
#define AVR_PLAN_K1P    3   /* + res_off, blk_base, blk_slice                       */

typedef struct {            /* DEVICE arrays the caller allocated; those a level does not write are ignored */
    uint64_t *out_off;      /* n + 1 */
    uint64_t *rec_off;      /* n + 1, or NULL: slice-major record offsets; slice i takes roundup(n_bins[i], rec_round)  */
    uint32_t  rec_round;    /* 8 (two-byte records, offsets in records) or 16 (one-byte, offsets in bytes) */
    uint32_t *chunk_base;  uint32_t *chunk_slice;  uint64_t cap_chunks;
    uint64_t *dig_off;  uint64_t *res_off;
    uint32_t *blk_base;    uint32_t *blk_slice;    uint64_t cap_blocks;
} avr_plan_arrays;

typedef struct { uint64_t total_bins, out_total, rec_total, res_total, dig_total, total_chunks, total_blocks, tile_chunks; } avr_plan_totals;

void   avr_plan_bounds(size_t n_slices, uint64_t max_total_bins, uint64_t *cap_chunks, uint64_t *cap_blocks);   /* host */
size_t avr_plan_workspace_bytes(size_t n_slices);                                                               /* host, covers all three calls */
int avr_plan_chunks_device(int device, void *stream, const uint32_t *n_bins, size_t n_slices, int level,
                           const avr_plan_arrays *arrays, void *workspace, size_t workspace_bytes, avr_plan_totals *totals) AVR_NOWAIT;
int avr_plan_tiles_device(int device, void *stream, const uint32_t *n_bins, size_t n_slices, uint32_t records_per_chunk /* 8 | 16 */,
                          uint32_t *order, uint64_t *tile_off, void *workspace, size_t workspace_bytes, avr_plan_totals *totals) AVR_NOWAIT;
int avr_chunk_plan_from(const avr_plan_arrays *arrays, const avr_plan_totals *totals, avr_chunk_plan *plan);     /* host, after a sync */
int avr_compact_device(int device, void *stream, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, size_t n_slices,
                       uint8_t *dense, uint64_t dense_capacity, uint64_t *dense_off /* n + 1 */, void *workspace, size_t workspace_bytes) AVR_NOWAIT;

/* ------------------------------------------------------------------ the way back's epilogue on the device
 * avr_compact_device ends at coded bytes.  The bytes a NAL unit holds are one step further: the stop byte dropped (avr_drop_stop_byte),
 * the tail patched (avr_tail_patch) and, for a slice whose container block says so, emulation prevention put back -- which changes
 * lengths, so that a caller whose output stays in HBM could not know where slice i + 1 starts without it.  avr_finish_device is
 * avr_compact_device with that step in it (avr_plan_dev.hip, the per-run rules in avrecode-ms_amd/csrc/avr_finish.h): it enqueues on
 * `stream` and returns, never waits or allocates, and writes nothing outside its workspace, dense_off[0 .. n] and dense[0 .. capacity).
 *   finish[i]   one word per slice, on the device (AVR_FINISH_WORD):
 *                 bits 0-7    last_byte            bit 8   length_parity
 *                 bit 9       the container had both (the tail is patched; without it bits 0-8 are ignored)
 *                 bit 10      escape               bits 11-12   the zero bytes directly in front of the payload (3 is taken as 2)
 *   status      n words on the device, or NULL: every slice is AVR_SLICE_OK.  A slice of any other status gives no bytes.
 *   workspace   avr_finish_workspace_bytes(n_slices) bytes of device memory (a quote of its own), 256-byte aligned, arbitrary on entry
 * Per slice: L = min(out_len[i], out_off[i + 1] - out_off[i]) bytes are taken, as compaction has it; one trailing 0x80 is dropped; with
 * bit 9 the last byte is appended where the length's parity differs from bit 8, else written over the last byte (where there is one);
 * with bit 10 the result p becomes escape(p, z): s = z; for every byte b: if s == 2 and b <= 3, 0x03 is emitted and s = 0; b is
 * emitted; s = b == 0 ? s + 1 : 0.  A slice grows to L + 1 + (L + 1 + z) / 2 bytes at the most.
 * dense_off[n + 1] is the exclusive prefix sum of the final lengths with the total appended, complete whatever the capacity; slice i's
 * bytes go to dense + dense_off[i] whole or not at all, and no byte is written at or past dense_capacity: avr_compact_device's
 * contract, and its very output where every word of `finish` is 0 and no slice ends on 0x80.  All lengths and offsets are 64 bits wide.
 * Refused as avr_compact_device refuses (AVR_ERR_INVALID), `finish` being one more array that may not be null with n_slices > 0 and
 * must be 4-byte aligned, as `status` must where it is given.
 * avr_batch and avr_multi do not finish: their lengths reach the host anyway.  Nor does the command line, which keeps its host
 * epilogue (its CPU build links a stand-in for this library that knows no symbol newer than the batch's). */
#define AVR_FINISH_WORD(last_byte, length_parity, patch, escape, zeros_before) \
    ((uint32_t)((last_byte) & 0xffu) | (uint32_t)((length_parity) & 1u) << 8 | (uint32_t)((patch) ? 1u : 0u) << 9 | \
     (uint32_t)((escape) ? 1u : 0u) << 10 | (uint32_t)((zeros_before) > 2u ? 2u : (zeros_before)) << 11)
size_t avr_finish_workspace_bytes(size_t n_slices);                                                             /* host */
int avr_finish_device(int device, void *stream, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
                      const int32_t *status /* or NULL: all OK */, size_t n_slices, const uint32_t *finish /* n, device */,
                      uint8_t *dense, uint64_t dense_capacity, uint64_t *dense_off /* n + 1 */, void *workspace, size_t workspace_bytes) AVR_NOWAIT;

/* ------------------------------------------------------------------ the estimators from ONE-BYTE key records (AVR_KIND_RANGE_KEYS8)
 * avr_range_resolve_device and avr_range_keys_verify_device for one-byte key records (format above): the same kernels in another
 * width, and the contracts of the two-byte calls word for word -- enqueue on `stream` and return, no wait, no allocation, nothing
 * written outside the documented extents, the same refusals -- with these differences:
 *   keys8         one byte a record; slice i at BYTE rec_off[i], a multiple of 16 (else: the group rule above, AVR_SLICE_BAD_RECORD),
 *                 readable to the next multiple of 16; what lies past n_bins there may hold anything.  16-byte aligned.
 *   recs_out/recs two-byte K2 range records at the SAME rec_off counted in RECORDS: bin | pos << 1 | neg << 8 for [0, n_bins),
 *                 AVR_NOP_RANGE from n_bins to the slice's next multiple of 8 -- not 16: the K2 packers, K2p and the K2 verifier read what
 *                 they read behind the two-byte resolver -- and nothing beyond.  recs_out may not alias keys8.  The checker's rule (1)
 *                 reads bit 0 of the byte, its rule (4) keeps the extent of 8.
 *   est_in/est_out  tables of AVR_EST_KEYS8 = 128 byte pairs in the dense numbering
 *   workspace     resolver: align256(4 n_slices) + align256(4 n_groups) + 2 ceil(total_chunks / 16) * 768
 *                 checker:  align256(4 n_slices) + 2 ceil(total_chunks / 16) * 512, never above the resolver's
 * The checker gives a slice whose rec_off is not a multiple of 16, if it takes part, a finding at bin 0 and reads nothing of it. */
size_t avr_range_resolve8_workspace_bytes(size_t n_slices, size_t n_groups, const avr_chunk_plan *plan);
int avr_range_resolve8_device(int device, void *stream, const uint8_t *keys8, const uint64_t *rec_off, const uint32_t *n_bins, size_t n_slices,
                              const uint32_t *group_first, size_t n_groups, const uint8_t *est_in, uint8_t *est_out,
                              const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                              uint16_t *recs_out, int32_t *status) AVR_NOWAIT;
size_t avr_range_keys8_verify_workspace_bytes(size_t n_slices, size_t n_groups, const avr_chunk_plan *plan);
int avr_range_keys8_verify_device(int device, void *stream, const uint8_t *keys8, const uint16_t *recs, const uint64_t *rec_off,
                                  const uint32_t *n_bins, size_t n_slices, const uint32_t *group_first, size_t n_groups,
                                  const uint8_t *est_in /* may be NULL */, const uint8_t *est_out /* may be NULL */,
                                  const avr_chunk_plan *plan, void *workspace, size_t workspace_bytes,
                                  int32_t *status, uint32_t *first_bad) AVR_NOWAIT;

/* ------------------------------------------------------------------ dense context ids
 * A context is identified by the offset of its state byte in libavcodec's cabac_state[1024]
 * (recode.cpp:325 keys the model on the address), but a stream uses far fewer of them, and K1
 * keeps 64 lanes x n_states state bytes in LDS per wave: renumbering a batch onto the contexts it
 * uses raises occupancy.  EVERY K1 ENTRY POINT ABOVE DOES THIS BY ITSELF, inside the call (census kernel,
 * look-up on load): records and states go in under the caller's numbering and nothing has to be prepared.
 * The three calls below are the same steps as separate passes, for a caller that wants a renumbered copy of
 * its records for its own purposes; no path of this library needs them.  recs is any flat array of CABAC
 * records on the device (a tile buffer or a slice-major buffer), n_records a multiple of 8.
 *   avr_context_census_device   bitmap[32] |= one bit per selector < 1024 that occurs (zero it first)
 *   avr_context_remap_device    selector s < 1024 -> table[s] in place (table: 1024 x uint16 on the device)
 *   avr_states_permute_device   gather (scatter = 0): dst[slice][j] = src[slice][index[j]], j < n_index,
 *                               or scatter back (1): dst[slice][index[j]] = src[slice][j]
 * The caller builds table / index from the bitmap (128 bytes, host side). */
int avr_context_census_device(int device, void *stream, const uint16_t *recs, uint64_t n_records, uint32_t *bitmap);
int avr_context_remap_device(int device, void *stream, uint16_t *recs, uint64_t n_records, const uint16_t *table);
int avr_states_permute_device(int device, void *stream, const uint8_t *src, size_t n_src, uint8_t *dst, size_t n_dst,
                              const uint16_t *index, size_t n_index, size_t n_slices, int scatter);

/* ------------------------------------------------------------------ synthetic bin streams
 * Seeded generators for the BASELINE.json configurations; the same code
 * runs on the host (avr_synth_*_host) and on the device so that CPU checks and GPU runs see
 * identical records.  `workload`: 2 = 1080p30 slices, 3 = ragged "directory of files",
 * 4 = 4K60 8 slices/frame, 5 = residual-only roofline stress.  `scale_permille` scales the
 * per-slice length (1000 = the configuration's own size) so tests can run small cases.
 * Slice i of a run is generated from (seed, first_slice + i) alone, which is what lets ranks
 * shard a workload without exchanging anything. */
typedef struct {
    int      workload;
    uint32_t scale_permille;
    uint64_t seed;
    uint64_t first_slice;
    uint32_t n_states;       /* out: state bytes per slice this workload declares */
} avr_synth_config;

int avr_synth_config_init(avr_synth_config *cfg, int workload, uint32_t scale_permille,
                          uint64_t first_slice);
/* number of records slice i will have (host; cheap closed loop over the generator) */
int avr_synth_count_host(const avr_synth_config *cfg, int kind, size_t n_slices, uint32_t *n_bins);
int avr_synth_generate_host(const avr_synth_config *cfg, int kind, size_t n_slices,
                            const uint64_t *rec_off, uint16_t *recs, uint8_t *init_states);
int avr_synth_count_device(int device, void *stream, const avr_synth_config *cfg, int kind,
                           size_t n_slices, uint32_t *n_bins);
/* slice-major: slice i at recs + rec_off[i], rec_off multiples of 8, chunk padding = no-op records */
int avr_synth_generate_slices_device(int device, void *stream, const avr_synth_config *cfg, int kind,
                                     size_t n_slices, const uint64_t *rec_off, uint16_t *recs,
                                     uint8_t *init_states);
/* writes straight into the tile layout */
int avr_synth_generate_tiles_device(int device, void *stream, const avr_synth_config *cfg, int kind,
                                    size_t n_slices, const uint32_t *order,
                                    const uint64_t *tile_off, void *tiles, uint8_t *init_states);

/* ------------------------------------------------------------------ host epilogue helpers
 * decompressor::cabac_decoder::finish (recode.cpp:1508-1512): length after dropping a
 * trailing 0x80; decompressor::run tail patch (recode.cpp:1354-1360): buf must have room for
 * len+1 bytes; length_parity -1 = "no patch recorded". */
size_t avr_drop_stop_byte(const uint8_t *buf, size_t len);
size_t avr_tail_patch(uint8_t *buf, size_t len, int length_parity, uint8_t last_byte);

#ifdef __cplusplus
}
#endif
#endif /* AVRECODE_MS_AMD_H */
