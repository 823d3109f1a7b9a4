// avr_multi: one batch over several GPUs (include/avrecode_ms_amd.h, "one batch over several GPUs").
//
// The layer that shards, and nothing else: it keeps the caller's slices, groups and expectations on the host, places them by units
// (avr_multi.h) at avr_multi_submit, and drives one avr_batch per entry of the device list through the PUBLIC batch calls alone -- no
// HIP, no kernel, nothing of avr_api.cpp's insides.  So it links against the CPU stand-in for the batch calls as well
// (tests/cpu_batch.cpp, tests/multi_check.cpp), which is how its bookkeeping and its threads run under the sanitizers.
//
// THE RULE it is held to: for any sequence of calls, slice by slice and group by group, an avr_multi over any device list gives what
// one avr_batch on devices[0] given the same calls gives -- bytes, lengths, statuses, final states, every check's answer, every
// group's table afterwards.  Which entry coded a slice, and which path its sub-batch chose for its share, show in none of these.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/avrecode_ms_amd.h"
#include "avr_multi.h"

namespace {

int fail(int code, const char *fmt, ...) {
    char text[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    return avr::multi_set_error(code, text);
}

constexpr size_t kEstTable = size_t(AVR_EST_KEYS) * 2;           // bytes of one table of estimators

// open: takes slices; in flight: between submit and wait; ran: the getters answer; failed: an entry's add, submit or wait failed
enum class State { open, in_flight, ran, failed };

}  // namespace

struct avr_multi {
    std::vector<int> devices;
    size_t max_slices = 0, max_bins = 0, total_bins = 0;
    int kind = -1;                           // as the caller's call names it (AVR_KIND_CABAC8 and AVR_KIND_RANGE_KEYS included)
    size_t n_states = 0;
    State state = State::open;
    bool verify = false, verify_k1 = false;  // the two settings: kept over avr_multi_reset, applied to every sub-batch at submit
    std::vector<uint8_t> store;              // the slices' records / codes, back to back (bytes)
    std::vector<uint64_t> off;               // n+1 byte offsets into store
    std::vector<uint32_t> n_bins;
    std::vector<uint8_t> states;             // n x n_states
    // key records: the groups (first slice of each) and their start tables, copied at avr_multi_begin_group ({1, 1} for a fresh one)
    std::vector<uint32_t> group_first;
    std::vector<uint8_t> est_in, est_given;
    // the restore check's expectations, copied at avr_multi_expect
    std::vector<uint8_t> expect_store;
    std::vector<uint64_t> expect_off;        // per slice, once any slice has one
    std::vector<uint32_t> expect_len;        // AVR_EXPECT_NONE: none
    // one sub-batch per entry of devices, kept from run to run with the capacity it was created with
    std::vector<avr_batch *> sub;
    std::vector<size_t> cap_slices, cap_bins;
    int created = 0;
    // the last placement
    std::vector<uint8_t> used;               // per entry: it got a slice
    std::vector<int> place, local;           // slice -> entry of devices, index inside that sub-batch
    std::vector<int> group_entry, group_local;   // group -> entry (-1: a group without slices), index inside that sub-batch
    std::vector<uint64_t> load;
};

namespace {

bool is_k1(int kind) { return kind == AVR_KIND_CABAC || kind == AVR_KIND_CABAC8 || kind == AVR_KIND_CABAC_CODES; }
bool is_k2(int kind) { return kind == AVR_KIND_RANGE || kind == AVR_KIND_RANGE_KEYS; }

// The refusals the entry points open with.  check_idle: for what changes the object between runs; check_open: for what adds to a
// run that has not started; check_ran: for the getters.
int check_idle(const avr_multi *m) {
    if (!m) return fail(AVR_ERR_INVALID, "null batch");
    if (m->state == State::in_flight) return fail(AVR_ERR_INVALID, "batch is in flight; call avr_multi_wait first");
    return AVR_OK;
}
int check_open(const avr_multi *m) {
    if (int rc = check_idle(m)) return rc;
    if (m->state == State::ran) return fail(AVR_ERR_INVALID, "batch already ran");
    if (m->state == State::failed) return fail(AVR_ERR_INVALID, "a run of this batch failed; call avr_multi_reset first");
    return AVR_OK;
}
int check_ran(const avr_multi *m, bool more = true) {
    if (!m || m->state != State::ran || !more) return fail(AVR_ERR_INVALID, "batch has not run");
    return AVR_OK;
}
int check_slice(const avr_multi *m, size_t slice) {
    if (int rc = check_ran(m)) return rc;
    if (slice >= m->n_bins.size()) return fail(AVR_ERR_INVALID, "slice %zu out of range", slice);
    return AVR_OK;
}
int check_entry(const avr_multi *m, size_t entry, bool more) {
    if (int rc = check_ran(m, more)) return rc;
    if (entry >= m->devices.size()) return fail(AVR_ERR_INVALID, "device entry %zu out of range", entry);
    return AVR_OK;
}

int multi_add(avr_multi *m, int kind, const void *data, size_t n, size_t elem, const uint8_t *init_states, size_t n_states) {
    if (!m) return fail(AVR_ERR_INVALID, "null batch");
    if (!data && n) return fail(AVR_ERR_INVALID, "null records");
    if (int rc = check_open(m)) return rc;
    if ((m->kind >= 0 && m->kind != kind) || (kind != AVR_KIND_RANGE_KEYS && !m->group_first.empty()))
        return fail(AVR_ERR_INVALID, "a batch holds slices of one kind only");
    if (n > 0xfffffff0u) return fail(AVR_ERR_INVALID, "slice too long");
    if (m->n_bins.size() >= m->max_slices) return fail(AVR_ERR_CAPACITY, "batch holds max_slices=%zu slices", m->max_slices);
    if (m->total_bins + n > m->max_bins) return fail(AVR_ERR_CAPACITY, "batch holds max_bins=%zu records", m->max_bins);
    if (kind == AVR_KIND_RANGE_KEYS && m->group_first.empty()) {                 // no group begun: a fresh one
        if (int rc = avr_multi_begin_group(m, nullptr); rc < 0) return rc;
    }
    if (kind == AVR_KIND_CABAC || kind == AVR_KIND_CABAC8) {
        if (n_states > AVR_MAX_STATES) return fail(AVR_ERR_INVALID, "n_states %zu > %d", n_states, AVR_MAX_STATES);
        if (!init_states && n_states) return fail(AVR_ERR_INVALID, "null init_states");
        if (!m->n_bins.empty() && n_states != m->n_states) return fail(AVR_ERR_INVALID, "all slices of a batch use the same n_states");
        m->n_states = n_states;
        m->states.insert(m->states.end(), init_states, init_states + n_states);
    }
    const uint8_t *p = static_cast<const uint8_t *>(data);
    m->store.insert(m->store.end(), p, p + n * elem);
    m->off.push_back(m->store.size());
    m->n_bins.push_back(uint32_t(n));
    m->total_bins += n;
    m->kind = kind;
    return int(m->n_bins.size()) - 1;
}

// One entry's share of a run: which slices, in the caller's order, and the room they need of a sub-batch.
struct Share {
    std::vector<uint32_t> slices;
    size_t bins = 0;
};

// The entry's sub-batch, empty: the one it has where the capacity it was created with covers the share, else a new one that covers
// the larger of the two, *made = 1 with it.  (A sub-batch that a failed run left in a state avr_batch_reset refuses is replaced as well.)
int take_sub(avr_multi *m, size_t e, const Share &s, uint8_t *made) {
    const size_t need_slices = s.slices.size(), need_bins = s.bins + 8;
    if (m->sub[e] && m->cap_slices[e] >= need_slices && m->cap_bins[e] >= need_bins && avr_batch_reset(m->sub[e]) == AVR_OK) return AVR_OK;
    const size_t slices = m->sub[e] ? std::max(m->cap_slices[e], need_slices) : need_slices;
    const size_t bins = m->sub[e] ? std::max(m->cap_bins[e], need_bins) : need_bins;
    if (m->sub[e]) { avr_batch_destroy(m->sub[e]); m->sub[e] = nullptr; }
    avr_batch *b = avr_batch_create(m->devices[e], slices, bins);
    if (!b) return AVR_ERR_HIP;
    *made = 1;
    m->sub[e] = b;
    m->cap_slices[e] = slices;
    m->cap_bins[e] = bins;
    return AVR_OK;
}

// Fill the entry's sub-batch with its share -- settings, groups, slices, expectations -- and submit it.
int fill_and_submit(avr_multi *m, size_t e, const Share &s) {
    avr_batch *b = m->sub[e];
    int rc;
    if ((rc = avr_batch_set_verify(b, m->verify)) < 0 || (rc = avr_batch_set_verify_k1(b, m->verify_k1)) < 0) return rc;
    size_t next_group = 0;                                       // the first of the caller's groups not yet looked at
    for (size_t j = 0; j < s.slices.size(); j++) {
        const uint32_t i = s.slices[j];
        const uint8_t *p = m->store.data() + m->off[i];
        const uint8_t *st = m->states.data() + size_t(i) * m->n_states;
        if (m->kind == AVR_KIND_RANGE_KEYS) {
            // the entry's groups in the caller's order: a group is begun where its first slice comes up (all its slices are here)
            for (; next_group < m->group_first.size() && m->group_first[next_group] <= i; next_group++) {
                if (m->group_entry[next_group] != int(e)) continue;
                rc = avr_batch_begin_group(b, m->est_given[next_group] ? m->est_in.data() + next_group * kEstTable : nullptr);
                if (rc < 0) return rc;
                m->group_local[next_group] = rc;
            }
            rc = avr_batch_add_slice_range_keys(b, reinterpret_cast<const uint16_t *>(p), m->n_bins[i]);
        } else if (m->kind == AVR_KIND_CABAC) rc = avr_batch_add_slice_cabac(b, reinterpret_cast<const uint16_t *>(p), m->n_bins[i], st, m->n_states);
        else if (m->kind == AVR_KIND_CABAC8) rc = avr_batch_add_slice_cabac8(b, p, m->n_bins[i], st, m->n_states);
        else if (m->kind == AVR_KIND_RANGE) rc = avr_batch_add_slice_range(b, reinterpret_cast<const uint16_t *>(p), m->n_bins[i]);
        else rc = avr_batch_add_slice_codes(b, p, m->n_bins[i]);
        if (rc < 0) return rc;
        m->local[i] = rc;
        if (i < m->expect_len.size() && m->expect_len[i] != AVR_EXPECT_NONE) {
            const uint8_t *bytes = m->expect_len[i] ? m->expect_store.data() + m->expect_off[i] : nullptr;
            if ((rc = avr_batch_expect(b, size_t(m->local[i]), bytes, m->expect_len[i])) < 0) return rc;
        }
    }
    return avr_batch_submit(b);
}

// fn(e) for every entry that has a share, each from a host thread of its own (the first on the caller's); the error text is per
// thread, so a worker's is carried over.  Returns the first failing entry, or the number of entries.
template <class F>
size_t for_each_used(avr_multi *m, std::vector<int> &rc, std::vector<std::string> &err, F fn) {
    const size_t nd = m->devices.size();
    rc.assign(nd, AVR_OK);
    err.assign(nd, std::string());
    auto work = [&](size_t e) {
        if ((rc[e] = fn(e)) < 0) err[e] = avr_last_error();
    };
    std::vector<size_t> todo;
    for (size_t e = 0; e < nd; e++)
        if (m->used[e]) todo.push_back(e);
    std::vector<std::thread> threads;
    for (size_t k = 1; k < todo.size(); k++) threads.emplace_back(work, todo[k]);
    if (!todo.empty()) work(todo[0]);
    for (std::thread &t : threads) t.join();
    for (size_t e = 0; e < nd; e++)
        if (rc[e] < 0) return e;
    return nd;
}

int entry_failed(avr_multi *m, size_t e, int rc, const std::string &err) {
    m->state = State::failed;
    return fail(rc, "device entry %zu (device %d): %s", e, m->devices[e], err.c_str());
}

}  // namespace

extern "C" {

avr_multi *avr_multi_create(const int *devices, size_t n_devices, size_t max_slices, size_t max_bins) {
    if (!devices || n_devices == 0 || n_devices > 64) { fail(AVR_ERR_INVALID, "need 1..64 devices"); return nullptr; }
    if (max_slices == 0 || max_slices > 0x7fffffffu) { fail(AVR_ERR_INVALID, "max_slices out of range"); return nullptr; }
    for (size_t i = 0; i < n_devices; i++)
        if (avr::multi_check_device(devices[i]) != AVR_OK) return nullptr;
    avr_multi *m = new (std::nothrow) avr_multi;
    if (!m) { fail(AVR_ERR_NOMEM, "out of host memory"); return nullptr; }
    m->devices.assign(devices, devices + n_devices);
    m->max_slices = max_slices;
    m->max_bins = max_bins;
    m->off.push_back(0);
    m->sub.assign(n_devices, nullptr);
    m->cap_slices.assign(n_devices, 0);
    m->cap_bins.assign(n_devices, 0);
    m->used.assign(n_devices, 0);
    return m;
}

void avr_multi_destroy(avr_multi *m) {
    if (!m) return;
    for (avr_batch *b : m->sub) avr_batch_destroy(b);           // (a sub-batch in flight is drained by its own destructor)
    delete m;
}

int avr_multi_reset(avr_multi *m) {
    if (int rc = check_idle(m)) return rc;
    m->kind = -1; m->n_states = 0; m->total_bins = 0; m->state = State::open;
    m->store.clear(); m->off.assign(1, 0); m->n_bins.clear(); m->states.clear();
    m->group_first.clear(); m->est_in.clear(); m->est_given.clear();
    m->expect_store.clear(); m->expect_off.clear(); m->expect_len.clear();
    m->place.clear(); m->local.clear(); m->group_entry.clear(); m->group_local.clear(); m->load.clear();
    std::fill(m->used.begin(), m->used.end(), uint8_t(0));
    return AVR_OK;
}

int avr_multi_created(avr_multi *m) {
    if (!m) return fail(AVR_ERR_INVALID, "null batch");
    return m->created;
}

int avr_multi_add_slice_cabac(avr_multi *m, const uint16_t *recs, size_t n, const uint8_t *init_states, size_t n_states) {
    return multi_add(m, AVR_KIND_CABAC, recs, n, 2, init_states, n_states);
}
int avr_multi_add_slice_range(avr_multi *m, const uint16_t *recs, size_t n) { return multi_add(m, AVR_KIND_RANGE, recs, n, 2, nullptr, 0); }
int avr_multi_add_slice_codes(avr_multi *m, const uint8_t *codes, size_t n) { return multi_add(m, AVR_KIND_CABAC_CODES, codes, n, 1, nullptr, 0); }
int avr_multi_add_slice_cabac8(avr_multi *m, const uint8_t *recs8, size_t n, const uint8_t *init_states, size_t n_states) {
    if (n_states > AVR_MAX_STATES8)                              // (first: what needs no batch is checked without one)
        return fail(AVR_ERR_INVALID, "n_states %zu > %d: one-byte records name at most %d contexts", n_states, AVR_MAX_STATES8, AVR_MAX_STATES8);
    return multi_add(m, AVR_KIND_CABAC8, recs8, n, 1, init_states, n_states);
}
int avr_multi_add_slice_range_keys(avr_multi *m, const uint16_t *recs, size_t n) { return multi_add(m, AVR_KIND_RANGE_KEYS, recs, n, 2, nullptr, 0); }

int avr_multi_begin_group(avr_multi *m, const uint8_t *est_in) {
    if (int rc = check_open(m)) return rc;
    if (m->kind >= 0 && m->kind != AVR_KIND_RANGE_KEYS) return fail(AVR_ERR_INVALID, "a batch holds slices of one kind only: groups belong to key records");
    if (m->group_first.size() >= m->max_slices) return fail(AVR_ERR_CAPACITY, "batch holds max_slices=%zu groups", m->max_slices);
    for (size_t k = 0; est_in && k < AVR_EST_KEYS; k++) {
        const unsigned pos = est_in[2 * k], neg = est_in[2 * k + 1];
        if (pos < 1 || neg < 1 || pos + neg > 0x60)
            return fail(AVR_ERR_INVALID, "start table entry %zu = {%u, %u}: need pos >= 1, neg >= 1, pos + neg <= 0x60", k, pos, neg);
    }
    const size_t g = m->group_first.size();
    m->est_in.resize((g + 1) * kEstTable);
    uint8_t *dst = m->est_in.data() + g * kEstTable;
    if (est_in) memcpy(dst, est_in, kEstTable); else memset(dst, 1, kEstTable);      // fresh: {1, 1}
    m->est_given.push_back(est_in != nullptr);
    m->group_first.push_back(uint32_t(m->n_bins.size()));
    return int(g);
}

int avr_multi_set_verify(avr_multi *m, int on) {
    if (int rc = check_idle(m)) return rc;
    if (m->state == State::failed) return fail(AVR_ERR_INVALID, "a run of this batch failed; call avr_multi_reset first");
    m->verify = on != 0;
    return AVR_OK;
}

int avr_multi_set_verify_k1(avr_multi *m, int on) {
    if (int rc = check_idle(m)) return rc;
    if (m->state == State::failed) return fail(AVR_ERR_INVALID, "a run of this batch failed; call avr_multi_reset first");
    m->verify_k1 = on != 0;
    return AVR_OK;
}

int avr_multi_expect(avr_multi *m, size_t slice, const uint8_t *bytes, size_t len) {
    if (int rc = check_open(m)) return rc;
    if (is_k2(m->kind)) return fail(AVR_ERR_INVALID, "the restore check exists for K1 batches only: not for a K2 batch");
    if (slice >= m->n_bins.size()) return fail(AVR_ERR_INVALID, "slice %zu has not been added", slice);
    if (len >= 0xffffffffull) return fail(AVR_ERR_INVALID, "expectation too long");
    if (!bytes && len) return fail(AVR_ERR_INVALID, "null bytes");
    if (slice < m->expect_len.size() && m->expect_len[slice] != AVR_EXPECT_NONE)
        return fail(AVR_ERR_INVALID, "slice %zu has an expectation already", slice);
    m->expect_off.resize(m->n_bins.size(), 0);
    m->expect_len.resize(m->n_bins.size(), AVR_EXPECT_NONE);
    m->expect_off[slice] = m->expect_store.size();
    m->expect_len[slice] = uint32_t(len);
    if (len) m->expect_store.insert(m->expect_store.end(), bytes, bytes + len);
    return AVR_OK;
}

int avr_multi_submit(avr_multi *m) {
    if (int rc = check_open(m)) return rc;
    // the wrong direction is the multi's own refusal, in front of every sub-batch: the object stays as it was
    if (m->verify && is_k1(m->kind)) return fail(AVR_ERR_INVALID, "verification exists for the compress direction only: not for a K1 batch");
    if (m->verify_k1 && is_k2(m->kind)) return fail(AVR_ERR_INVALID, "K1 verification exists for the decompress direction only: not for a K2 batch");
    const size_t n = m->n_bins.size(), nd = m->devices.size(), ng = m->group_first.size();
    const bool keys = m->kind == AVR_KIND_RANGE_KEYS;
    m->place.assign(n, 0);
    m->local.assign(n, 0);
    m->load.assign(nd, 0);
    avr::multi_place(m->n_bins.data(), n, keys ? m->group_first.data() : nullptr, ng, nd, m->place.data(), m->load.data());
    m->group_entry.assign(ng, -1);
    m->group_local.assign(ng, -1);
    for (size_t g = 0; g < ng; g++) {
        const size_t first = m->group_first[g], last = g + 1 < ng ? m->group_first[g + 1] : n;
        if (first < last) m->group_entry[g] = m->place[first];
    }
    std::vector<Share> share(nd);
    for (size_t i = 0; i < n; i++) {                             // index order: each entry keeps the caller's order
        Share &s = share[size_t(m->place[i])];
        s.slices.push_back(uint32_t(i));
        s.bins += m->n_bins[i];
    }
    for (size_t e = 0; e < nd; e++) m->used[e] = !share[e].slices.empty();
    std::vector<int> rc;
    std::vector<std::string> err;
    std::vector<uint8_t> submitted(nd, 0), made(nd, 0);
    const size_t bad = for_each_used(m, rc, err, [&](size_t e) {
        int r = take_sub(m, e, share[e], &made[e]);
        if (r == AVR_OK && (r = fill_and_submit(m, e, share[e])) == AVR_OK) submitted[e] = 1;
        return r;
    });
    for (size_t e = 0; e < nd; e++) m->created += made[e];
    if (bad < nd) {                                              // nothing stays in flight behind a failure
        for (size_t e = 0; e < nd; e++)
            if (submitted[e]) (void)avr_batch_wait(m->sub[e]);
        return entry_failed(m, bad, rc[bad], err[bad]);
    }
    m->state = State::in_flight;
    return AVR_OK;
}

int avr_multi_wait(avr_multi *m) {
    if (!m) return fail(AVR_ERR_INVALID, "null batch");
    if (m->state != State::in_flight) return fail(AVR_ERR_INVALID, "batch has not been submitted");
    std::vector<int> rc;
    std::vector<std::string> err;
    // from threads: a wait may run a sub-batch's second pass.  Every entry is waited for, whatever another one's wait returns.
    const size_t bad = for_each_used(m, rc, err, [&](size_t e) { return avr_batch_wait(m->sub[e]); });
    if (bad < m->devices.size()) return entry_failed(m, bad, rc[bad], err[bad]);
    m->state = State::ran;
    return AVR_OK;
}

int avr_multi_run(avr_multi *m) {
    if (int rc = avr_multi_submit(m)) return rc;
    return avr_multi_wait(m);
}

int avr_multi_get(avr_multi *m, size_t slice, const uint8_t **bytes, size_t *len, int *status) {
    if (int rc = check_slice(m, slice)) return rc;
    return avr_batch_get(m->sub[size_t(m->place[slice])], size_t(m->local[slice]), bytes, len, status);
}

int avr_multi_get_states(avr_multi *m, size_t slice, const uint8_t **states, size_t *n_states) {
    if (int rc = check_slice(m, slice)) return rc;
    return avr_batch_get_states(m->sub[size_t(m->place[slice])], size_t(m->local[slice]), states, n_states);
}

int avr_multi_get_verify(avr_multi *m, size_t slice, uint32_t *first_bad) {
    if (int rc = check_slice(m, slice)) return rc;
    return avr_batch_get_verify(m->sub[size_t(m->place[slice])], size_t(m->local[slice]), first_bad);
}

int avr_multi_get_verify_est(avr_multi *m, size_t slice, uint32_t *first_bad) {
    if (int rc = check_slice(m, slice)) return rc;
    return avr_batch_get_verify_est(m->sub[size_t(m->place[slice])], size_t(m->local[slice]), first_bad);
}

int avr_multi_get_restore(avr_multi *m, size_t slice, uint32_t *first_diff) {
    if (int rc = check_slice(m, slice)) return rc;
    return avr_batch_get_restore(m->sub[size_t(m->place[slice])], size_t(m->local[slice]), first_diff);
}

int avr_multi_get_estimators(avr_multi *m, size_t group, const uint8_t **pos_neg, size_t *n_keys) {
    if (int rc = check_ran(m)) return rc;
    if (m->kind != AVR_KIND_RANGE_KEYS) return fail(AVR_ERR_INVALID, "not a batch of key records");
    if (group >= m->group_first.size()) return fail(AVR_ERR_INVALID, "group %zu out of range", group);
    if (m->group_entry[group] >= 0)
        return avr_batch_get_estimators(m->sub[size_t(m->group_entry[group])], size_t(m->group_local[group]), pos_neg, n_keys);
    if (pos_neg) *pos_neg = m->est_in.data() + group * kEstTable;     // a group without slices went to no device: its start table
    if (n_keys) *n_keys = AVR_EST_KEYS;
    return AVR_OK;
}

int avr_multi_placement(avr_multi *m, size_t slice) {
    if (int rc = check_slice(m, slice)) return rc;
    return m->place[slice];
}

int avr_multi_load(avr_multi *m, uint64_t *bins_per_device) {
    if (int rc = check_ran(m, bins_per_device != nullptr)) return rc;
    for (size_t d = 0; d < m->load.size(); d++) bins_per_device[d] = m->load[d];
    return AVR_OK;
}

int avr_multi_entry_info(avr_multi *m, size_t entry, uint32_t info[4]) {
    if (int rc = check_entry(m, entry, info != nullptr)) return rc;
    memset(info, 0, 4 * sizeof(uint32_t));
    return m->used[entry] ? avr_batch_run_info(m->sub[entry], info) : AVR_OK;
}

int avr_multi_entry_ms(avr_multi *m, size_t entry, float ms[7]) {
    if (int rc = check_entry(m, entry, ms != nullptr)) return rc;
    for (int i = 0; i < 7; i++) ms[i] = 0;
    if (!m->used[entry]) return AVR_OK;
    avr_batch *b = m->sub[entry];
    int rc;
    if ((rc = avr_batch_timings(b, ms)) < 0 || (rc = avr_batch_verify_ms(b, ms + 4)) < 0 || (rc = avr_batch_verify_est_ms(b, ms + 5)) < 0) return rc;
    return avr_batch_restore_ms(b, ms + 6);
}

}  // extern "C"
