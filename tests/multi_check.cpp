// TEST INFRASTRUCTURE: avr_multi (csrc/avr_multi.cpp) on the CPU stand-in for the batch calls (tests/cpu_batch.cpp, as it stands, coded
// by oracle/), as a stand-alone program that tests/test_multi_cpu.py builds and runs under ASan + UBSan and under ThreadSanitizer.
//
// What the stand-in lacks for this is supplied here: avr_batch_submit / avr_batch_wait as run / no-op, the calls of kinds the stand-in
// does not code (two-byte and one-byte CABAC records: refused; run info and timings: zeros), and the two seams of csrc/avr_multi.h --
// the multi's error text is kept here, per thread (g_multi_error).
//
//   multi_check rule     an avr_multi over 1, 3 and 4 entries and ONE stand-in avr_batch are given the same calls, and everything in
//                        the equivalence rule is compared: bytes, lengths, statuses, first_bad of the verifier and of the estimator
//                        checker, first_diff of the restore check, every group's table.  One multi object per entry count goes through
//                        range records, codes, key records in seven groups (two started from tables, one with a malformed key in its
//                        second slice, one empty), both verify switches, expectations right / short / long / differing, the
//                        wrong-direction refusal, submit / wait and their refusals, a failing entry, with avr_multi_reset between all
//                        of these, and created() is held to the reuse rule.
//   multi_check fault    AVR_CPU_BATCH_FAULT names verify_flip=K, est_flip=K (with est_flip_bin=M) or restore_flip=K.  The stand-in's
//                        fault points address each (sub-)batch's own slice K - 1, so the program works out from avr_multi_placement
//                        which of the caller's slices that is for every entry, builds ONE stand-in batch per entry holding that
//                        entry's slices (and groups), and holds the multi to it: those slices, and only those, come back
//                        AVR_SLICE_VERIFY_FAILED with that batch's first_bad / first_diff.
// Exit status 0 and "multi_check ok: ..." on stdout, or 1 with the first difference on stderr.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/avrecode_ms_amd.h"
#include "../oracle/avr_oracle.h"
#include "../avrecode-ms_amd/csrc/avr_multi.h"

// ------------------------------------------------------------------ what the stand-in lacks

namespace {
thread_local std::string g_multi_error;
std::atomic<int> g_fail_submits{0};          // that many avr_batch_submit calls from now on fail
std::atomic<int> g_waits{0}, g_submits{0};
}  // namespace

namespace avr {
int multi_set_error(int code, const char *text) { g_multi_error = text; return code; }
int multi_check_device(int device) { return device >= 0 && device < 8 ? AVR_OK : multi_set_error(AVR_ERR_INVALID, "device out of range (0..7)"); }
}  // namespace avr

extern "C" {
int avr_batch_submit(avr_batch *b) {
    g_submits++;
    int left = g_fail_submits.load();
    while (left > 0 && !g_fail_submits.compare_exchange_weak(left, left - 1)) {}
    if (left > 0) return AVR_ERR_HIP;
    return avr_batch_run(b);
}
int avr_batch_wait(avr_batch *b) { g_waits++; return b ? AVR_OK : AVR_ERR_INVALID; }
int avr_batch_add_slice_cabac(avr_batch *, const uint16_t *, size_t, const uint8_t *, size_t) { return AVR_ERR_INVALID; }
int avr_batch_add_slice_cabac8(avr_batch *, const uint8_t *, size_t, const uint8_t *, size_t) { return AVR_ERR_INVALID; }
int avr_batch_get_states(avr_batch *, size_t, const uint8_t **, size_t *) { return AVR_ERR_INVALID; }
int avr_batch_run_info(avr_batch *b, uint32_t info[4]) { if (!b || !info) return AVR_ERR_INVALID; memset(info, 0, 4 * sizeof(uint32_t)); return AVR_OK; }
int avr_batch_timings(avr_batch *b, float ms[4]) { if (!b || !ms) return AVR_ERR_INVALID; for (int i = 0; i < 4; i++) ms[i] = 0; return AVR_OK; }
}

// ------------------------------------------------------------------ the checks' plumbing

namespace {

[[noreturn]] void die(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "multi_check: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) die(__VA_ARGS__); } while (0)

struct Rng {                                                     // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    uint32_t below(uint32_t n) { return uint32_t(next() % n); }
};

using Recs = std::vector<uint16_t>;
using Bytes = std::vector<uint8_t>;

Recs range_records(Rng &r, size_t n) {
    Recs v(n);
    for (uint16_t &x : v) x = uint16_t(r.below(2) | (1 + r.below(47)) << 1 | (1 + r.below(47)) << 8);
    return v;
}
Recs key_records(Rng &r, size_t n) {
    Recs v(n);
    for (uint16_t &x : v) {
        const uint32_t pick = r.below(40);
        const uint32_t key = pick == 0 ? AVR_SEL_BYPASS : pick == 1 ? AVR_SEL_TERMINATE : r.below(24);
        x = uint16_t(r.below(4) != 0 ? 1 | key << 1 : key << 1);     // skewed bins: the estimators move
    }
    return v;
}
Bytes codes(Rng &r, size_t n) {
    Bytes v(n);
    for (uint8_t &x : v) x = uint8_t(r.below(16) ? r.below(252) : r.below(8) ? 252 + r.below(2) : AVR_CODE_TERMINATE(0));
    if (n && r.below(2)) v.back() = AVR_CODE_TERMINATE(1);
    return v;
}
Bytes table(Rng &r) {
    Bytes t(size_t(AVR_EST_KEYS) * 2);
    for (uint8_t &x : t) x = uint8_t(1 + r.below(47));
    return t;
}
std::vector<size_t> lengths(Rng &r, size_t n, size_t lo, size_t hi) {
    std::vector<size_t> v(n);
    for (size_t &x : v) x = lo + r.below(uint32_t(hi - lo + 1));
    return v;
}

// A batch as the caller describes it: the calls, in order, that the multi and the single batch are both given.
struct Group { size_t first; bool given; Bytes est; };
struct Expect { size_t slice; Bytes bytes; };
struct Desc {
    int kind = -1;
    std::vector<Recs> recs;                                      // range or key records
    std::vector<Bytes> code;                                     // codes
    std::vector<Group> groups;                                   // key records: begun in front of slice `first`
    std::vector<Expect> expects;
    int bad_group = -1;                                          // the group with a malformed record: its table is undefined
    size_t size() const { return kind == AVR_KIND_CABAC_CODES ? code.size() : recs.size(); }
    size_t bins(size_t i) const { return kind == AVR_KIND_CABAC_CODES ? code[i].size() : recs[i].size(); }
};

// The same calls to either object.  `only`: the slices to give (a share of the batch), all where null; groups that have none of them
// are left out, as the multi leaves them out of a sub-batch.
template <class T> struct Calls;
template <> struct Calls<avr_batch> {
    static int begin(avr_batch *b, const uint8_t *e) { return avr_batch_begin_group(b, e); }
    static int keys(avr_batch *b, const Recs &r) { return avr_batch_add_slice_range_keys(b, r.data(), r.size()); }
    static int range(avr_batch *b, const Recs &r) { return avr_batch_add_slice_range(b, r.data(), r.size()); }
    static int code(avr_batch *b, const Bytes &c) { return avr_batch_add_slice_codes(b, c.data(), c.size()); }
    static int expect(avr_batch *b, size_t i, const Bytes &x) { return avr_batch_expect(b, i, x.data(), x.size()); }
};
template <> struct Calls<avr_multi> {
    static int begin(avr_multi *m, const uint8_t *e) { return avr_multi_begin_group(m, e); }
    static int keys(avr_multi *m, const Recs &r) { return avr_multi_add_slice_range_keys(m, r.data(), r.size()); }
    static int range(avr_multi *m, const Recs &r) { return avr_multi_add_slice_range(m, r.data(), r.size()); }
    static int code(avr_multi *m, const Bytes &c) { return avr_multi_add_slice_codes(m, c.data(), c.size()); }
    static int expect(avr_multi *m, size_t i, const Bytes &x) { return avr_multi_expect(m, i, x.data(), x.size()); }
};

template <class T>
void feed(T *t, const Desc &d, const std::vector<size_t> *only = nullptr) {
    const size_t n = d.size();
    std::vector<int> index(n, -1);                               // the caller's slice -> its index in t
    size_t g = 0, k = 0;
    for (size_t i = 0; i <= n; i++) {
        for (; g < d.groups.size() && d.groups[g].first == i; g++) {
            if (only) {                                          // a share holds a group iff it holds its first slice (a group is one unit)
                const size_t last = g + 1 < d.groups.size() ? d.groups[g + 1].first : n;
                if (i >= last || k >= only->size() || (*only)[k] != i) continue;
            }
            const int rc = Calls<T>::begin(t, d.groups[g].given ? d.groups[g].est.data() : nullptr);
            CHECK(rc >= 0, "begin_group %zu: %d", g, rc);
        }
        if (i == n) break;
        if (only) {
            if (k >= only->size() || (*only)[k] != i) continue;
            k++;
        }
        int rc;
        if (d.kind == AVR_KIND_RANGE_KEYS) rc = Calls<T>::keys(t, d.recs[i]);
        else if (d.kind == AVR_KIND_RANGE) rc = Calls<T>::range(t, d.recs[i]);
        else rc = Calls<T>::code(t, d.code[i]);
        CHECK(rc >= 0, "add slice %zu: %d", i, rc);
        index[i] = rc;
    }
    for (const Expect &x : d.expects)
        if (index[x.slice] >= 0) CHECK(Calls<T>::expect(t, size_t(index[x.slice]), x.bytes) == AVR_OK, "expect slice %zu", x.slice);
}

struct Answer {
    Bytes bytes;
    int status = -1;
    uint32_t first_bad = 0, first_bad_est = 0, first_diff = 0;
    bool operator==(const Answer &o) const {
        return bytes == o.bytes && status == o.status && first_bad == o.first_bad && first_bad_est == o.first_bad_est && first_diff == o.first_diff;
    }
};
Answer answer(avr_batch *b, size_t i) {
    Answer a;
    const uint8_t *p = nullptr;
    size_t len = 0;
    CHECK(avr_batch_get(b, i, &p, &len, &a.status) == AVR_OK, "avr_batch_get %zu", i);
    a.bytes.assign(p, p + len);
    CHECK(avr_batch_get_verify(b, i, &a.first_bad) == AVR_OK && avr_batch_get_verify_est(b, i, &a.first_bad_est) == AVR_OK &&
          avr_batch_get_restore(b, i, &a.first_diff) == AVR_OK, "the batch's answers for slice %zu", i);
    return a;
}
Answer answer(avr_multi *m, size_t i) {
    Answer a;
    const uint8_t *p = nullptr;
    size_t len = 0;
    CHECK(avr_multi_get(m, i, &p, &len, &a.status) == AVR_OK, "avr_multi_get %zu: %s", i, g_multi_error.c_str());
    a.bytes.assign(p, p + len);
    CHECK(avr_multi_get_verify(m, i, &a.first_bad) == AVR_OK && avr_multi_get_verify_est(m, i, &a.first_bad_est) == AVR_OK &&
          avr_multi_get_restore(m, i, &a.first_diff) == AVR_OK, "the multi's answers for slice %zu", i);
    return a;
}
void same(const Answer &got, const Answer &want, const char *what, size_t i) {
    CHECK(got == want, "%s: slice %zu differs: status %d / %d, %zu / %zu bytes, first_bad %u / %u, est %u / %u, first_diff %u / %u", what, i, got.status,
          want.status, got.bytes.size(), want.bytes.size(), got.first_bad, want.first_bad, got.first_bad_est, want.first_bad_est, got.first_diff, want.first_diff);
}

Bytes estimators(avr_batch *b, size_t g) {
    const uint8_t *p = nullptr;
    size_t n = 0;
    CHECK(avr_batch_get_estimators(b, g, &p, &n) == AVR_OK && n == AVR_EST_KEYS, "avr_batch_get_estimators %zu", g);
    return Bytes(p, p + 2 * n);
}
Bytes estimators(avr_multi *m, size_t g) {
    const uint8_t *p = nullptr;
    size_t n = 0;
    CHECK(avr_multi_get_estimators(m, g, &p, &n) == AVR_OK && n == AVR_EST_KEYS, "avr_multi_get_estimators %zu: %s", g, g_multi_error.c_str());
    return Bytes(p, p + 2 * n);
}

avr_batch *single(const Desc &d, bool verify, bool verify_k1, const std::vector<size_t> *only = nullptr) {
    avr_batch *b = avr_batch_create(0, d.size() + 1, size_t(1) << 24);
    CHECK(b && avr_batch_set_verify(b, verify) == AVR_OK && avr_batch_set_verify_k1(b, verify_k1) == AVR_OK, "the single batch");
    feed(b, d, only);
    CHECK(avr_batch_run(b) == AVR_OK, "the single batch's run: %s", avr_last_error());
    return b;
}

// The oracle itself, where the kind has no model in between: what the single batch is held to, so the multi through it.
void against_oracle(avr_batch *b, const Desc &d) {
    for (size_t i = 0; i < d.size() && d.kind != AVR_KIND_RANGE_KEYS; i++) {
        Bytes out(d.bins(i) * 2 + 64);
        int status = 0;
        const size_t len = d.kind == AVR_KIND_RANGE ? avr_oracle_range_encode(d.recs[i].data(), d.recs[i].size(), out.data(), out.size(), &status)
                                                    : avr_oracle_cabac_encode_codes(d.code[i].data(), d.code[i].size(), out.data(), out.size(), &status);
        out.resize(status == AVR_ORACLE_OK ? len : 0);
        const Answer a = answer(b, i);
        CHECK(a.bytes == out && (a.status == status || a.status == AVR_SLICE_VERIFY_FAILED), "the stand-in against the oracle, slice %zu", i);
    }
}

// The calls to the multi and its run, in one call or as submit and wait with the refusals in between.
void run_multi(avr_multi *m, const Desc &d, bool split_submit, const char *what) {
    feed(m, d);
    if (split_submit) {
        CHECK(avr_multi_submit(m) == AVR_OK, "%s: submit: %s", what, g_multi_error.c_str());
        const uint8_t *p;
        size_t len;
        int st;
        uint32_t v;
        const Recs one(4, uint16_t(3 << 1 | 3 << 8));
        const Bytes byte(1, 0);
        // between submit and wait nothing but wait (and destroy) is taken, and nothing is disturbed by the asking
        CHECK(avr_multi_add_slice_range(m, one.data(), one.size()) == AVR_ERR_INVALID && avr_multi_add_slice_codes(m, byte.data(), 1) == AVR_ERR_INVALID &&
              avr_multi_add_slice_range_keys(m, one.data(), one.size()) == AVR_ERR_INVALID && avr_multi_begin_group(m, nullptr) == AVR_ERR_INVALID &&
              avr_multi_expect(m, 0, byte.data(), 1) == AVR_ERR_INVALID && avr_multi_reset(m) == AVR_ERR_INVALID &&
              avr_multi_get(m, 0, &p, &len, &st) == AVR_ERR_INVALID && avr_multi_get_verify(m, 0, &v) == AVR_ERR_INVALID &&
              avr_multi_get_restore(m, 0, &v) == AVR_ERR_INVALID && avr_multi_placement(m, 0) == AVR_ERR_INVALID &&
              avr_multi_submit(m) == AVR_ERR_INVALID && avr_multi_set_verify(m, 1) == AVR_ERR_INVALID && avr_multi_set_verify_k1(m, 1) == AVR_ERR_INVALID,
              "%s: a call between submit and wait was taken", what);
        CHECK(g_multi_error.find("in flight") != std::string::npos, "%s: the in-flight message: %s", what, g_multi_error.c_str());
        CHECK(avr_multi_wait(m) == AVR_OK, "%s: wait: %s", what, g_multi_error.c_str());
    } else {
        CHECK(avr_multi_run(m) == AVR_OK, "%s: run: %s", what, g_multi_error.c_str());
    }
    CHECK(avr_multi_submit(m) == AVR_ERR_INVALID && g_multi_error == "batch already ran", "%s: a second submit: %s", what, g_multi_error.c_str());
}

// One run of the multi held to one run of a single batch: every slice, every group.  Returns the findings (slices not AVR_SLICE_OK).
size_t compare(avr_multi *m, avr_batch *b, const Desc &d, const char *what) {
    size_t findings = 0;
    for (size_t i = 0; i < d.size(); i++) {
        const Answer want = answer(b, i);
        same(answer(m, i), want, what, i);
        findings += want.status != AVR_SLICE_OK;
    }
    for (size_t g = 0; g < d.groups.size(); g++) {
        if (int(g) == d.bad_group) continue;
        CHECK(estimators(m, g) == estimators(b, g), "%s: the table of group %zu differs", what, g);
    }
    const uint8_t *p;
    size_t len;
    int st;
    uint32_t v;
    CHECK(avr_multi_get(m, d.size(), &p, &len, &st) == AVR_ERR_INVALID && avr_multi_get_verify(m, d.size(), &v) == AVR_ERR_INVALID &&
          avr_multi_get_restore(m, d.size(), &v) == AVR_ERR_INVALID && avr_multi_placement(m, d.size()) == AVR_ERR_INVALID &&
          avr_multi_get_estimators(m, d.groups.size(), &p, &len) == AVR_ERR_INVALID, "%s: an index out of range was taken", what);
    return findings;
}

// the slices of every entry, in the caller's order, and the placement held to the rule while at it
std::vector<std::vector<size_t>> shares(avr_multi *m, const Desc &d, size_t entries) {
    std::vector<std::vector<size_t>> mine(entries);
    std::vector<uint64_t> load(entries, 0), sum(entries, 0);
    std::vector<uint32_t> n_bins(d.size()), first;
    for (size_t i = 0; i < d.size(); i++) {
        const int e = avr_multi_placement(m, i);
        CHECK(e >= 0 && size_t(e) < entries, "placement of slice %zu: %d", i, e);
        mine[size_t(e)].push_back(i);
        sum[size_t(e)] += n_bins[i] = uint32_t(d.bins(i));
    }
    CHECK(avr_multi_load(m, load.data()) == AVR_OK && load == sum, "avr_multi_load is not the sum of the entries' slices");
    for (const Group &g : d.groups) first.push_back(uint32_t(g.first));
    std::vector<int> owner(d.size());
    avr::multi_place(n_bins.data(), d.size(), d.kind == AVR_KIND_RANGE_KEYS ? first.data() : nullptr, first.size(), entries, owner.data(), load.data());
    for (size_t i = 0; i < d.size(); i++) CHECK(owner[i] == avr_multi_placement(m, i), "slice %zu is not where the placement rule puts it", i);
    for (size_t e = 0; e < entries; e++) {
        uint32_t info[4] = {9, 9, 9, 9};
        float ms[7] = {9, 9, 9, 9, 9, 9, 9};
        CHECK(avr_multi_entry_info(m, e, info) == AVR_OK && avr_multi_entry_ms(m, e, ms) == AVR_OK, "entry_info / entry_ms of entry %zu", e);
        if (mine[e].empty())
            for (int k = 0; k < 7; k++) CHECK(ms[k] == 0 && info[k & 3] == 0, "an entry without a slice reports something");
    }
    uint32_t info[4];
    CHECK(avr_multi_entry_info(m, entries, info) == AVR_ERR_INVALID, "an entry out of range was taken");
    return mine;
}

// ------------------------------------------------------------------ the batches

Desc range_batch(Rng &r, size_t n) {
    Desc d;
    d.kind = AVR_KIND_RANGE;
    std::vector<size_t> len = lengths(r, n, 0, 700);
    len[1] = 0; len[2] = 1; len[n - 1] = 0;
    for (size_t l : len) d.recs.push_back(range_records(r, l));
    return d;
}
Desc code_batch(Rng &r, size_t n, size_t lo = 0) {
    Desc d;
    d.kind = AVR_KIND_CABAC_CODES;
    std::vector<size_t> len = lengths(r, n, lo, 900);
    if (!lo) { len[0] = 0; len[3] = 1; }
    for (size_t l : len) d.code.push_back(codes(r, l));
    return d;
}
// seven groups: 0 fresh (3 slices), 1 from a table (2), 2 fresh with a malformed key in its second slice (3), 3 without slices,
// 4 from a table (1), 5 fresh with an empty slice (4), 6 fresh (2)
Desc key_batch(Rng &r, bool malformed = true, size_t lo = 0) {
    Desc d;
    d.kind = AVR_KIND_RANGE_KEYS;
    const size_t counts[7] = {3, 2, 3, 0, 1, 4, 2};
    for (size_t g = 0; g < 7; g++) {
        const bool given = g == 1 || g == 4;
        d.groups.push_back({d.recs.size(), given, given ? table(r) : Bytes()});
        for (size_t j = 0; j < counts[g]; j++) d.recs.push_back(key_records(r, g == 5 && j == 1 && !lo ? 0 : lo + r.below(uint32_t(3000 - lo))));
    }
    if (malformed) {
        Recs &bad = d.recs[d.groups[2].first + 1];
        if (bad.size() < 8) bad = key_records(r, 100);
        bad[bad.size() / 2] = uint16_t((AVR_SEL_TERMINATE + 2) << 1);
        d.bad_group = 2;
    }
    return d;
}
// what K1's coded bytes restore to where nothing is wrong: the bytes without their stop byte (the tail patch then changes nothing)
Bytes restored(const Bytes &code) {
    Bytes out(code.size() * 2 + 64);
    int status = 0;
    const size_t len = avr_oracle_cabac_encode_codes(code.data(), code.size(), out.data(), out.size(), &status);
    out.resize(avr_oracle_drop_stop_byte(out.data(), status == AVR_ORACLE_OK ? len : 0));
    return out;
}
Desc expect_batch(Rng &r, size_t n) {                            // right ones, three wrong on purpose, and slices without
    Desc d = code_batch(r, n, 200);
    for (size_t i = 0; i < n; i++) {
        if (i % 4 == 3) continue;
        Bytes want = restored(d.code[i]);
        if (i == 1) want.pop_back();                             // shorter
        if (i == 5) want.insert(want.end(), 2, 0x5a);            // longer (by two: the tail patch itself restores one byte more)
        if (i == 9) want[want.size() / 2] ^= 0x10;               // one byte differing
        d.expects.push_back({i, want});
    }
    return d;
}

// ------------------------------------------------------------------ rule

void expect_created(avr_multi *m, int want, const char *what) {
    CHECK(avr_multi_created(m) == want, "%s: created() = %d, expected %d", what, avr_multi_created(m), want);
}

void rule(size_t entries) {
    Rng r{0x5eed0000 + entries};
    std::vector<int> devices(entries);
    for (size_t e = 0; e < entries; e++) devices[e] = int(e % 3);
    avr_multi *m = avr_multi_create(devices.data(), entries, 256, size_t(1) << 22);
    CHECK(m, "avr_multi_create");
    expect_created(m, 0, "fresh");
    const uint8_t *p;
    size_t len;
    int st;
    CHECK(avr_multi_get(m, 0, &p, &len, &st) == AVR_ERR_INVALID && avr_multi_wait(m) == AVR_ERR_INVALID && avr_multi_placement(m, 0) == AVR_ERR_INVALID,
          "a getter or a wait before any run was taken");

    struct Step { const char *what; Desc d; bool verify, verify_k1, split; size_t findings; };
    std::vector<Step> steps;
    steps.push_back({"range records", range_batch(r, 40), false, false, false, 0});
    steps.push_back({"codes with the K1 verifier", code_batch(r, 35), false, true, true, 0});
    steps.push_back({"key records", key_batch(r), false, false, false, 2});
    steps.push_back({"key records with the verifier", key_batch(r), true, false, true, 2});
    steps.push_back({"range records with the verifier", range_batch(r, 25), true, false, false, 0});
    steps.push_back({"codes with expectations", expect_batch(r, 20), false, false, true, 3});
    steps.push_back({"codes with expectations and the K1 verifier", expect_batch(r, 14), false, true, false, 3});
    int created = 0;
    std::vector<size_t> cap_slices(entries, 0), cap_bins(entries, 0);
    for (Step &s : steps) {
        CHECK(avr_multi_set_verify(m, s.verify) == AVR_OK && avr_multi_set_verify_k1(m, s.verify_k1) == AVR_OK, "%s: the settings", s.what);
        run_multi(m, s.d, s.split, s.what);
        avr_batch *b = single(s.d, s.verify, s.verify_k1);
        against_oracle(b, s.d);
        const size_t findings = compare(m, b, s.d, s.what);
        CHECK(findings == s.findings, "%s: %zu slices with a finding or a bad record, expected %zu", s.what, findings, s.findings);
        const std::vector<std::vector<size_t>> mine = shares(m, s.d, entries);
        if (s.d.kind == AVR_KIND_RANGE_KEYS) {                  // the group without slices: its start table, from the multi's own copy
            CHECK(estimators(m, 3) == Bytes(size_t(AVR_EST_KEYS) * 2, 1), "%s: the empty group's table", s.what);
            for (size_t g = 0; g < s.d.groups.size(); g++) {
                const size_t first = s.d.groups[g].first, last = g + 1 < s.d.groups.size() ? s.d.groups[g + 1].first : s.d.size();
                for (size_t i = first; i < last; i++) CHECK(avr_multi_placement(m, i) == avr_multi_placement(m, first), "%s: a group on two entries", s.what);
            }
        }
        // Reuse: an entry's sub-batch is replaced only where this share outgrows what it was created with.  Counted here by the rule
        // itself from the shares so far.
        for (size_t e = 0; e < entries; e++) {
            if (mine[e].empty()) continue;
            size_t bins = 8;
            for (size_t i : mine[e]) bins += s.d.bins(i);
            if (cap_slices[e] >= mine[e].size() && cap_bins[e] >= bins) continue;
            cap_slices[e] = std::max(cap_slices[e], mine[e].size());
            cap_bins[e] = std::max(cap_bins[e], bins);
            created++;
        }
        expect_created(m, created, s.what);
        avr_batch_destroy(b);
        // the same slices again after a reset: the same answers, and no new sub-batch
        CHECK(avr_multi_reset(m) == AVR_OK, "%s: reset", s.what);
        CHECK(avr_multi_get(m, 0, &p, &len, &st) == AVR_ERR_INVALID, "%s: a getter after reset was taken", s.what);
        if (&s == &steps[1] || &s == &steps[3]) {
            run_multi(m, s.d, !s.split, s.what);
            b = single(s.d, s.verify, s.verify_k1);
            compare(m, b, s.d, s.what);
            avr_batch_destroy(b);
            expect_created(m, created, "the same slices a second time");
            CHECK(avr_multi_reset(m) == AVR_OK, "%s: reset", s.what);
        }
    }

    // the wrong direction: refused by submit before any sub-batch is touched; the object runs once the switch is off
    {
        Desc d = code_batch(r, 12);
        CHECK(avr_multi_set_verify(m, 1) == AVR_OK && avr_multi_set_verify_k1(m, 0) == AVR_OK, "settings");
        feed(m, d);
        const int submits = g_submits.load();
        CHECK(avr_multi_submit(m) == AVR_ERR_INVALID && g_multi_error.find("compress direction only") != std::string::npos, "K2 verification of a K1 multi: %s", g_multi_error.c_str());
        CHECK(avr_multi_run(m) == AVR_ERR_INVALID && g_submits.load() == submits, "the refusal reached a sub-batch");
        CHECK(avr_multi_set_verify(m, 0) == AVR_OK && avr_multi_run(m) == AVR_OK, "the run after the switch is off: %s", g_multi_error.c_str());
        avr_batch *b = single(d, false, false);
        compare(m, b, d, "after the wrong-direction refusal");
        avr_batch_destroy(b);
        CHECK(avr_multi_reset(m) == AVR_OK, "reset");
        Desc k = key_batch(r, false);
        CHECK(avr_multi_set_verify_k1(m, 1) == AVR_OK, "settings");
        feed(m, k);
        CHECK(avr_multi_submit(m) == AVR_ERR_INVALID && g_multi_error.find("decompress direction only") != std::string::npos, "K1 verification of a K2 multi: %s", g_multi_error.c_str());
        CHECK(avr_multi_set_verify_k1(m, 0) == AVR_OK && avr_multi_run(m) == AVR_OK, "the run after the switch is off: %s", g_multi_error.c_str());
        b = single(k, false, false);
        compare(m, b, k, "key records after the wrong-direction refusal");
        avr_batch_destroy(b);
        CHECK(avr_multi_reset(m) == AVR_OK, "reset");
    }

    // refusals at the call, as the batch's
    {
        const Recs one = range_records(r, 16);
        const Bytes byte(4, 7);
        Bytes bad = table(r);
        bad[2 * 500] = 0;
        CHECK(avr_multi_begin_group(m, bad.data()) == AVR_ERR_INVALID && g_multi_error.find("start table entry 500") != std::string::npos, "a malformed start table: %s", g_multi_error.c_str());
        bad[2 * 500] = 0x40; bad[2 * 500 + 1] = 0x21;
        CHECK(avr_multi_begin_group(m, bad.data()) == AVR_ERR_INVALID, "pos + neg above 0x60 was taken");
        CHECK(avr_multi_expect(m, 0, byte.data(), 4) == AVR_ERR_INVALID && g_multi_error.find("has not been added") != std::string::npos, "an expectation for no slice");
        CHECK(avr_multi_add_slice_codes(m, byte.data(), 4) == 0, "add");
        CHECK(avr_multi_expect(m, 0, nullptr, 4) == AVR_ERR_INVALID && avr_multi_expect(m, 0, byte.data(), 0xffffffffull) == AVR_ERR_INVALID &&
              avr_multi_expect(m, 1, byte.data(), 4) == AVR_ERR_INVALID, "a bad expectation was taken");
        CHECK(avr_multi_expect(m, 0, byte.data(), 4) == AVR_OK && avr_multi_expect(m, 0, byte.data(), 4) == AVR_ERR_INVALID &&
              g_multi_error.find("an expectation already") != std::string::npos, "a second expectation");
        CHECK(avr_multi_add_slice_range(m, one.data(), one.size()) == AVR_ERR_INVALID && avr_multi_begin_group(m, nullptr) == AVR_ERR_INVALID &&
              avr_multi_add_slice_range_keys(m, one.data(), one.size()) == AVR_ERR_INVALID, "a second kind was taken");
        CHECK(avr_multi_reset(m) == AVR_OK && avr_multi_add_slice_range(m, one.data(), one.size()) == 0, "reset, add");
        CHECK(avr_multi_expect(m, 0, byte.data(), 4) == AVR_ERR_INVALID && g_multi_error.find("K1 batches only") != std::string::npos, "an expectation of a K2 multi");
        CHECK(avr_multi_reset(m) == AVR_OK && avr_multi_begin_group(m, nullptr) == 0, "reset, begin_group");
        CHECK(avr_multi_add_slice_range(m, one.data(), one.size()) == AVR_ERR_INVALID && avr_multi_add_slice_codes(m, byte.data(), 4) == AVR_ERR_INVALID,
              "a group took a slice of another kind");
        CHECK(avr_multi_reset(m) == AVR_OK, "reset");
    }

    // a run without slices succeeds and runs nothing; a wait without a submit is refused
    {
        const int submits = g_submits.load();
        CHECK(avr_multi_submit(m) == AVR_OK && avr_multi_wait(m) == AVR_OK && g_submits.load() == submits, "the run without slices: %s", g_multi_error.c_str());
        uint32_t info[4] = {1, 1, 1, 1};
        CHECK(avr_multi_entry_info(m, 0, info) == AVR_OK && !info[0] && !info[1] && !info[2] && !info[3], "entry_info of a run without slices");
        CHECK(avr_multi_wait(m) == AVR_ERR_INVALID && avr_multi_get(m, 0, &p, &len, &st) == AVR_ERR_INVALID, "after the run without slices");
        CHECK(avr_multi_reset(m) == AVR_OK, "reset");
    }

    // one entry's submit fails: the others are waited for, the entry's code comes back under the entry's name, and the object takes
    // reset and destroy only -- after which it runs as a fresh one
    {
        Desc d = range_batch(r, 30);
        feed(m, d);
        const int waits = g_waits.load(), submits = g_submits.load();
        g_fail_submits = 1;
        CHECK(avr_multi_submit(m) == AVR_ERR_HIP && g_multi_error.compare(0, 13, "device entry ") == 0, "the failing submit: %s", g_multi_error.c_str());
        const int used = g_submits.load() - submits;
        CHECK(used == int(std::min<size_t>(entries, 30)) && g_waits.load() - waits == used - 1, "%d entries submitted, %d waited for", used, g_waits.load() - waits);
        const Recs one = range_records(r, 16);
        CHECK(avr_multi_add_slice_range(m, one.data(), one.size()) == AVR_ERR_INVALID && avr_multi_submit(m) == AVR_ERR_INVALID && avr_multi_wait(m) == AVR_ERR_INVALID &&
              avr_multi_get(m, 0, &p, &len, &st) == AVR_ERR_INVALID && avr_multi_set_verify(m, 0) == AVR_ERR_INVALID, "a failed multi took a call");
        CHECK(avr_multi_reset(m) == AVR_OK, "reset after the failure");
        run_multi(m, d, true, "after a failure");
        avr_batch *b = single(d, false, false);
        compare(m, b, d, "after a failure");
        avr_batch_destroy(b);
        // a kind the stand-in does not code fails in every entry's add: nothing was submitted, nothing is waited for
        CHECK(avr_multi_reset(m) == AVR_OK, "reset");
        const Recs k1(10, uint16_t(5 << 1));
        const Bytes states(8, 0);
        const int waits2 = g_waits.load();
        CHECK(avr_multi_add_slice_cabac(m, k1.data(), k1.size(), states.data(), states.size()) == 0 && avr_multi_run(m) == AVR_ERR_INVALID &&
              g_multi_error.compare(0, 24, "device entry 0 (device 0") == 0 && g_waits.load() == waits2, "the failing add: %s", g_multi_error.c_str());
    }
    avr_multi_destroy(m);                                        // (in the failed state)

    // a group split over two multis, the second begun from the first one's table: the bytes and the table of the unsplit group
    {
        Desc whole;
        whole.kind = AVR_KIND_RANGE_KEYS;
        whole.groups.push_back({0, false, Bytes()});
        for (size_t j = 0; j < 6; j++) whole.recs.push_back(key_records(r, 200 + r.below(1500)));
        avr_batch *b = single(whole, false, false);
        avr_multi *first = avr_multi_create(devices.data(), entries, 16, size_t(1) << 20), *second = avr_multi_create(devices.data(), entries, 16, size_t(1) << 20);
        CHECK(first && second, "avr_multi_create");
        for (size_t j = 0; j < 3; j++) CHECK(avr_multi_add_slice_range_keys(first, whole.recs[j].data(), whole.recs[j].size()) == int(j), "add");
        CHECK(avr_multi_run(first) == AVR_OK, "run: %s", g_multi_error.c_str());
        const Bytes half = estimators(first, 0);
        CHECK(avr_multi_begin_group(second, half.data()) == 0, "begin_group from the first half's table: %s", g_multi_error.c_str());
        for (size_t j = 3; j < 6; j++) CHECK(avr_multi_add_slice_range_keys(second, whole.recs[j].data(), whole.recs[j].size()) == int(j - 3), "add");
        CHECK(avr_multi_run(second) == AVR_OK, "run: %s", g_multi_error.c_str());
        for (size_t j = 0; j < 6; j++) same(answer(j < 3 ? first : second, j % 3), answer(b, j), "the split group", j);
        CHECK(estimators(second, 0) == estimators(b, 0), "the split group's table");
        avr_multi_destroy(first);
        avr_multi_destroy(second);
        avr_batch_destroy(b);
    }
}

// ------------------------------------------------------------------ fault

uint32_t fault_value(const char *name) {
    const char *env = getenv("AVR_CPU_BATCH_FAULT");
    const std::string s = env ? env : "", key = std::string(name) + "=";
    for (size_t at = 0; at < s.size();) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        if (s.compare(at, key.size(), key) == 0) return uint32_t(strtoul(s.c_str() + at + key.size(), nullptr, 10));
        at = end + 1;
    }
    return 0;
}

// The multi under the fault point against one stand-in batch per entry, each holding that entry's share: local slice k - 1 of every
// entry that has one, and no other slice, has a finding, and it is that batch's.
void fault_case(size_t entries, const Desc &d, bool verify, bool verify_k1, uint32_t k, const char *what) {
    std::vector<int> devices(entries, 0);
    avr_multi *m = avr_multi_create(devices.data(), entries, 256, size_t(1) << 22);
    CHECK(m && avr_multi_set_verify(m, verify) == AVR_OK && avr_multi_set_verify_k1(m, verify_k1) == AVR_OK, "%s: the multi", what);
    run_multi(m, d, false, what);
    const std::vector<std::vector<size_t>> mine = shares(m, d, entries);
    size_t hit = 0;
    for (size_t e = 0; e < entries; e++) {
        if (mine[e].empty()) continue;
        avr_batch *b = single(d, verify, verify_k1, &mine[e]);
        for (size_t j = 0; j < mine[e].size(); j++) {
            const Answer want = answer(b, j), got = answer(m, mine[e][j]);
            same(got, want, what, mine[e][j]);
            const bool finding = got.status == AVR_SLICE_VERIFY_FAILED;
            CHECK(finding == (j + 1 == k), "%s: entry %zu, local slice %zu (slice %zu): status %d", what, e, j, mine[e][j], got.status);
            CHECK(finding == (got.first_bad != AVR_VERIFY_NONE || got.first_bad_est != AVR_VERIFY_NONE || got.first_diff != AVR_VERIFY_NONE),
                  "%s: slice %zu: a finding without an answer, or an answer without a finding", what, mine[e][j]);
            hit += finding;
        }
        avr_batch_destroy(b);
    }
    CHECK(hit >= 2 || entries == 1, "%s: the fault point hit %zu entries", what, hit);
    avr_multi_destroy(m);
}

void fault() {
    const uint32_t verify_flip = fault_value("verify_flip"), est_flip = fault_value("est_flip"), restore_flip = fault_value("restore_flip");
    CHECK(verify_flip || est_flip || restore_flip, "AVR_CPU_BATCH_FAULT names no fault point");
    for (size_t entries : {size_t(1), size_t(3), size_t(4)}) {
        Rng r{0xfa170000 + entries};
        if (verify_flip) {
            Desc d = range_batch(r, 24);
            for (Recs &x : d.recs) if (x.size() < 40) x = range_records(r, 40 + r.below(300));
            fault_case(entries, d, true, false, verify_flip, "verify_flip, range records");
            fault_case(entries, code_batch(r, 24, 60), false, true, verify_flip, "verify_flip, codes");
            fault_case(entries, key_batch(r, false, 60), true, false, verify_flip, "verify_flip, key records");
        }
        if (est_flip) {
            Desc d;                                              // eight groups of two slices: every entry's second slice is a group's second
            d.kind = AVR_KIND_RANGE_KEYS;
            for (size_t g = 0; g < 8; g++) {
                d.groups.push_back({d.recs.size(), g == 5, g == 5 ? table(r) : Bytes()});
                for (size_t j = 0; j < 2; j++) d.recs.push_back(key_records(r, 100 + r.below(2000)));
            }
            fault_case(entries, d, true, false, est_flip, "est_flip");
        }
        if (restore_flip) {
            Desc d = code_batch(r, 24, 200);
            for (size_t i = 0; i < d.size(); i++) d.expects.push_back({i, restored(d.code[i])});
            fault_case(entries, d, false, false, restore_flip, "restore_flip");
            fault_case(entries, d, false, true, restore_flip, "restore_flip behind the K1 verifier");
        }
    }
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "rule";
    if (mode == "rule") {
        CHECK(!getenv("AVR_CPU_BATCH_FAULT"), "the rule is checked without fault points");
        for (size_t entries : {size_t(1), size_t(3), size_t(4)}) rule(entries);
    } else if (mode == "fault") {
        fault();
    } else {
        die("unknown mode %s", mode.c_str());
    }
    printf("multi_check ok: %s, %d sub-batch submits, %d waits\n", mode.c_str(), g_submits.load(), g_waits.load());
    return 0;
}
