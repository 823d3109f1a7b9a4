// The host arithmetic of the device planner (csrc/avr_plan_dev.h: scan_levels, sort_shape, the three layouts and the quote), compiled
// alone by g++ under AddressSanitizer and UBSan and held to what the kernels of avr_plan_dev.hip index, restated here in plain
// integers: for every n in 0..5000, every n within two of a power of two up to 2^31, and 2^31 - 1.  A 2^31-entry scan cannot be run in
// a test of seconds, so its three levels are covered here.  Started by tests/test_plan_dev_layout.py; prints "ok" and the case count.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

#include "avr_plan_dev.h"

using namespace avr;
using namespace avr::plan_dev;

static uint64_t g_n = 0;
#define CHECK(cond)                                                                                             \
    do {                                                                                                        \
        if (!(cond)) {                                                                                          \
            fprintf(stderr, "n = %" PRIu64 ": %s (%s:%d)\n", g_n, #cond, __FILE__, __LINE__);                 \
            exit(1);                                                                                            \
        }                                                                                                       \
    } while (0)

static uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }

// a scan over `entries` entries of `sum_bytes` a sum: the levels k_reduce / k_apply are launched over, and the bytes they index
static uint64_t check_scan(uint64_t entries, uint32_t sum_bytes) {
    const ScanLevels L = scan_levels(entries, sum_bytes);
    CHECK((L.count == 0) == (entries <= 1024));
    CHECK(L.count <= 3);
    if (entries > (uint64_t(1) << 30) && entries <= (uint64_t(1) << 40)) CHECK(L.count == 3);
    if (entries > (uint64_t(1) << 20) && entries <= (uint64_t(1) << 30)) CHECK(L.count == 2);
    uint64_t want = ceil_div(entries, 1024), end = 0;
    for (uint32_t j = 0; j < L.count; j++) {
        CHECK(L.n[j] == want);                                   // one sum per workgroup of the level below
        CHECK(L.n[j] <= 0xffffffffu);                            // a grid's x dimension
        CHECK(L.off[j] >= end && L.off[j] % 8 == 0);             // ascending, apart, aligned for 64-bit sums
        end = L.off[j] + L.n[j] * sum_bytes;
        want = ceil_div(want, 1024);
    }
    if (L.count) CHECK(L.n[L.count - 1] <= 1024 && L.n[L.count - 1] > 1);   // the top level is one workgroup's
    for (uint32_t j = L.count; j < 4; j++) CHECK(L.n[j] == 0 && L.off[j] == 0);
    CHECK(L.bytes >= end);
    return L.bytes;
}

struct Region { uint64_t at, bytes; };

static void check_regions(const std::vector<Region> &r, uint64_t total, uint64_t quote) {
    uint64_t end = 0;
    for (const Region &x : r) {
        CHECK(x.at >= end && x.at % 256 == 0);
        end = x.at + x.bytes;
    }
    CHECK(end <= total && total <= quote);
}

static void check(uint64_t n) {
    g_n = n;
    const uint64_t scan7 = check_scan(n, 7 * 8), scan1 = check_scan(n, 8), tiles1 = check_scan(ceil_div(n, 64), 8);

    const SortShape s = sort_shape(size_t(n));
    CHECK(s.blocks >= 1 && s.blocks <= 1024);
    CHECK(s.per_block % 256 == 0);
    CHECK(uint64_t(s.blocks) * s.per_block >= n);
    CHECK(256u * s.blocks <= 1024u * 256u);                      // the histogram table: at most 256 tiles of 1024, one sum each
    if (n) CHECK(uint64_t(s.blocks - 1) * s.per_block < n || s.blocks == 1024);    // below 1024 workgroups none is empty

    const uint64_t quote = workspace_bytes(size_t(n));
    CHECK(quote % 256 == 0 && quote >= 256);

    const ChunksLayout c = chunks_layout(size_t(n));
    check_regions({{c.totals, sizeof(avr_plan_totals)}, {c.sums, scan7}}, c.total, quote);

    const TilesLayout t = tiles_layout(size_t(n));
    const uint64_t hist_entries = 256u * uint64_t(s.blocks);
    check_regions({{t.keys[0], 4 * n}, {t.vals[0], 4 * n}, {t.keys[1], 4 * n}, {t.vals[1], 4 * n}, {t.hist, 4 * hist_entries},
                   {t.hist_sums, 4 * ceil_div(hist_entries, 1024)}, {t.sums, tiles1}},
                  t.total, quote);

    const CompactLayout k = compact_layout(size_t(n));
    check_regions({{k.sums, scan1}}, k.total, quote);
}

int main() {
    static_assert(sizeof(avr_plan_totals) == 64, "eight 64-bit totals");
    static_assert(kScanTile == 1024 && kSortTile == 256 && kSortBlocks == 1024 && kSortDigits == 256 && kPlanSums == 7, "the kernels' constants");
    std::set<uint64_t> ns;
    for (uint64_t n = 0; n <= 5000; n++) ns.insert(n);
    for (int k = 0; k <= 31; k++)
        for (int d = -2; d <= 2; d++) {
            const int64_t n = (int64_t(1) << k) + d;
            if (n >= 0) ns.insert(uint64_t(n));
        }
    ns.insert((uint64_t(1) << 31) - 1);
    for (uint64_t n : ns) check(n);
    g_n = (uint64_t(1) << 30) + 1;
    CHECK(scan_levels(g_n, 8).count == 3 && scan_levels(g_n - 1, 8).count == 2);
    CHECK(scan_levels(1025, 8).count == 1 && scan_levels((1u << 20) + 1, 8).count == 2 && scan_levels(1u << 20, 8).count == 1);
    printf("ok %zu cases\n", ns.size());
    return 0;
}
