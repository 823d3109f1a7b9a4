// TEST INFRASTRUCTURE: avr::multi_place (csrc/avr_multi.h), the placement of avr_multi, as a stand-alone program that the test builds with
// -fsanitize=address,undefined and runs directly (tests/test_multi_plan.py).  It reads cases from standard input,
//     n_cases, then per case:  n_slices  n_groups (-1: every slice is its own unit)  n_entries  n_bins[n_slices]  group_first[n_groups]
// prints per case the owner of every slice and the load of every entry, which the test compares with the Python twins
// (sharding.lpt_assign_groups, sharding.lpt_assign), and checks by itself what needs no twin: the loads add up to the bins of the
// placed slices, each entry's load is the sum over its slices, a group sits on one entry, and no entry leads another by more than
// the heaviest unit.  Exit status 1 with a line on stderr where one of these fails.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../avrecode-ms_amd/csrc/avr_multi.h"

static int bad(size_t c, const char *what) {
    fprintf(stderr, "multi_plan_check: case %zu: %s\n", c, what);
    return 1;
}

int main() {
    size_t n_cases = 0;
    if (scanf("%zu", &n_cases) != 1) return 2;
    for (size_t c = 0; c < n_cases; c++) {
        size_t n = 0, nd = 0;
        long ng = 0;
        if (scanf("%zu %ld %zu", &n, &ng, &nd) != 3) return 2;
        std::vector<uint32_t> n_bins(n), group_first(ng > 0 ? size_t(ng) : 0);
        for (uint32_t &v : n_bins)
            if (scanf("%u", &v) != 1) return 2;
        for (uint32_t &v : group_first)
            if (scanf("%u", &v) != 1) return 2;
        // exact-size heap arrays: the sanitizer sees a write past either end
        std::vector<int> owner(n, -7);
        std::vector<uint64_t> load(nd, ~uint64_t(0));
        avr::multi_place(n_bins.data(), n, ng >= 0 ? group_first.data() : nullptr, ng >= 0 ? size_t(ng) : 0, nd, owner.data(), load.data());

        std::vector<uint64_t> sum(nd, 0);
        uint64_t total = 0, placed = 0, heaviest = 0;
        for (size_t i = 0; i < n; i++) {
            if (owner[i] < 0 || size_t(owner[i]) >= nd) return bad(c, "an owner out of range");
            sum[size_t(owner[i])] += n_bins[i];
            total += n_bins[i];
        }
        if (ng >= 0) {
            for (size_t g = 0; g < size_t(ng); g++) {
                const size_t first = group_first[g], last = g + 1 < size_t(ng) ? group_first[g + 1] : n;
                uint64_t w = 0;
                for (size_t i = first; i < last; i++) {
                    if (owner[i] != owner[first]) return bad(c, "a group on two entries");
                    w += n_bins[i];
                }
                if (w > heaviest) heaviest = w;
            }
        } else {
            for (uint32_t v : n_bins)
                if (v > heaviest) heaviest = v;
        }
        uint64_t lo = ~uint64_t(0), hi = 0;
        for (size_t e = 0; e < nd; e++) {
            if (load[e] != sum[e]) return bad(c, "an entry's load is not the sum of its slices");
            placed += load[e];
            if (load[e] < lo) lo = load[e];
            if (load[e] > hi) hi = load[e];
        }
        if (placed != total) return bad(c, "the loads do not add up to the total");
        if (hi - lo > heaviest) return bad(c, "an entry leads another by more than the heaviest unit");

        for (size_t i = 0; i < n; i++) printf("%d ", owner[i]);
        printf("\n");
        for (size_t e = 0; e < nd; e++) printf("%llu ", static_cast<unsigned long long>(load[e]));
        printf("\n");
    }
    return 0;
}
