// avr_multi (avr_multi.cpp): what the layer that shards one batch over a device list shares with the rest -- its placement rule, a
// plain host function that the tests compile on its own (tests/multi_plan_check.cpp), and the two things it needs from whoever
// implements the avr_batch_* calls beside it.  No HIP: avr_multi.cpp is written on include/avrecode_ms_amd.h alone, so it links
// against the device library (avr_api.cpp) and against the CPU stand-in for the batch calls (tests/cpu_batch.cpp) alike.
#ifndef AVR_MULTI_H
#define AVR_MULTI_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace avr {

// The two seams.  avr_api.cpp defines them for the libraries; a program that links avr_multi.cpp with another implementation of the
// batch calls defines its own.
//   multi_set_error     `text` becomes the calling thread's avr_last_error(); returns `code`
//   multi_check_device  AVR_OK for a device index the batch calls would take, else the error (message set) avr_batch_create would give
int multi_set_error(int code, const char *text);
int multi_check_device(int device);

// Placement by units.  A unit is a slice (group_first == nullptr), or, for key records, a whole group: group g holds the slices
// [group_first[g], group_first[g + 1]), the last one up to n_slices, and weighs the sum of their bins.  A group without slices is no
// unit and goes nowhere.
//   Units are taken heaviest first, equal weights in the caller's order (stable); each goes to the entry with the fewest bins so far,
//   ties to the lower entry.
// owner[i] (n_slices values): the entry of slice i; load[e] (n_entries values): the bins entry e was given.  An entry's slices, taken
// in index order, are its units in the caller's order.  The Python twin is sharding.lpt_assign_groups (lpt_assign for slices).
inline void multi_place(const uint32_t *n_bins, size_t n_slices, const uint32_t *group_first, size_t n_groups, size_t n_entries,
                        int *owner, uint64_t *load) {
    struct Unit { size_t first, last; uint64_t weight; };
    std::vector<Unit> units;
    if (group_first) {
        for (size_t g = 0; g < n_groups; g++) {
            const size_t first = group_first[g], last = g + 1 < n_groups ? group_first[g + 1] : n_slices;
            if (first >= last) continue;
            uint64_t w = 0;
            for (size_t i = first; i < last; i++) w += n_bins[i];
            units.push_back({first, last, w});
        }
    } else {
        units.reserve(n_slices);
        for (size_t i = 0; i < n_slices; i++) units.push_back({i, i + 1, n_bins[i]});
    }
    std::vector<size_t> by_weight(units.size());
    std::iota(by_weight.begin(), by_weight.end(), size_t(0));
    std::stable_sort(by_weight.begin(), by_weight.end(), [&](size_t a, size_t b) { return units[a].weight > units[b].weight; });
    std::fill(load, load + n_entries, uint64_t(0));
    std::fill(owner, owner + n_slices, 0);
    for (size_t u : by_weight) {
        const size_t e = size_t(std::min_element(load, load + n_entries) - load);
        load[e] += units[u].weight;
        for (size_t i = units[u].first; i < units[u].last; i++) owner[i] = int(e);
    }
}

}  // namespace avr

#endif
