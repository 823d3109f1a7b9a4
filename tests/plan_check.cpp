// The plan rules of csrc/avr_plan.h, printed: the header compiled alone by g++ (no HIP), driven by tests/test_plan.py.
// stdin, a line each:   "plan k nb_0 ... nb_(k-1)"   or   "big k nb_0 ... nb_(k-1)"   or   "path n_slices total_bins"   or
// "tiles records_per_chunk k nb_0 ... nb_(k-1)".
// stdout for a plan: the per-slice values (chunks, blocks, work, digits, out), then every array of the K1p plan by name; and a line
// "lesser" telling whether the lesser paths (Serial, Chunks, Codes) build the same arrays and leave the others empty.
// stdout for "big" (slices of up to 2^32 - 1 bins: millions of chunks): the same without the per-chunk arrays, of which a line
// "slices" gives the two sizes and whether every entry is the slice whose range of chunk_base / blk_base holds it.
// stdout for a path: "path 0" or "path 1" (want_chunked).
// stdout for tiles: "order" and "tile_off" of plan_tiles.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "avr_plan.h"

using namespace avr;

template <class V>
static void line(const char *name, const V &v) {
    printf("%s", name);
    for (auto x : v) printf(" %" PRIu64, uint64_t(x));
    printf("\n");
}

int main() {
    uint8_t *const base = reinterpret_cast<uint8_t *>(uintptr_t(0x10000));
    for (unsigned d : {0u, 1u, 255u, 256u, 257u})                 // the pointer round-up: the next multiple of 256, itself if it is one
        if (align256(base + d) != base + (d + 255) / 256 * 256) return 2;
    char what[8];
    while (scanf("%7s", what) == 1) {
        if (!strcmp(what, "path")) {
            uint64_t n_slices, total_bins;
            if (scanf("%" SCNu64 " %" SCNu64, &n_slices, &total_bins) != 2) return 1;
            printf("path %d\n", int(want_chunked(size_t(n_slices), total_bins)));
            continue;
        }
        if (!strcmp(what, "tiles")) {
            uint32_t per_chunk;
            uint64_t k;
            if (scanf("%" SCNu32 " %" SCNu64, &per_chunk, &k) != 2) return 1;
            std::vector<uint32_t> nb(k), order;
            std::vector<uint64_t> tile_off;
            for (auto &x : nb)
                if (scanf("%" SCNu32, &x) != 1) return 1;
            plan_tiles(nb, order, tile_off, per_chunk);
            line("order", order); line("tile_off", tile_off);
            continue;
        }
        uint64_t k;
        const bool big = !strcmp(what, "big");
        if ((!big && strcmp(what, "plan")) || scanf("%" SCNu64, &k) != 1) return 1;
        std::vector<uint32_t> nb(k);
        for (auto &x : nb)
            if (scanf("%" SCNu32, &x) != 1) return 1;
        std::vector<uint64_t> chunks, blocks, work, digits, out;
        for (uint32_t x : nb) {
            chunks.push_back(slice_chunks(x)); blocks.push_back(slice_blocks(x)); work.push_back(slice_work_bytes(x));
            digits.push_back(slice_digit_sums(x)); out.push_back(slice_out_bytes(x));
        }
        line("chunks", chunks); line("blocks", blocks); line("work", work); line("digits", digits); line("out", out);
        HostPlan p, q;
        fill_plan(p, nb.data(), nb.size(), PlanFor::K1p);
        line("out_off", p.out_off); line("res_off", p.res_off); line("dig_off", p.dig_off); line("chunk_base", p.chunk_base);
        if (big) {
            bool in_place = p.chunk_slice.size() == p.chunk_base.back() && p.blk_slice.size() == p.blk_base.back();
            for (size_t i = 0; in_place && i < nb.size(); i++) {
                for (uint32_t c = p.chunk_base[i]; c < p.chunk_base[i + 1]; c++) in_place = in_place && p.chunk_slice[c] == i;
                for (uint32_t b = p.blk_base[i]; b < p.blk_base[i + 1]; b++) in_place = in_place && p.blk_slice[b] == i;
            }
            line("blk_base", p.blk_base);
            printf("slices %zu %zu %d\n", p.chunk_slice.size(), p.blk_slice.size(), int(in_place));
        } else {
            line("chunk_slice", p.chunk_slice); line("blk_base", p.blk_base); line("blk_slice", p.blk_slice);
        }
        printf("totals %" PRIu64 " %" PRIu64 " %" PRIu32 " %" PRIu32 "\n", plan_total(p.res_off), plan_total(p.dig_off), plan_total(p.chunk_base), plan_total(p.blk_base));
        bool same = true;
        q = p;                                                    // refilled from a full plan: what a path does not read must go
        fill_plan(q, nb.data(), nb.size(), PlanFor::Codes);
        same = same && q.out_off == p.out_off && q.chunk_base == p.chunk_base && q.chunk_slice == p.chunk_slice && q.dig_off == p.dig_off &&
               q.res_off.empty() && q.blk_base.empty() && q.blk_slice.empty() && plan_total(q.res_off) == 0 && plan_total(q.blk_base) == 0;
        fill_plan(q, nb.data(), nb.size(), PlanFor::Chunks);
        same = same && q.out_off == p.out_off && q.chunk_base == p.chunk_base && q.chunk_slice == p.chunk_slice && q.dig_off.empty() &&
               q.res_off.empty() && q.blk_base.empty() && q.blk_slice.empty() && plan_total(q.dig_off) == 0;
        fill_plan(q, nb.data(), nb.size(), PlanFor::Serial);
        same = same && q.out_off == p.out_off && q.chunk_base.empty() && q.chunk_slice.empty() && q.dig_off.empty() && q.res_off.empty() &&
               q.blk_base.empty() && q.blk_slice.empty() && plan_total(q.chunk_base) == 0;
        printf("lesser %d\n", int(same));
    }
    return 0;
}
