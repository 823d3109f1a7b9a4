// The workspace layouts of csrc/avr_layout.h, printed: the header compiled alone by g++ (no HIP), driven by tests/test_layouts.py.
// stdin: one shape a line -- n_slices n_states n_groups res_total dig_total total_chunks total_blocks out_total.
// stdout: a line of sizeofs, then per shape one line per layout: its name, the regions' offsets in order, its total.
#include <inttypes.h>
#include <initializer_list>
#include <stdio.h>

#include "avr_layout.h"

using namespace avr;

static void line(const char *name, std::initializer_list<uint64_t> v) {
    printf("%s", name);
    for (uint64_t x : v) printf(" %" PRIu64, x);
    printf("\n");
}

int main() {
    printf("sizeof %zu %zu %zu %zu\n", sizeof(k1p::Stretch), sizeof(k1p::Entry), sizeof(k1p::SliceTotals), sizeof(SegSummary));
    uint64_t n_slices, n_states, n_groups, res_total, dig_total, total_chunks, total_blocks, out_total;
    while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &n_slices, &n_states,
                 &n_groups, &res_total, &dig_total, &total_chunks, &total_blocks, &out_total) == 8) {
        avr_chunk_plan pl{};
        pl.res_total = res_total; pl.dig_total = dig_total;
        pl.total_chunks = uint32_t(total_chunks); pl.total_blocks = uint32_t(total_blocks);
        const ResolveLayout r = resolve_layout(n_slices, uint32_t(n_states), &pl);
        line("resolve", {r.lbits, r.lend, r.est, r.stretch, r.meta, r.summ, r.total});
        const CodeLayout c = code_layout(n_slices, &pl);
        line("code", {c.stretch, c.entry, c.totals, c.sums, c.tile, c.total});
        const K1pLayout k = k1p_layout(n_slices, uint32_t(n_states), &pl);
        line("k1p", {k.codes, k.resolve, k.code, k.total});
        const K2pLayout k2 = k2p_layout(n_slices, uint32_t(total_chunks), out_total);
        line("k2p", {k2.ck_range, k2.ck_pos, k2.fin_range, k2.fin_pos, k2.long_chunks, k2.sums, k2.total});
        const EstLayout e = est_layout(n_slices, n_groups, total_chunks);
        line("est", {e.slice_group, e.group_bad, e.row32, e.row16, e.total});
    }
    return 0;
}
