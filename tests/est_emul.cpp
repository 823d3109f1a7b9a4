// CPU emulation of the estimator resolver (csrc/avr_est.h) -- the very functions the kernels of avr_est.hip run, pass by
// pass and 64 lanes a step, with the chunk size and the window size as parameters so that a test can put every halving on,
// before and after a chunk, a row and a slice boundary.  Test build only (tests/test_est_emul.py compares with a plain
// restatement of the update rule).
#include <cstdint>
#include <cstring>
#include <vector>

#include "avr_est.h"

using namespace avr::est;

namespace {

struct Emul {
    const uint16_t *keys;
    const uint64_t *rec_off;
    const uint32_t *n_bins;
    const uint32_t *group_first;
    const uint16_t *est_in;
    uint16_t *est_out;
    uint32_t n_slices, n_groups, cb, W, total_chunks;
    std::vector<uint32_t> chunk_base, chunk_slice, slice_group, group_bad, row32;
    std::vector<uint16_t> row16;
    uint16_t *recs_out;
    int32_t *status;

    struct ChunkRef { uint32_t s, n, padded; uint64_t base; };
    ChunkRef chunk_ref(uint32_t c) const {
        ChunkRef k;
        k.s = chunk_slice[c];
        const uint32_t start = (c - chunk_base[k.s]) * cb, nb = n_bins[k.s];
        k.n = nb > start ? (nb - start < cb ? nb - start : cb) : 0u;
        k.padded = padded_bins(start, k.n, nb);
        k.base = rec_off[k.s] + start;
        return k;
    }
    Row group_of(uint32_t c) const {
        Row r;
        r.g = slice_group[chunk_slice[c]];
        r.a = chunk_base[group_first[r.g]];
        r.b = chunk_base[group_first[r.g + 1]];
        r.c0 = r.c1 = 0;
        return r;
    }
    uint32_t start_entry(uint32_t g, uint32_t k) const { return est_in ? est_in[size_t(g) * kKeys + k] : kFresh; }
    void rows_of(uint32_t w, Row rows[2]) const { window_rows(w, W, total_chunks, [&](uint32_t c) { return group_of(c); }, rows); }

    // one step: the lanes' records, and per lane the mask of the lanes that hold its key
    struct Step { uint32_t rec[64], key[64], bin[64]; bool in_chunk[64], valid[64]; uint64_t mask[64], ones; };
    Step load_step(const ChunkRef &ck, uint32_t i0) const {
        Step s{};
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t idx = i0 + l;
            s.in_chunk[l] = idx < ck.n;
            s.rec[l] = s.in_chunk[l] ? keys[ck.base + idx] : 0u;
            s.valid[l] = s.in_chunk[l] && key_ok(s.rec[l]);
            s.key[l] = s.rec[l] >> 1;
            s.bin[l] = s.rec[l] & 1u;
            if (s.valid[l] && s.bin[l]) s.ones |= uint64_t(1) << l;
        }
        for (uint32_t l = 0; l < 64; l++)
            for (uint32_t m = 0; m < 64; m++)
                if (s.valid[l] && s.valid[m] && s.key[l] == s.key[m]) s.mask[l] |= uint64_t(1) << m;
        return s;
    }

    void prep() {
        slice_group.assign(n_slices, 0);
        for (uint32_t i = 0; i < n_slices; i++) {
            uint32_t lo = 0, hi = n_groups - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) / 2;
                if (group_first[mid] <= i) lo = mid; else hi = mid - 1;
            }
            slice_group[i] = lo;
        }
        group_bad.assign(n_groups, kNoBad);
        for (uint32_t g = 0; g < n_groups; g++)
            if (est_out && group_first[g] == group_first[g + 1])
                for (uint32_t k = 0; k < kKeys; k++) est_out[size_t(g) * kKeys + k] = uint16_t(start_entry(g, k));
    }
    void count(uint32_t w) {
        Row rows[2];
        rows_of(w, rows);
        for (int ri = 0; ri < 2; ri++) {
            const Row r = rows[ri];
            if (r.c0 >= r.c1) continue;
            uint32_t *cnt = &row32[size_t(2 * w + ri) * kKeysPad];
            memset(cnt, 0, kKeysPad * 4);
            for (uint32_t c = r.c0; c < r.c1; c++) {
                const ChunkRef ck = chunk_ref(c);
                for (uint32_t i = 0; i < ck.n; i++) if (key_ok(keys[ck.base + i])) cnt[keys[ck.base + i] >> 1]++;
            }
        }
    }
    void heads_of(uint32_t w, BlockHead heads[2]) const {
        Row rows[2];
        rows_of(w, rows);
        window_block_heads(w, W, rows, heads);
    }
    void scan_agg(uint32_t w) {
        BlockHead heads[2];
        heads_of(w, heads);
        for (int h = 0; h < 2; h++) {
            if (!heads[h].any) continue;
            const RowSeq seq = heads[h].seq;
            const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
            for (uint32_t k = 0; k < kKeys; k++) {
                uint32_t sum = 0;
                for (uint32_t i = i0; i < i1; i++) sum += row32[size_t(seq.row(i)) * kKeysPad + k];
                row32[size_t(seq.row(i1 - 1)) * kKeysPad + k] = sum;
            }
        }
    }
    void scan(uint32_t w) {
        BlockHead heads[2];
        heads_of(w, heads);
        for (int h = 0; h < 2; h++) {
            if (!heads[h].any) continue;
            const RowSeq seq = heads[h].seq;
            const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
            for (uint32_t k = 0; k < kKeys; k++) {
                const uint32_t t = total(start_entry(heads[h].g, k));
                uint64_t j = 0;
                for (uint32_t kb = 0; kb < heads[h].kb; kb++) j += row32[size_t(seq.row(seq.block_end(kb) - 1)) * kKeysPad + k];
                for (uint32_t i = i0; i < i1; i++) {
                    const size_t at = size_t(seq.row(i)) * kKeysPad + k;
                    row16[at] = uint16_t(total_after(t, j));
                    j += row32[at];
                }
            }
        }
    }
    void func(uint32_t w) {
        Row rows[2];
        rows_of(w, rows);
        for (int ri = 0; ri < 2; ri++) {
            const Row r = rows[ri];
            if (r.c0 >= r.c1) continue;
            const size_t row = size_t(2 * w + ri) * kKeysPad;
            std::vector<uint32_t> fn(kKeysPad, kFnIdentity);
            std::vector<uint16_t> run(kKeysPad);
            for (uint32_t k = 0; k < kKeys; k++) run[k] = row16[row + k] & 0xffu;
            for (uint32_t c = r.c0; c < r.c1; c++) {
                const ChunkRef ck = chunk_ref(c);
                for (uint32_t i0 = 0; i0 < ck.n; i0 += 64) {
                    const Step s = load_step(ck, i0);
                    for (uint32_t l = 0; l < 64; l++) {
                        if (!(s.valid[l] && (s.mask[l] >> l) == 1)) continue;            // the key's last lane
                        const uint32_t ru = run[s.key[l]];
                        const FnRun o = fn_walk_group(FnRun{fn[s.key[l]], ru & 0xffu, ru >> 8}, s.mask[l], s.ones);
                        fn[s.key[l]] = o.fn;
                        run[s.key[l]] = uint16_t(o.tot | (o.ones << 8));
                    }
                }
            }
            for (uint32_t k = 0; k < kKeys; k++) row32[row + k] = fn_close(fn[k], run[k] >> 8);
        }
    }
    void chain_agg(uint32_t w) {
        BlockHead heads[2];
        heads_of(w, heads);
        for (int h = 0; h < 2; h++) {
            if (!heads[h].any) continue;
            const RowSeq seq = heads[h].seq;
            const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
            for (uint32_t k = 0; k < kKeys; k++) {
                uint32_t f = kFnIdentity;
                for (uint32_t i = i0; i < i1; i++) f = fn_compose(f, row32[size_t(seq.row(i)) * kKeysPad + k]);
                row32[size_t(seq.row(i1 - 1)) * kKeysPad + k] = f;
            }
        }
    }
    void chain(uint32_t w) {
        BlockHead heads[2];
        heads_of(w, heads);
        for (int h = 0; h < 2; h++) {
            if (!heads[h].any) continue;
            const RowSeq seq = heads[h].seq;
            const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
            for (uint32_t k = 0; k < kKeys; k++) {
                uint32_t pos = start_entry(heads[h].g, k) & 0xffu;
                for (uint32_t kb = 0; kb < heads[h].kb; kb++) pos = fn_apply(row32[size_t(seq.row(seq.block_end(kb) - 1)) * kKeysPad + k], pos);
                for (uint32_t i = i0; i < i1; i++) {
                    const size_t at = size_t(seq.row(i)) * kKeysPad + k;
                    row16[at] = uint16_t(pos | (((row16[at] & 0xffu) - pos) << 8));
                    pos = fn_apply(row32[at], pos);
                }
            }
        }
    }
    void emit(uint32_t w) {
        uint16_t tab[kKeysPad] = {}, pre[64] = {};
        const uint32_t lo = w * W, hi = lo + W < total_chunks ? lo + W : total_chunks;
        for (uint32_t c = lo; c < hi; c++) {
            const ChunkRef ck = chunk_ref(c);
            const Row gr = group_of(c);
            if (c == lo || c == gr.a) {
                if (c == gr.a) for (uint32_t k = 0; k < kKeys; k++) tab[k] = uint16_t(start_entry(gr.g, k));
                else for (uint32_t k = 0; k < kKeys; k++) tab[k] = row16[size_t(2 * w) * kKeysPad + k];
            }
            bool bad = false;
            for (uint32_t i0 = 0; i0 < ck.padded; i0 += 64) {
                const Step s = load_step(ck, i0);
                uint32_t st[64];
                bool plain[64];
                for (uint32_t l = 0; l < 64; l++) {                 // every lane reads the table ...
                    bad |= s.in_chunk[l] && !s.valid[l];
                    const uint32_t st0 = s.valid[l] ? tab[s.key[l]] : 0u;
                    const uint64_t below = s.mask[l] & ((uint64_t(1) << l) - 1);
                    plain[l] = no_halving(st0, popc64(s.mask[l]));
                    st[l] = advance(st0, popc64(below), popc64(below & s.ones));
                }
                uint16_t tab_new[64];
                for (uint32_t l = 0; l < 64; l++) {                 // ... then each key's last lane writes it
                    if (!(s.valid[l] && (s.mask[l] >> l) == 1)) continue;
                    const uint32_t st0 = tab[s.key[l]];
                    if (plain[l]) tab_new[l] = uint16_t(advance(st0, popc64(s.mask[l]), popc64(s.mask[l] & s.ones)));
                    else tab_new[l] = uint16_t(walk_group(st0, s.mask[l], s.ones, [&](uint32_t m, uint32_t v) { pre[m] = uint16_t(v); }));
                }
                for (uint32_t l = 0; l < 64; l++) if (s.valid[l] && (s.mask[l] >> l) == 1) tab[s.key[l]] = tab_new[l];
                for (uint32_t l = 0; l < 64; l++) {
                    if (s.valid[l] && !plain[l]) st[l] = pre[l];
                    if (i0 + l < ck.padded) recs_out[ck.base + i0 + l] = uint16_t(s.valid[l] ? record(st[l], s.bin[l]) : 0u);
                }
            }
            if (bad && ck.s < group_bad[gr.g]) group_bad[gr.g] = ck.s;
            if (c + 1 == gr.b && est_out) for (uint32_t k = 0; k < kKeys; k++) est_out[size_t(gr.g) * kKeys + k] = tab[k];
        }
    }
};

}  // namespace

extern "C" {

// The resolver of avr_range_resolve_device with chunks of chunk_bins bins and windows of `window` chunks.  info[0] = chunks,
// info[1] = rows that a spanning group used, info[2] = groups that span, info[3] = block heads beyond a group's first block
// (kb > 0: the blocks that read the aggregates of the blocks before them).  Returns 0.
int est_emul_resolve(const uint16_t *keys, const uint64_t *rec_off, const uint32_t *n_bins, uint32_t n_slices,
                     const uint32_t *group_first, uint32_t n_groups, const uint8_t *est_in, uint8_t *est_out,
                     uint32_t chunk_bins, uint32_t window, uint16_t *recs_out, int32_t *status, uint32_t *info) {
    if (!n_slices || !n_groups) return 0;
    Emul e{};
    e.keys = keys; e.rec_off = rec_off; e.n_bins = n_bins; e.group_first = group_first;
    e.est_in = reinterpret_cast<const uint16_t *>(est_in);
    e.est_out = reinterpret_cast<uint16_t *>(est_out);
    e.n_slices = n_slices; e.n_groups = n_groups; e.cb = chunk_bins; e.W = window;
    e.recs_out = recs_out; e.status = status;
    e.chunk_base.assign(n_slices + 1, 0);
    for (uint32_t i = 0; i < n_slices; i++) {
        const uint32_t nc = n_bins[i] ? (n_bins[i] + chunk_bins - 1) / chunk_bins : 1;
        e.chunk_base[i + 1] = e.chunk_base[i] + nc;
        e.chunk_slice.insert(e.chunk_slice.end(), nc, i);
    }
    e.total_chunks = e.chunk_base[n_slices];
    const uint64_t rows = n_rows(e.total_chunks, window);
    e.row32.assign(rows * kKeysPad, 0xdeadbeefu);                 // the kernels' workspace is not zeroed either
    e.row16.assign(rows * kKeysPad, 0xdeadu);
    const uint32_t n_windows = (e.total_chunks + window - 1) / window;
    e.prep();
    for (uint32_t w = 0; w < n_windows; w++) e.count(w);
    for (uint32_t w = 0; w < n_windows; w++) e.scan_agg(w);
    for (uint32_t w = n_windows; w-- > 0;) e.scan(w);             // (any order, here and below)
    for (uint32_t w = 0; w < n_windows; w++) e.func(w);
    for (uint32_t w = 0; w < n_windows; w++) e.chain_agg(w);
    for (uint32_t w = n_windows; w-- > 0;) e.chain(w);
    for (uint32_t w = n_windows; w-- > 0;) e.emit(w);             // any order: a window's walk depends on no other window's
    for (uint32_t i = 0; i < n_slices; i++) if (i >= e.group_bad[e.slice_group[i]]) status[i] = 3;
    if (info) {
        info[0] = e.total_chunks; info[1] = info[2] = info[3] = 0;
        for (uint32_t w = 0; w < n_windows; w++) {
            Row rows2[2];
            BlockHead heads[2];
            e.rows_of(w, rows2);
            window_block_heads(w, window, rows2, heads);
            info[1] += (rows2[0].c0 < rows2[0].c1) + (rows2[1].c0 < rows2[1].c1);
            info[2] += rows2[1].c0 < rows2[1].c1;
            info[3] += (heads[0].any && heads[0].kb > 0) + (heads[1].any && heads[1].kb > 0);
        }
    }
    return 0;
}

uint64_t est_emul_workspace_bytes(uint64_t n_slices, uint64_t n_groups, uint64_t total_chunks) {
    return workspace_bytes(n_slices, n_groups, total_chunks);
}

}  // extern "C"
