// CPU emulation of the estimator checker (csrc/avr_est_verify.h) -- the very functions the kernels of avr_est_verify.hip run, pass by
// pass and 64 lanes a step, with the chunk size and the span as parameters so that a test can put a key's first, last and next bin on,
// before and after a chunk, a span and a slice boundary.  The workspace is one heap buffer of exactly the quoted size, preset to a
// byte of the caller's.  Test build only (tests/test_est_verify_emul.py compares with tests/est_verify_ref.py; tests/est_verify_check.cpp
// includes this file and runs it under the sanitizers).
#include <cstdint>
#include <cstring>
#include <vector>

#include "avr_est_verify.h"

using namespace avr::estv;

namespace {

struct EmulV {
    const uint16_t *keys, *recs;
    const uint64_t *rec_off;
    const uint32_t *n_bins;
    const uint32_t *group_first;
    const uint16_t *est_in, *est_out;
    uint32_t n_slices, n_groups, cb, S, total_chunks;
    std::vector<uint32_t> chunk_base, chunk_slice;
    uint32_t *slice_group;
    uint16_t *tab, *agg;
    int32_t *status;
    uint32_t *first_bad;

    struct ChunkAt { uint32_t s, start, n, padded; uint64_t base; };
    ChunkAt chunk_at(uint32_t c) const {
        ChunkAt k;
        k.s = chunk_slice[c];
        const uint32_t nb = n_bins[k.s];
        k.start = (c - chunk_base[k.s]) * cb;
        k.n = nb > k.start ? (nb - k.start < cb ? nb - k.start : cb) : 0u;
        k.padded = padded_bins(k.start, k.n, nb);
        k.base = rec_off[k.s] + k.start;
        return k;
    }
    Group group_at(uint32_t c) const {
        Group r;
        r.g = slice_group[chunk_slice[c]];
        r.a = chunk_base[group_first[r.g]];
        r.b = chunk_base[group_first[r.g + 1]];
        return r;
    }
    uint32_t start_entry(uint32_t g, uint32_t k) const { return est_in ? est_in[size_t(g) * kKeys + k] : kFresh; }
    bool takes_part(uint32_t s) const { return status[s] != kBadRecord; }
    void note(uint32_t s, uint32_t v) { if (v < first_bad[s]) first_bad[s] = v; }          // atomicMin
    void pieces_of(uint32_t w, Piece pc[2]) const { span_pieces(w, S, total_chunks, [&](uint32_t c) { return group_at(c); }, pc); }
    void heads_of(uint32_t w, BlockHead heads[2]) const {
        Piece pc[2];
        pieces_of(w, pc);
        span_block_heads(w, S, pc, heads);
    }

    void prep() {
        for (uint32_t i = 0; i < n_slices; i++) {
            uint32_t lo = 0, hi = n_groups - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) / 2;
                if (group_first[mid] <= i) lo = mid; else hi = mid - 1;
            }
            slice_group[i] = lo;
            first_bad[i] = kNone;
        }
    }
    void last(uint32_t w) {
        Piece pc[2];
        pieces_of(w, pc);
        for (int pi = 0; pi < 2; pi++) {
            if (pc[pi].c0 >= pc[pi].c1) continue;
            std::vector<uint32_t> la(kTabStride, 0);
            for (uint32_t c = pc[pi].c1; c-- > pc[pi].c0;) {         // any order: backwards here
                const ChunkAt ck = chunk_at(c);
                if (!takes_part(ck.s)) continue;
                const uint32_t at = (c - pc[pi].c0) * cb;
                for (uint32_t i = ck.n; i-- > 0;) {
                    const uint32_t krec = keys[ck.base + i], rrec = recs[ck.base + i];
                    if (!key_ok(krec)) continue;
                    const uint32_t v = last_entry(at + i, next_of(rrec, krec));
                    if (v > la[krec >> 1]) la[krec >> 1] = v;        // atomicMax
                }
            }
            uint16_t *dst = tab + size_t(2 * w + pi) * kTabStride;
            for (uint32_t k = 0; k < kKeys; k++) dst[k] = uint16_t(la[k]);
        }
    }
    void aggregate(uint32_t w) {
        BlockHead heads[2];
        heads_of(w, heads);
        for (int h = 0; h < 2; h++) {
            if (!heads[h].any) continue;
            const PieceSeq seq = heads[h].seq;
            const uint32_t i0 = heads[h].kb * kPieceBlock, i1 = seq.block_end(heads[h].kb);
            for (uint32_t k = 0; k < kKeys; k++) {
                uint32_t a = 0;
                for (uint32_t i = i0; i < i1; i++) a = then(a, tab[size_t(seq.slot(i)) * kTabStride + k]);
                agg[size_t(seq.slot(i1 - 1)) * kTabStride + k] = uint16_t(a);
            }
        }
    }
    void start(uint32_t w) {
        BlockHead heads[2];
        heads_of(w, heads);
        for (int h = 0; h < 2; h++) {
            if (!heads[h].any) continue;
            const PieceSeq seq = heads[h].seq;
            const uint32_t i0 = heads[h].kb * kPieceBlock, i1 = seq.block_end(heads[h].kb);
            for (uint32_t k = 0; k < kKeys; k++) {
                uint32_t cur = start_entry(heads[h].g, k);
                for (uint32_t kb = 0; kb < heads[h].kb; kb++) cur = then(cur, agg[size_t(seq.slot(seq.block_end(kb) - 1)) * kTabStride + k]);
                for (uint32_t i = i0; i < i1; i++) {
                    const size_t at = size_t(seq.slot(i)) * kTabStride + k;
                    const uint32_t nx = tab[at];
                    tab[at] = uint16_t(cur);
                    cur = then(cur, nx);
                }
            }
        }
    }
    void check(uint32_t w) {
        uint16_t t[kTabStride] = {};
        const uint32_t lo = w * S, hi = lo + S < total_chunks ? lo + S : total_chunks;
        for (uint32_t c = lo; c < hi; c++) {
            const ChunkAt ck = chunk_at(c);
            const Group gr = group_at(c);
            if (c == lo || c == gr.a) {
                if (c == gr.a) for (uint32_t k = 0; k < kKeys; k++) t[k] = uint16_t(start_entry(gr.g, k));
                else for (uint32_t k = 0; k < kKeys; k++) t[k] = tab[size_t(2 * w) * kTabStride + k];
            }
            if (!takes_part(ck.s)) continue;
            bool pad_bad = false;
            for (uint32_t i0 = 0; i0 < ck.padded; i0 += 64) {
                uint32_t krec[64], rrec[64], nx[64];
                bool in_chunk[64], valid[64];
                uint64_t mask[64] = {};
                for (uint32_t l = 0; l < 64; l++) {
                    const uint32_t idx = i0 + l;
                    in_chunk[l] = idx < ck.n;
                    krec[l] = in_chunk[l] ? keys[ck.base + idx] : 0u;
                    rrec[l] = idx < ck.padded ? recs[ck.base + idx] : 0u;
                    valid[l] = in_chunk[l] && key_ok(krec[l]);
                    nx[l] = next_of(rrec[l], krec[l]);
                }
                for (uint32_t l = 0; l < 64; l++)
                    for (uint32_t m = 0; m < 64; m++)
                        if (valid[l] && valid[m] && (krec[l] >> 1) == (krec[m] >> 1)) mask[l] |= uint64_t(1) << m;
                int first = -1;
                for (uint32_t l = 0; l < 64; l++) {                  // every lane reads the table ...
                    const int from = valid[l] ? lower_lane(mask[l], l) : -1;
                    const uint32_t expected = from >= 0 ? nx[from] : valid[l] ? t[krec[l] >> 1] : 0u;
                    if (in_chunk[l] && bin_bad(krec[l], rrec[l], expected) && first < 0) first = int(l);
                    pad_bad |= !in_chunk[l] && rrec[l] != 0;
                }
                for (uint32_t l = 0; l < 64; l++)                    // ... then each key's last lane writes it
                    if (valid[l] && (mask[l] >> l) == 1) t[krec[l] >> 1] = uint16_t(nx[l]);
                if (first >= 0) note(ck.s, ck.start + i0 + uint32_t(first));
            }
            if (pad_bad) note(ck.s, n_bins[ck.s]);
            if (c + 1 == gr.b && est_out) {
                bool diff = false;
                for (uint32_t k = 0; k < kKeys; k++) diff |= t[k] != est_out[size_t(gr.g) * kKeys + k];
                if (diff) note(ck.s, n_bins[ck.s]);
            }
        }
    }
};

}  // namespace

extern "C" {

// The checker of avr_range_keys_verify_device with chunks of chunk_bins bins and spans of `span` chunks (span * chunk_bins < 65536),
// its workspace preset to `poison`.  info[0] = chunks, info[1] = pieces of crossing groups, info[2] = crossing groups, info[3] = blocks
// beyond a group's first.  Returns 0.
int estv_emul_verify(const uint16_t *keys, const uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins, uint32_t n_slices,
                     const uint32_t *group_first, uint32_t n_groups, const uint8_t *est_in, const uint8_t *est_out, uint32_t chunk_bins,
                     uint32_t span, uint32_t poison, int32_t *status, uint32_t *first_bad, uint32_t *info) {
    if (!n_slices || !n_groups) return 0;
    EmulV e{};
    e.keys = keys; e.recs = recs; e.rec_off = rec_off; e.n_bins = n_bins; e.group_first = group_first;
    e.est_in = reinterpret_cast<const uint16_t *>(est_in);
    e.est_out = reinterpret_cast<const uint16_t *>(est_out);
    e.n_slices = n_slices; e.n_groups = n_groups; e.cb = chunk_bins; e.S = span;
    e.status = status; e.first_bad = first_bad;
    e.chunk_base.assign(n_slices + 1, 0);
    for (uint32_t i = 0; i < n_slices; i++) {
        const uint32_t nc = n_bins[i] ? (n_bins[i] + chunk_bins - 1) / chunk_bins : 1;
        e.chunk_base[i + 1] = e.chunk_base[i] + nc;
        e.chunk_slice.insert(e.chunk_slice.end(), nc, i);
    }
    e.total_chunks = e.chunk_base[n_slices];
    // the layout of avr_layout.h for this span: the same three regions
    const uint64_t slots = avr::estv::n_slots(e.total_chunks, span);
    const uint64_t sg = avr::align256(4ull * n_slices), tb = slots * kTabStride * 2;
    uint8_t *ws = new uint8_t[sg + 2 * tb];
    memset(ws, int(poison & 0xff), sg + 2 * tb);
    e.slice_group = reinterpret_cast<uint32_t *>(ws);
    e.tab = reinterpret_cast<uint16_t *>(ws + sg);
    e.agg = reinterpret_cast<uint16_t *>(ws + sg + tb);
    const uint32_t n_spans = (e.total_chunks + span - 1) / span;
    e.prep();
    for (uint32_t w = n_spans; w-- > 0;) e.last(w);               // (any order, here and below)
    for (uint32_t w = 0; w < n_spans; w++) e.aggregate(w);
    for (uint32_t w = n_spans; w-- > 0;) e.start(w);
    for (uint32_t w = n_spans; w-- > 0;) e.check(w);
    for (uint32_t i = 0; i < n_slices; i++) if (first_bad[i] != kNone && status[i] == kOk) status[i] = kVerifyFailed;
    if (info) {
        info[0] = e.total_chunks; info[1] = info[2] = info[3] = 0;
        for (uint32_t w = 0; w < n_spans; w++) {
            Piece pc[2];
            BlockHead heads[2];
            e.pieces_of(w, pc);
            span_block_heads(w, span, pc, heads);
            info[1] += (pc[0].c0 < pc[0].c1) + (pc[1].c0 < pc[1].c1);
            info[2] += pc[1].c0 < pc[1].c1;
            info[3] += (heads[0].any && heads[0].kb > 0) + (heads[1].any && heads[1].kb > 0);
        }
    }
    delete[] ws;
    return 0;
}

uint64_t estv_emul_workspace_bytes(uint64_t n_slices, uint64_t total_chunks) { return workspace_bytes(n_slices, total_chunks); }
uint32_t estv_emul_step(uint32_t e, uint32_t b) { return step(e, b); }
uint32_t estv_emul_span() { return kSpan; }

}  // extern "C"
