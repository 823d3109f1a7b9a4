// The estimator resolver (avr_est.h): key records -> K2 range records, on the device.  Kernels and their launcher.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "avr_est.h"
#include "avr_internal.h"

namespace avr {
namespace {

using namespace est;

struct EstParams {
    const uint16_t *keys;
    const uint64_t *rec_off;
    const uint32_t *n_bins;
    const uint32_t *group_first;
    const uint16_t *est_in;                 // {pos, neg} byte pairs read as pos | neg << 8
    uint16_t *est_out;
    const uint32_t *chunk_base, *chunk_slice;
    uint32_t *slice_group, *group_bad, *row32;
    uint16_t *row16;
    uint16_t *recs_out;
    int32_t *status;
    uint32_t n_slices, n_groups, total_chunks;
};

// one chunk: its slice, its bins (n, and up to `padded` the no-op records of the slice's last group of eight), its first record
struct ChunkRef { uint32_t s, n, padded; uint64_t base; };
__device__ inline ChunkRef chunk_ref(const EstParams &p, uint32_t c) {
    ChunkRef k;
    k.s = p.chunk_slice[c];
    const uint32_t in_slice = c - p.chunk_base[k.s], start = chunk_start(in_slice), nb = p.n_bins[k.s];
    k.n = chunk_bins(in_slice, nb);                              // 0 for a chunk that starts at the slice's end (an empty slice's)
    k.padded = padded_bins(start, k.n, nb);
    k.base = p.rec_off[k.s] + start;
    return k;
}
__device__ inline Row group_of(const EstParams &p, uint32_t c) {
    Row r;
    r.g = p.slice_group[p.chunk_slice[c]];
    r.a = p.chunk_base[p.group_first[r.g]];
    r.b = p.chunk_base[p.group_first[r.g + 1]];
    r.c0 = r.c1 = 0;
    return r;
}
__device__ inline uint32_t start_entry(const EstParams &p, uint32_t g, uint32_t k) {
    return p.est_in ? p.est_in[size_t(g) * kKeys + k] : kFresh;
}

// the lanes of the wave that hold this lane's key
__device__ inline uint64_t match_key(uint32_t key, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 11; b++) {
        const bool bit = (key >> b) & 1u;
        const uint64_t bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// slice -> group; no bad slice yet; the table of a group without slices passes through
__global__ __launch_bounds__(256) void k_est_prep(EstParams p) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.n_slices) {
        uint32_t lo = 0, hi = p.n_groups - 1;                    // the last group that starts at or before slice i
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) / 2;
            if (p.group_first[mid] <= i) lo = mid; else hi = mid - 1;
        }
        p.slice_group[i] = lo;
    }
    if (i < p.n_groups) {
        p.group_bad[i] = kNoBad;
        if (p.est_out && p.group_first[i] == p.group_first[i + 1])
            for (uint32_t k = 0; k < kKeys; k++) p.est_out[size_t(i) * kKeys + k] = uint16_t(start_entry(p, i, k));
    }
}

// bins per key of every row (a spanning group's part of a window); order does not matter: 16-byte loads, LDS atomics
__global__ __launch_bounds__(64) void k_est_count(EstParams p) {
    __shared__ uint32_t cnt[kKeysPad];
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    Row rows[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    for (int ri = 0; ri < 2; ri++) {
        const Row r = rows[ri];
        if (r.c0 >= r.c1) continue;
        for (uint32_t k = lane; k < kKeysPad; k += 64) cnt[k] = 0;
        __syncthreads();
        for (uint32_t c = r.c0; c < r.c1; c++) {
            const ChunkRef ck = chunk_ref(p, c);
            const uint4 *src = reinterpret_cast<const uint4 *>(p.keys + ck.base);
            for (uint32_t v = lane; v * 8 < ck.n; v += 64) {
                const uint4 q = src[v];
                const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (uint32_t e = 0; e < 8; e++) {
                    const uint32_t rec = (wd[e / 2] >> (16 * (e & 1))) & 0xffffu;
                    if (v * 8 + e < ck.n && key_ok(rec)) atomicAdd(&cnt[rec >> 1], 1u);
                }
            }
        }
        __syncthreads();
        uint32_t *dst = p.row32 + size_t(2 * w + ri) * kKeysPad;
        for (uint32_t k = lane; k < kKeys; k += 64) dst[k] = cnt[k];
        __syncthreads();
    }
}

// The scan over a spanning group's rows, in blocks (avr_est.h): every block's count sum into the slot of its last row ...
__global__ __launch_bounds__(256) void k_est_scan_agg(EstParams p) {
    const uint32_t w = blockIdx.x;
    Row rows[2];
    BlockHead heads[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    window_block_heads(w, kWindow, rows, heads);
    for (int h = 0; h < 2; h++) {
        if (!heads[h].any) continue;
        const RowSeq seq = heads[h].seq;
        const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
        for (uint32_t k = threadIdx.x; k < kKeys; k += 256) {
            uint32_t sum = 0;
#pragma unroll 8
            for (uint32_t i = i0; i < i1; i++) sum += p.row32[size_t(seq.row(i)) * kKeysPad + k];
            p.row32[size_t(seq.row(i1 - 1)) * kKeysPad + k] = sum;
        }
    }
}
// ... then the total of every key's estimator at the start of every row, from the key's rank there
__global__ __launch_bounds__(256) void k_est_scan(EstParams p) {
    const uint32_t w = blockIdx.x;
    Row rows[2];
    BlockHead heads[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    window_block_heads(w, kWindow, rows, heads);
    const uint32_t *__restrict__ row32 = p.row32;
    uint16_t *__restrict__ row16 = p.row16;
    for (int h = 0; h < 2; h++) {
        if (!heads[h].any) continue;
        const RowSeq seq = heads[h].seq;
        const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
        for (uint32_t k = threadIdx.x; k < kKeys; k += 256) {
            const uint32_t t = total(start_entry(p, heads[h].g, k));
            uint64_t j = 0;
#pragma unroll 8
            for (uint32_t kb = 0; kb < heads[h].kb; kb++) j += row32[size_t(seq.row(seq.block_end(kb) - 1)) * kKeysPad + k];
#pragma unroll 8
            for (uint32_t i = i0; i < i1; i++) {
                const size_t at = size_t(seq.row(i)) * kKeysPad + k;
                row16[at] = uint16_t(total_after(t, j));
                j += row32[at];                                  // (the block's last: its sum, and j is not used again)
            }
        }
    }
}

// One step of a walk: lane l holds bin i0 + l of the chunk.
struct StepIn { uint32_t rec, key, bin; bool in_chunk, valid, leader; uint64_t mask, ones; };
// The walks read a chunk's records from LDS, where stage_chunk puts them with 16-byte loads (two a lane and chunk).
__device__ inline void stage_chunk(const EstParams &p, const ChunkRef &ck, uint16_t *buf, uint32_t lane) {
    const uint4 *src = reinterpret_cast<const uint4 *>(p.keys + ck.base);
    __syncthreads();                                             // the chunk before is done with buf
    for (uint32_t v = lane; v * 8 < ck.n; v += 64) reinterpret_cast<uint4 *>(buf)[v] = src[v];
    __syncthreads();
}
__device__ inline StepIn load_step(const uint16_t *buf, const ChunkRef &ck, uint32_t i0, uint32_t lane) {
    StepIn s;
    const uint32_t idx = i0 + lane;
    s.in_chunk = idx < ck.n;
    s.rec = s.in_chunk ? buf[idx] : 0u;
    s.valid = s.in_chunk && key_ok(s.rec);
    s.key = s.rec >> 1;
    s.bin = s.rec & 1u;
    s.mask = match_key(s.key, s.valid);
    s.ones = __ballot(s.valid && s.bin);
    s.leader = s.valid && (s.mask >> lane) == 1;                 // the key's last lane of the step writes the table
    return s;
}

// every row as a function of pos at its start
__global__ __launch_bounds__(64) void k_est_func(EstParams p) {
    __shared__ uint32_t fn[kKeysPad];
    __shared__ uint16_t run[kKeysPad];                           // total | 1-bins since the last halving << 8
    __shared__ __attribute__((aligned(16))) uint16_t buf[kChunk];
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    Row rows[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    for (int ri = 0; ri < 2; ri++) {
        const Row r = rows[ri];
        if (r.c0 >= r.c1) continue;
        const size_t row = size_t(2 * w + ri) * kKeysPad;
        for (uint32_t k = lane; k < kKeys; k += 64) { fn[k] = kFnIdentity; run[k] = p.row16[row + k] & 0xffu; }
        __syncthreads();
        for (uint32_t c = r.c0; c < r.c1; c++) {
            const ChunkRef ck = chunk_ref(p, c);
            stage_chunk(p, ck, buf, lane);
            for (uint32_t i0 = 0; i0 < ck.n; i0 += 64) {
                const StepIn s = load_step(buf, ck, i0, lane);
                if (s.leader) {
                    const uint32_t ru = run[s.key];
                    const FnRun o = fn_walk_group(FnRun{fn[s.key], ru & 0xffu, ru >> 8}, s.mask, s.ones);
                    fn[s.key] = o.fn;
                    run[s.key] = uint16_t(o.tot | (o.ones << 8));
                }
                __syncthreads();
            }
        }
        for (uint32_t k = lane; k < kKeys; k += 64) p.row32[row + k] = fn_close(fn[k], run[k] >> 8);
        __syncthreads();
    }
}

// The chain over a spanning group's rows, in blocks: every block's functions composed into the slot of its last row ...
__global__ __launch_bounds__(256) void k_est_chain_agg(EstParams p) {
    const uint32_t w = blockIdx.x;
    Row rows[2];
    BlockHead heads[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    window_block_heads(w, kWindow, rows, heads);
    for (int h = 0; h < 2; h++) {
        if (!heads[h].any) continue;
        const RowSeq seq = heads[h].seq;
        const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
        for (uint32_t k = threadIdx.x; k < kKeys; k += 256) {
            uint32_t f = kFnIdentity;
#pragma unroll 8
            for (uint32_t i = i0; i < i1; i++) f = fn_compose(f, p.row32[size_t(seq.row(i)) * kKeysPad + k]);
            p.row32[size_t(seq.row(i1 - 1)) * kKeysPad + k] = f;
        }
    }
}
// ... then {pos, neg} at the start of every row: one fn_apply a block before this one, one a row inside it
__global__ __launch_bounds__(256) void k_est_chain(EstParams p) {
    const uint32_t w = blockIdx.x;
    Row rows[2];
    BlockHead heads[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    window_block_heads(w, kWindow, rows, heads);
    const uint32_t *__restrict__ row32 = p.row32;
    uint16_t *__restrict__ row16 = p.row16;
    for (int h = 0; h < 2; h++) {
        if (!heads[h].any) continue;
        const RowSeq seq = heads[h].seq;
        const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
        for (uint32_t k = threadIdx.x; k < kKeys; k += 256) {
            uint32_t pos = start_entry(p, heads[h].g, k) & 0xffu;
#pragma unroll 8
            for (uint32_t kb = 0; kb < heads[h].kb; kb++) pos = fn_apply(row32[size_t(seq.row(seq.block_end(kb) - 1)) * kKeysPad + k], pos);
#pragma unroll 8
            for (uint32_t i = i0; i < i1; i++) {
                const size_t at = size_t(seq.row(i)) * kKeysPad + k;
                row16[at] = uint16_t(pos | (((row16[at] & 0xffu) - pos) << 8));
                pos = fn_apply(row32[at], pos);                  // (the block's last: its composed function, and pos is not used again)
            }
        }
    }
}

// The walk that writes the records: a window's chunks in stream order, the table of the group at hand in LDS.
__global__ __launch_bounds__(64) void k_est_emit(EstParams p) {
    __shared__ uint16_t tab[kKeysPad];
    __shared__ uint16_t pre[64];
    __shared__ __attribute__((aligned(16))) uint16_t buf[kChunk];        // the chunk's key records, then its range records
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    const uint32_t lo = w * kWindow, hi = min(lo + kWindow, p.total_chunks);
    for (uint32_t c = lo; c < hi; c++) {
        const ChunkRef ck = chunk_ref(p, c);
        const Row gr = group_of(p, c);
        if (c == lo || c == gr.a) {                              // a group's first chunk: its start table; a window's: the row's
            __syncthreads();
            if (c == gr.a) for (uint32_t k = lane; k < kKeys; k += 64) tab[k] = uint16_t(start_entry(p, gr.g, k));
            else for (uint32_t k = lane; k < kKeys; k += 64) tab[k] = p.row16[size_t(2 * w) * kKeysPad + k];
            __syncthreads();
        }
        bool bad = false;
        stage_chunk(p, ck, buf, lane);
        for (uint32_t i0 = 0; i0 < ck.padded; i0 += 64) {
            const StepIn s = load_step(buf, ck, i0, lane);
            bad |= s.in_chunk && !s.valid;
            const uint32_t st0 = s.valid ? tab[s.key] : 0u;
            const uint64_t below = s.mask & ((uint64_t(1) << lane) - 1);
            const uint32_t n = popc64(s.mask);
            const bool plain = no_halving(st0, n);               // the same for every lane of the key
            uint32_t st = advance(st0, popc64(below), popc64(below & s.ones));
            __syncthreads();                                     // every lane has read the table
            if (s.leader) {
                if (plain) tab[s.key] = uint16_t(advance(st0, n, popc64(s.mask & s.ones)));
                else tab[s.key] = uint16_t(walk_group(st0, s.mask, s.ones, [&](uint32_t l, uint32_t v) { pre[l] = uint16_t(v); }));
            }
            __syncthreads();
            if (s.valid && !plain) st = pre[lane];
            if (i0 + lane < ck.padded) buf[i0 + lane] = uint16_t(s.valid ? record(st, s.bin) : AVR_NOP_RANGE);
        }
        __syncthreads();
        for (uint32_t v = lane; v * 8 < ck.padded; v += 64)      // (padded: a multiple of eight, as the chunk's start is)
            reinterpret_cast<uint4 *>(p.recs_out + ck.base)[v] = reinterpret_cast<const uint4 *>(buf)[v];
        if (__ballot(bad) && lane == 0) atomicMin(&p.group_bad[gr.g], ck.s);
        if (c + 1 == gr.b && p.est_out) {
            __syncthreads();
            for (uint32_t k = lane; k < kKeys; k += 64) p.est_out[size_t(gr.g) * kKeys + k] = tab[k];
        }
    }
}

// a malformed record leaves the later slices of its group without estimators: that slice and every later one of the group
__global__ __launch_bounds__(256) void k_est_status(EstParams p) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.n_slices && i >= p.group_bad[p.slice_group[i]]) p.status[i] = AVR_SLICE_BAD_RECORD;
}

}  // namespace

hipError_t launch_est_resolve(hipStream_t s, const Slices &keys, const uint32_t *group_first, uint32_t n_groups, const uint8_t *est_in,
                              uint8_t *est_out, const avr_chunk_plan *pl, void *workspace, uint16_t *recs_out, int32_t *status) {
    const uint32_t n_slices = keys.n_slices, total_chunks = pl->total_chunks;
    if (n_slices == 0 || n_groups == 0) return hipSuccess;
    EstParams p{};
    p.keys = keys.as<uint16_t>(); p.rec_off = keys.off; p.n_bins = keys.n_bins; p.group_first = group_first;
    p.est_in = reinterpret_cast<const uint16_t *>(est_in);
    p.est_out = reinterpret_cast<uint16_t *>(est_out);
    p.chunk_base = pl->chunk_base; p.chunk_slice = pl->chunk_slice;
    const EstLayout L = est_layout(n_slices, n_groups, total_chunks);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    p.slice_group = reinterpret_cast<uint32_t *>(ws + L.slice_group);
    p.group_bad = reinterpret_cast<uint32_t *>(ws + L.group_bad);
    p.row32 = reinterpret_cast<uint32_t *>(ws + L.row32);
    p.row16 = reinterpret_cast<uint16_t *>(ws + L.row16);
    p.recs_out = recs_out; p.status = status;
    p.n_slices = n_slices; p.n_groups = n_groups; p.total_chunks = total_chunks;
    const uint32_t n_windows = (total_chunks + est::kWindow - 1) / est::kWindow;
    k_est_prep<<<(std::max(n_slices, n_groups) + 255) / 256, 256, 0, s>>>(p);
    if (n_windows) {
        k_est_count<<<n_windows, 64, 0, s>>>(p);
        k_est_scan_agg<<<n_windows, 256, 0, s>>>(p);
        k_est_scan<<<n_windows, 256, 0, s>>>(p);
        k_est_func<<<n_windows, 64, 0, s>>>(p);
        k_est_chain_agg<<<n_windows, 256, 0, s>>>(p);
        k_est_chain<<<n_windows, 256, 0, s>>>(p);
        k_est_emit<<<n_windows, 64, 0, s>>>(p);
    }
    k_est_status<<<(n_slices + 255) / 256, 256, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace avr
