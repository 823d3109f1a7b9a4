// The estimator resolver (avr_est.h): key records -> K2 range records, on the device.  Kernels and their launcher.
// Every kernel that touches a key record or a table is a template on the record's form (Keys16, Keys8 below): one resolver, two widths.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "avr_est.h"
#include "avr_internal.h"

namespace avr {
namespace {

using namespace est;

// The two forms of key records.  Rec: a record; kKeys: estimators to a table (est_in, est_out); kPad: a table's stride in LDS and in the
// workspace; kBallots: bits of a key (match_key); kPerLoad: records to a 16-byte load.
//   Keys16  AVR_KIND_RANGE_KEYS: bin | key << 1, key <= AVR_SEL_TERMINATE; rec_off in records, multiples of 8
//   Keys8   AVR_KIND_RANGE_KEYS8: bin | dense id << 1, every value a key; rec_off in bytes, multiples of 16 (a slice whose rec_off is
//           not is read from the multiple of 16 below, written nowhere, and is a bad slice of its group)
// Emit: k_est_emit's LDS buffers of a chunk -- its range records on their way out, and where its key records are staged: two-byte
// keys in the same 2 KiB (a lane reads its key before it writes its record there), one-byte keys in 1 KiB of their own
struct Keys16 {
    struct Emit {
        uint16_t out[kChunk];
        __device__ uint16_t *keys() { return out; }
    };
    using Rec = uint16_t;
    static constexpr uint32_t kKeys = est::kKeys, kPad = kKeysPad, kBallots = 11, kPerLoad = 8;
    static constexpr bool kOneByte = false;
};
struct Keys8 {
    struct Emit {
        uint16_t out[kChunk];
        uint8_t in[kChunk];
        __device__ uint8_t *keys() { return in; }
    };
    using Rec = uint8_t;
    static constexpr uint32_t kKeys = AVR_EST_KEYS8, kPad = kKeysPad8, kBallots = 7, kPerLoad = 16;
    static constexpr bool kOneByte = true;
};
template <class T> __device__ inline bool rec_ok(uint32_t rec) { if constexpr (T::kOneByte) return true; else return key_ok(rec); }
// record e of the kPerLoad a 16-byte load holds, wd its four words
template <class T> __device__ inline uint32_t rec_of(const uint32_t wd[4], uint32_t e) {
    constexpr uint32_t per_word = T::kPerLoad / 4, bits = 32 / per_word;
    return (wd[e / per_word] >> (bits * (e % per_word))) & ((1u << bits) - 1);
}

template <class T>
struct EstParams {
    const typename T::Rec *keys;
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
template <class T>
__device__ inline ChunkRef chunk_ref(const EstParams<T> &p, uint32_t c) {
    ChunkRef k;
    k.s = p.chunk_slice[c];
    const uint32_t in_slice = c - p.chunk_base[k.s], start = chunk_start(in_slice), nb = p.n_bins[k.s];
    k.n = chunk_bins(in_slice, nb);                              // 0 for a chunk that starts at the slice's end (an empty slice's)
    k.padded = padded_bins(start, k.n, nb);
    k.base = p.rec_off[k.s] + start;
    return k;
}
// where the chunk's key records are read from (16-byte aligned: a chunk's start is a multiple of kChunk); one-byte records: whatever rec_off says
template <class T>
__device__ inline const uint4 *chunk_keys(const EstParams<T> &p, const ChunkRef &ck) {
    if constexpr (T::kOneByte) return reinterpret_cast<const uint4 *>(p.keys + (ck.base & ~uint64_t(15)));
    else return reinterpret_cast<const uint4 *>(p.keys + ck.base);
}
template <class T>
__device__ inline Row group_of(const EstParams<T> &p, uint32_t c) {
    Row r;
    r.g = p.slice_group[p.chunk_slice[c]];
    r.a = p.chunk_base[p.group_first[r.g]];
    r.b = p.chunk_base[p.group_first[r.g + 1]];
    r.c0 = r.c1 = 0;
    return r;
}
template <class T>
__device__ inline uint32_t start_entry(const EstParams<T> &p, uint32_t g, uint32_t k) {
    return p.est_in ? p.est_in[size_t(g) * T::kKeys + k] : kFresh;
}

// the lanes of the wave that hold this lane's key
template <class T>
__device__ inline uint64_t match_key(uint32_t key, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < int(T::kBallots); b++) {
        const bool bit = (key >> b) & 1u;
        const uint64_t bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// slice -> group; no bad slice yet; the table of a group without slices passes through
template <class T>
__global__ __launch_bounds__(256) void k_est_prep(EstParams<T> p) {
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
            for (uint32_t k = 0; k < T::kKeys; k++) p.est_out[size_t(i) * T::kKeys + k] = uint16_t(start_entry(p, i, k));
    }
}

// bins per key of every row (a spanning group's part of a window); order does not matter: 16-byte loads, LDS atomics
template <class T>
__global__ __launch_bounds__(64) void k_est_count(EstParams<T> p) {
    __shared__ uint32_t cnt[T::kPad];
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    Row rows[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    for (int ri = 0; ri < 2; ri++) {
        const Row r = rows[ri];
        if (r.c0 >= r.c1) continue;
        for (uint32_t k = lane; k < T::kPad; k += 64) cnt[k] = 0;
        __syncthreads();
        for (uint32_t c = r.c0; c < r.c1; c++) {
            const ChunkRef ck = chunk_ref(p, c);
            const uint4 *src = chunk_keys(p, ck);
            for (uint32_t v = lane; v * T::kPerLoad < ck.n; v += 64) {
                const uint4 q = src[v];
                const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (uint32_t e = 0; e < T::kPerLoad; e++) {
                    const uint32_t rec = rec_of<T>(wd, e);
                    if (v * T::kPerLoad + e < ck.n && rec_ok<T>(rec)) atomicAdd(&cnt[rec >> 1], 1u);
                }
            }
        }
        __syncthreads();
        uint32_t *dst = p.row32 + size_t(2 * w + ri) * T::kPad;
        for (uint32_t k = lane; k < T::kKeys; k += 64) dst[k] = cnt[k];
        __syncthreads();
    }
}

// The scan over a spanning group's rows, in blocks (avr_est.h): every block's count sum into the slot of its last row ...
template <class T>
__global__ __launch_bounds__(256) void k_est_scan_agg(EstParams<T> p) {
    const uint32_t w = blockIdx.x;
    Row rows[2];
    BlockHead heads[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    window_block_heads(w, kWindow, rows, heads);
    for (int h = 0; h < 2; h++) {
        if (!heads[h].any) continue;
        const RowSeq seq = heads[h].seq;
        const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
        for (uint32_t k = threadIdx.x; k < T::kKeys; k += 256) {
            uint32_t sum = 0;
#pragma unroll 8
            for (uint32_t i = i0; i < i1; i++) sum += p.row32[size_t(seq.row(i)) * T::kPad + k];
            p.row32[size_t(seq.row(i1 - 1)) * T::kPad + k] = sum;
        }
    }
}
// ... then the total of every key's estimator at the start of every row, from the key's rank there
template <class T>
__global__ __launch_bounds__(256) void k_est_scan(EstParams<T> p) {
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
        for (uint32_t k = threadIdx.x; k < T::kKeys; k += 256) {
            const uint32_t t = total(start_entry(p, heads[h].g, k));
            uint64_t j = 0;
#pragma unroll 8
            for (uint32_t kb = 0; kb < heads[h].kb; kb++) j += row32[size_t(seq.row(seq.block_end(kb) - 1)) * T::kPad + k];
#pragma unroll 8
            for (uint32_t i = i0; i < i1; i++) {
                const size_t at = size_t(seq.row(i)) * T::kPad + k;
                row16[at] = uint16_t(total_after(t, j));
                j += row32[at];                                  // (the block's last: its sum, and j is not used again)
            }
        }
    }
}

// One step of a walk: lane l holds bin i0 + l of the chunk.
struct StepIn { uint32_t rec, key, bin; bool in_chunk, valid, leader; uint64_t mask, ones; };
// The walks read a chunk's records from LDS, where stage_chunk puts them with 16-byte loads (two a lane and chunk; one of one-byte records).
template <class T>
__device__ inline void stage_chunk(const EstParams<T> &p, const ChunkRef &ck, typename T::Rec *buf, uint32_t lane) {
    const uint4 *src = chunk_keys(p, ck);
    __syncthreads();                                             // the chunk before is done with buf
    for (uint32_t v = lane; v * T::kPerLoad < ck.n; v += 64) reinterpret_cast<uint4 *>(buf)[v] = src[v];
    __syncthreads();
}
template <class T>
__device__ inline StepIn load_step(const typename T::Rec *buf, const ChunkRef &ck, uint32_t i0, uint32_t lane) {
    StepIn s;
    const uint32_t idx = i0 + lane;
    s.in_chunk = idx < ck.n;
    s.rec = s.in_chunk ? buf[idx] : 0u;
    s.valid = s.in_chunk && rec_ok<T>(s.rec);
    s.key = s.rec >> 1;
    s.bin = s.rec & 1u;
    s.mask = match_key<T>(s.key, s.valid);
    s.ones = __ballot(s.valid && s.bin);
    s.leader = s.valid && (s.mask >> lane) == 1;                 // the key's last lane of the step writes the table
    return s;
}

// every row as a function of pos at its start
template <class T>
__global__ __launch_bounds__(64) void k_est_func(EstParams<T> p) {
    __shared__ uint32_t fn[T::kPad];
    __shared__ uint16_t run[T::kPad];                            // total | 1-bins since the last halving << 8
    __shared__ __attribute__((aligned(16))) typename T::Rec buf[kChunk];
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    Row rows[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    for (int ri = 0; ri < 2; ri++) {
        const Row r = rows[ri];
        if (r.c0 >= r.c1) continue;
        const size_t row = size_t(2 * w + ri) * T::kPad;
        for (uint32_t k = lane; k < T::kKeys; k += 64) { fn[k] = kFnIdentity; run[k] = p.row16[row + k] & 0xffu; }
        __syncthreads();
        for (uint32_t c = r.c0; c < r.c1; c++) {
            const ChunkRef ck = chunk_ref(p, c);
            stage_chunk(p, ck, buf, lane);
            for (uint32_t i0 = 0; i0 < ck.n; i0 += 64) {
                const StepIn s = load_step<T>(buf, ck, i0, lane);
                if (s.leader) {
                    const uint32_t ru = run[s.key];
                    const FnRun o = fn_walk_group(FnRun{fn[s.key], ru & 0xffu, ru >> 8}, s.mask, s.ones);
                    fn[s.key] = o.fn;
                    run[s.key] = uint16_t(o.tot | (o.ones << 8));
                }
                __syncthreads();
            }
        }
        for (uint32_t k = lane; k < T::kKeys; k += 64) p.row32[row + k] = fn_close(fn[k], run[k] >> 8);
        __syncthreads();
    }
}

// The chain over a spanning group's rows, in blocks: every block's functions composed into the slot of its last row ...
template <class T>
__global__ __launch_bounds__(256) void k_est_chain_agg(EstParams<T> p) {
    const uint32_t w = blockIdx.x;
    Row rows[2];
    BlockHead heads[2];
    window_rows(w, kWindow, p.total_chunks, [&](uint32_t c) { return group_of(p, c); }, rows);
    window_block_heads(w, kWindow, rows, heads);
    for (int h = 0; h < 2; h++) {
        if (!heads[h].any) continue;
        const RowSeq seq = heads[h].seq;
        const uint32_t i0 = heads[h].kb * kRowBlock, i1 = seq.block_end(heads[h].kb);
        for (uint32_t k = threadIdx.x; k < T::kKeys; k += 256) {
            uint32_t f = kFnIdentity;
#pragma unroll 8
            for (uint32_t i = i0; i < i1; i++) f = fn_compose(f, p.row32[size_t(seq.row(i)) * T::kPad + k]);
            p.row32[size_t(seq.row(i1 - 1)) * T::kPad + k] = f;
        }
    }
}
// ... then {pos, neg} at the start of every row: one fn_apply a block before this one, one a row inside it
template <class T>
__global__ __launch_bounds__(256) void k_est_chain(EstParams<T> p) {
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
        for (uint32_t k = threadIdx.x; k < T::kKeys; k += 256) {
            uint32_t pos = start_entry(p, heads[h].g, k) & 0xffu;
#pragma unroll 8
            for (uint32_t kb = 0; kb < heads[h].kb; kb++) pos = fn_apply(row32[size_t(seq.row(seq.block_end(kb) - 1)) * T::kPad + k], pos);
#pragma unroll 8
            for (uint32_t i = i0; i < i1; i++) {
                const size_t at = size_t(seq.row(i)) * T::kPad + k;
                row16[at] = uint16_t(pos | (((row16[at] & 0xffu) - pos) << 8));
                pos = fn_apply(row32[at], pos);                  // (the block's last: its composed function, and pos is not used again)
            }
        }
    }
}

// The walk that writes the records: a window's chunks in stream order, the table of the group at hand in LDS.
template <class T>
__global__ __launch_bounds__(64) void k_est_emit(EstParams<T> p) {
    __shared__ uint16_t tab[T::kPad];
    __shared__ uint16_t pre[64];
    __shared__ __attribute__((aligned(16))) typename T::Emit stage;      // the chunk's key records and its range records (Keys16: one buffer)
    uint16_t *buf = stage.out;
    typename T::Rec *kbuf = stage.keys();
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    const uint32_t lo = w * kWindow, hi = min(lo + kWindow, p.total_chunks);
    for (uint32_t c = lo; c < hi; c++) {
        const ChunkRef ck = chunk_ref(p, c);
        const Row gr = group_of(p, c);
        if (c == lo || c == gr.a) {                              // a group's first chunk: its start table; a window's: the row's
            __syncthreads();
            if (c == gr.a) for (uint32_t k = lane; k < T::kKeys; k += 64) tab[k] = uint16_t(start_entry(p, gr.g, k));
            else for (uint32_t k = lane; k < T::kKeys; k += 64) tab[k] = p.row16[size_t(2 * w) * T::kPad + k];
            __syncthreads();
        }
        bool bad = false;
        if constexpr (T::kOneByte) bad = (ck.base & 15) != 0;    // rec_off not a multiple of 16: a bad slice, and nothing of it is written
        const bool store = !bad;                                 // (uniform)
        stage_chunk(p, ck, kbuf, lane);
        for (uint32_t i0 = 0; i0 < ck.padded; i0 += 64) {
            const StepIn s = load_step<T>(kbuf, ck, i0, lane);
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
        if (!T::kOneByte || store)
            for (uint32_t v = lane; v * 8 < ck.padded; v += 64)  // (padded: a multiple of eight, as the chunk's start is)
                reinterpret_cast<uint4 *>(p.recs_out + ck.base)[v] = reinterpret_cast<const uint4 *>(buf)[v];
        if (__ballot(bad) && lane == 0) atomicMin(&p.group_bad[gr.g], ck.s);
        if (c + 1 == gr.b && p.est_out) {
            __syncthreads();
            for (uint32_t k = lane; k < T::kKeys; k += 64) p.est_out[size_t(gr.g) * T::kKeys + k] = tab[k];
        }
    }
}

// a malformed record leaves the later slices of its group without estimators: that slice and every later one of the group
template <class T>
__global__ __launch_bounds__(256) void k_est_status(EstParams<T> p) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.n_slices && i >= p.group_bad[p.slice_group[i]]) p.status[i] = AVR_SLICE_BAD_RECORD;
}

template <class T>
hipError_t est_resolve(hipStream_t s, const Slices &keys, const uint32_t *group_first, uint32_t n_groups, const uint8_t *est_in,
                       uint8_t *est_out, const avr_chunk_plan *pl, void *workspace, uint16_t *recs_out, int32_t *status) {
    const uint32_t n_slices = keys.n_slices, total_chunks = pl->total_chunks;
    if (n_slices == 0 || n_groups == 0) return hipSuccess;
    EstParams<T> p{};
    p.keys = keys.as<typename T::Rec>(); p.rec_off = keys.off; p.n_bins = keys.n_bins; p.group_first = group_first;
    p.est_in = reinterpret_cast<const uint16_t *>(est_in);
    p.est_out = reinterpret_cast<uint16_t *>(est_out);
    p.chunk_base = pl->chunk_base; p.chunk_slice = pl->chunk_slice;
    const EstLayout L = est_layout(n_slices, n_groups, total_chunks, T::kPad);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    p.slice_group = reinterpret_cast<uint32_t *>(ws + L.slice_group);
    p.group_bad = reinterpret_cast<uint32_t *>(ws + L.group_bad);
    p.row32 = reinterpret_cast<uint32_t *>(ws + L.row32);
    p.row16 = reinterpret_cast<uint16_t *>(ws + L.row16);
    p.recs_out = recs_out; p.status = status;
    p.n_slices = n_slices; p.n_groups = n_groups; p.total_chunks = total_chunks;
    const uint32_t n_windows = (total_chunks + est::kWindow - 1) / est::kWindow;
    k_est_prep<T><<<(std::max(n_slices, n_groups) + 255) / 256, 256, 0, s>>>(p);
    if (n_windows) {
        k_est_count<T><<<n_windows, 64, 0, s>>>(p);
        k_est_scan_agg<T><<<n_windows, 256, 0, s>>>(p);
        k_est_scan<T><<<n_windows, 256, 0, s>>>(p);
        k_est_func<T><<<n_windows, 64, 0, s>>>(p);
        k_est_chain_agg<T><<<n_windows, 256, 0, s>>>(p);
        k_est_chain<T><<<n_windows, 256, 0, s>>>(p);
        k_est_emit<T><<<n_windows, 64, 0, s>>>(p);
    }
    k_est_status<T><<<(n_slices + 255) / 256, 256, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_est_resolve(hipStream_t s, const Slices &keys, const uint32_t *group_first, uint32_t n_groups, const uint8_t *est_in,
                              uint8_t *est_out, const avr_chunk_plan *pl, void *workspace, uint16_t *recs_out, int32_t *status) {
    return keys.rec_bytes == 1 ? est_resolve<Keys8>(s, keys, group_first, n_groups, est_in, est_out, pl, workspace, recs_out, status)
                               : est_resolve<Keys16>(s, keys, group_first, n_groups, est_in, est_out, pl, workspace, recs_out, status);
}

}  // namespace avr
