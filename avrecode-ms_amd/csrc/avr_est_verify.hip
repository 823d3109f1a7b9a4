// The estimator checker (avr_est_verify.h): resolved K2 records held to their key records and to each other.  Kernels and launcher.
// Writes first_bad and status only; reads nothing outside a slice's records and their padding to the next multiple of eight (one-byte
// key records: of sixteen).  The kernels that touch a key record or a table are templates on the record's form, as the resolver's are --
// stated here again, the checker includes nothing of the resolver.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "avr_est_verify.h"
#include "avr_internal.h"

namespace avr {
namespace {

using namespace estv;

// Keys16: AVR_KIND_RANGE_KEYS (bin | key << 1, rec_off in records); Keys8: AVR_KIND_RANGE_KEYS8 (bin | dense id << 1, every value a
// key, rec_off in bytes and a multiple of 16 -- a slice whose rec_off is not gets a finding at bin 0 and is not read).
// kKeys: estimators to a table; kStride: a table's stride in LDS and in the workspace; kBallots: bits of a key; kPerLoad: records to a 16-byte load
struct Keys16 {
    using Rec = uint16_t;
    static constexpr uint32_t kKeys = estv::kKeys, kStride = kTabStride, kBallots = 11, kPerLoad = 8;
    static constexpr bool kOneByte = false;
};
struct Keys8 {
    using Rec = uint8_t;
    static constexpr uint32_t kKeys = AVR_EST_KEYS8, kStride = kTabStride8, kBallots = 7, kPerLoad = 16;
    static constexpr bool kOneByte = true;
};
template <class T> __device__ inline bool rec_ok(uint32_t krec) { if constexpr (T::kOneByte) return true; else return key_ok(krec); }

template <class T>
struct EstvParams {
    const typename T::Rec *keys;
    const uint16_t *recs;
    const uint64_t *rec_off;
    const uint32_t *n_bins;
    const uint32_t *group_first;
    const uint16_t *est_in, *est_out;       // {pos, neg} byte pairs read as pos | neg << 8
    const uint32_t *chunk_base, *chunk_slice;
    uint32_t *slice_group;
    uint16_t *tab, *agg;
    int32_t *status;
    uint32_t *first_bad;
    uint32_t n_slices, n_groups, total_chunks;
};

// one chunk: its slice, its first bin in the slice, its bins, its records with the slice's padding, its first record
struct ChunkAt { uint32_t s, start, n, padded; uint64_t base; };
template <class T>
__device__ inline ChunkAt chunk_at(const EstvParams<T> &p, uint32_t c) {
    ChunkAt k;
    k.s = p.chunk_slice[c];
    const uint32_t nb = p.n_bins[k.s], in_slice = c - p.chunk_base[k.s];
    k.start = chunk_start(in_slice);
    k.n = chunk_bins(in_slice, nb);                              // 0 for a chunk that starts at the slice's end (an empty slice's)
    k.padded = padded_bins(k.start, k.n, nb);
    k.base = p.rec_off[k.s] + k.start;
    return k;
}
template <class T>
__device__ inline Group group_at(const EstvParams<T> &p, uint32_t c) {
    Group r;
    r.g = p.slice_group[p.chunk_slice[c]];
    r.a = p.chunk_base[p.group_first[r.g]];
    r.b = p.chunk_base[p.group_first[r.g + 1]];
    return r;
}
template <class T>
__device__ inline uint32_t start_entry(const EstvParams<T> &p, uint32_t g, uint32_t k) {
    return p.est_in ? p.est_in[size_t(g) * T::kKeys + k] : kFresh;
}
template <class T>
__device__ inline bool takes_part(const EstvParams<T> &p, uint32_t s) { return p.status[s] != kBadRecord; }
// one-byte key records: the slice's rec_off is a multiple of 16 (a chunk's start is one)
template <class T>
__device__ inline bool aligned_at(const ChunkAt &ck) { if constexpr (T::kOneByte) return (ck.base & 15) == 0; else return true; }

// the lanes of the wave that hold this lane's key
template <class T>
__device__ inline uint64_t same_key(uint32_t key, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < int(T::kBallots); b++) {
        const bool bit = (key >> b) & 1u;
        const uint64_t bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// slice -> group; no finding yet
template <class T>
__global__ __launch_bounds__(256) void k_estv_prep(EstvParams<T> p) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n_slices) return;
    uint32_t lo = 0, hi = p.n_groups - 1;                        // the last group that starts at or before slice i
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (p.group_first[mid] <= i) lo = mid; else hi = mid - 1;
    }
    p.slice_group[i] = lo;
    p.first_bad[i] = kNone;
}

// per piece of a crossing group and key: what the key's next bin must carry after the piece (0: not met).  Any order: 16-byte loads,
// one LDS atomicMax on position << 16 | next per bin.
template <class T>
__global__ __launch_bounds__(64) void k_estv_last(EstvParams<T> p) {
    __shared__ uint32_t last[T::kStride];
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    Piece pc[2];
    span_pieces(w, kSpan, p.total_chunks, [&](uint32_t c) { return group_at(p, c); }, pc);
    for (int pi = 0; pi < 2; pi++) {
        if (pc[pi].c0 >= pc[pi].c1) continue;
        for (uint32_t k = lane; k < T::kStride; k += 64) last[k] = 0;
        __syncthreads();
        for (uint32_t c = pc[pi].c0; c < pc[pi].c1; c++) {
            const ChunkAt ck = chunk_at(p, c);
            if (!takes_part(p, ck.s) || !aligned_at<T>(ck)) continue;
            const uint4 *ksrc = reinterpret_cast<const uint4 *>(p.keys + ck.base);
            const uint4 *rsrc = reinterpret_cast<const uint4 *>(p.recs + ck.base);
            const uint32_t at = chunk_start(c - pc[pi].c0);      // below 2^16: a piece has at most kSpan chunks
            if constexpr (T::kOneByte) {                         // sixteen key records a load, and their resolved records in two
                for (uint32_t v = lane; v * 16 < ck.n; v += 64) {
                    const uint4 kq = ksrc[v];
                    const uint32_t kw[4] = {kq.x, kq.y, kq.z, kq.w};
#pragma unroll
                    for (uint32_t h = 0; h < 2; h++) {
                        if (v * 16 + h * 8 >= ck.n) break;       // (the slice's resolved records end at its next multiple of eight)
                        const uint4 rq = rsrc[2 * v + h];
                        const uint32_t rw[4] = {rq.x, rq.y, rq.z, rq.w};
#pragma unroll
                        for (uint32_t e = 0; e < 8; e++) {
                            const uint32_t krec = (kw[2 * h + e / 4] >> (8 * (e & 3))) & 0xffu, rrec = (rw[e / 2] >> (16 * (e & 1))) & 0xffffu;
                            const uint32_t i = v * 16 + h * 8 + e;
                            if (i < ck.n) atomicMax(&last[krec >> 1], last_entry(at + i, next_of(rrec, krec)));
                        }
                    }
                }
            } else {
                for (uint32_t v = lane; v * 8 < ck.n; v += 64) {
                    const uint4 kq = ksrc[v], rq = rsrc[v];
                    const uint32_t kw[4] = {kq.x, kq.y, kq.z, kq.w}, rw[4] = {rq.x, rq.y, rq.z, rq.w};
#pragma unroll
                    for (uint32_t e = 0; e < 8; e++) {
                        const uint32_t krec = (kw[e / 2] >> (16 * (e & 1))) & 0xffffu, rrec = (rw[e / 2] >> (16 * (e & 1))) & 0xffffu;
                        if (v * 8 + e < ck.n && key_ok(krec)) atomicMax(&last[krec >> 1], last_entry(at + v * 8 + e, next_of(rrec, krec)));
                    }
                }
            }
        }
        __syncthreads();
        uint16_t *dst = p.tab + size_t(2 * w + pi) * T::kStride;
        for (uint32_t k = lane; k < T::kKeys; k += 64) dst[k] = uint16_t(last[k]);
        __syncthreads();
    }
}

// The walk over a crossing group's pieces, in blocks (avr_est_verify.h): every block's aggregate -- per key the last piece of the
// block that met it -- into the second table of the block's last slot ...
template <class T>
__global__ __launch_bounds__(256) void k_estv_agg(EstvParams<T> p) {
    const uint32_t w = blockIdx.x;
    Piece pc[2];
    BlockHead heads[2];
    span_pieces(w, kSpan, p.total_chunks, [&](uint32_t c) { return group_at(p, c); }, pc);
    span_block_heads(w, kSpan, pc, heads);
    const uint16_t *__restrict__ tab = p.tab;
    uint16_t *__restrict__ agg = p.agg;
    for (int h = 0; h < 2; h++) {
        if (!heads[h].any) continue;
        const PieceSeq seq = heads[h].seq;
        const uint32_t i0 = heads[h].kb * kPieceBlock, i1 = seq.block_end(heads[h].kb);
        for (uint32_t k = threadIdx.x; k < T::kKeys; k += 256) {
            uint32_t a = 0;
#pragma unroll 8
            for (uint32_t i = i0; i < i1; i++) a = then(a, tab[size_t(seq.slot(i)) * T::kStride + k]);
            agg[size_t(seq.slot(i1 - 1)) * T::kStride + k] = uint16_t(a);
        }
    }
}
// ... then every piece's table turned, in place, into the table at the piece's START
template <class T>
__global__ __launch_bounds__(256) void k_estv_start(EstvParams<T> p) {
    const uint32_t w = blockIdx.x;
    Piece pc[2];
    BlockHead heads[2];
    span_pieces(w, kSpan, p.total_chunks, [&](uint32_t c) { return group_at(p, c); }, pc);
    span_block_heads(w, kSpan, pc, heads);
    const uint16_t *__restrict__ agg = p.agg;
    uint16_t *tab = p.tab;
    for (int h = 0; h < 2; h++) {
        if (!heads[h].any) continue;
        const PieceSeq seq = heads[h].seq;
        const uint32_t i0 = heads[h].kb * kPieceBlock, i1 = seq.block_end(heads[h].kb);
        for (uint32_t k = threadIdx.x; k < T::kKeys; k += 256) {
            uint32_t cur = start_entry(p, heads[h].g, k);
#pragma unroll 8
            for (uint32_t kb = 0; kb < heads[h].kb; kb++) cur = then(cur, agg[size_t(seq.slot(seq.block_end(kb) - 1)) * T::kStride + k]);
            uint32_t i = i0;
            for (; i + 8 <= i1; i += 8) {                        // the addresses do not depend on cur: eight loads in flight
                uint32_t nx[8];
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) nx[j] = tab[size_t(seq.slot(i + j)) * T::kStride + k];
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) { tab[size_t(seq.slot(i + j)) * T::kStride + k] = uint16_t(cur); cur = then(cur, nx[j]); }
            }
            for (; i < i1; i++) {
                const size_t at = size_t(seq.slot(i)) * T::kStride + k;
                const uint32_t nx = tab[at];
                tab[at] = uint16_t(cur);
                cur = then(cur, nx);
            }
        }
    }
}

// The check: a span's chunks in stream order, the table of the group at hand in LDS, 64 bins a step.
template <class T>
__global__ __launch_bounds__(64) void k_estv_check(EstvParams<T> p) {
    __shared__ uint16_t tab[T::kStride];
    __shared__ __attribute__((aligned(16))) typename T::Rec kbuf[kChunk];
    __shared__ __attribute__((aligned(16))) uint16_t rbuf[kChunk];
    const uint32_t w = blockIdx.x, lane = threadIdx.x;
    const uint32_t lo = w * kSpan, hi = min(lo + kSpan, p.total_chunks);
    for (uint32_t c = lo; c < hi; c++) {
        const ChunkAt ck = chunk_at(p, c);
        const Group gr = group_at(p, c);
        if (c == lo || c == gr.a) {                              // a group's first chunk: its start table; a span's: the piece's
            __syncthreads();
            if (c == gr.a) for (uint32_t k = lane; k < T::kKeys; k += 64) tab[k] = uint16_t(start_entry(p, gr.g, k));
            else for (uint32_t k = lane; k < T::kKeys; k += 64) tab[k] = p.tab[size_t(2 * w) * T::kStride + k];
            __syncthreads();
        }
        if (!takes_part(p, ck.s)) continue;                      // (uniform; and so is every later slice of the group)
        if (!aligned_at<T>(ck)) {                                // (uniform) one-byte key records only
            if (lane == 0) atomicMin(&p.first_bad[ck.s], 0u);
            continue;
        }
        __syncthreads();                                         // the chunk before is done with the buffers
        for (uint32_t v = lane; v * T::kPerLoad < ck.n; v += 64)
            reinterpret_cast<uint4 *>(kbuf)[v] = reinterpret_cast<const uint4 *>(p.keys + ck.base)[v];
        for (uint32_t v = lane; v * 8 < ck.padded; v += 64)      // (padded: a multiple of eight, as the chunk's start is)
            reinterpret_cast<uint4 *>(rbuf)[v] = reinterpret_cast<const uint4 *>(p.recs + ck.base)[v];
        __syncthreads();
        bool pad_bad = false;
        for (uint32_t i0 = 0; i0 < ck.padded; i0 += 64) {
            const uint32_t idx = i0 + lane;
            const bool in_chunk = idx < ck.n;
            const uint32_t krec = in_chunk ? kbuf[idx] : 0u, rrec = idx < ck.padded ? rbuf[idx] : 0u;
            const bool valid = in_chunk && rec_ok<T>(krec);
            const uint32_t key = krec >> 1;
            const uint64_t mask = same_key<T>(key, valid);
            const uint32_t nx = next_of(rrec, krec);
            const int from = valid ? lower_lane(mask, lane) : -1;
            const uint32_t left = uint32_t(__shfl(int(nx), from < 0 ? int(lane) : from));
            const uint32_t expected = from >= 0 ? left : valid ? tab[key] : 0u;
            const bool bad = in_chunk && bin_bad(krec, rrec, expected);
            pad_bad |= !in_chunk && rrec != 0;                   // condition 4 (rrec is 0 beyond `padded`)
            __syncthreads();                                     // every lane has read the table
            if (valid && (mask >> lane) == 1) tab[key] = uint16_t(nx);      // the key's last lane of the step
            __syncthreads();
            const uint64_t bads = __ballot(bad);
            if (bads && lane == uint32_t(__builtin_ctzll(bads))) atomicMin(&p.first_bad[ck.s], ck.start + idx);
        }
        if (__ballot(pad_bad) && lane == 0) atomicMin(&p.first_bad[ck.s], p.n_bins[ck.s]);
        if (c + 1 == gr.b && p.est_out) {                        // condition 5 (this chunk's slice is the group's last, and it takes part)
            bool diff = false;
            for (uint32_t k = lane; k < T::kKeys; k += 64) diff |= tab[k] != p.est_out[size_t(gr.g) * T::kKeys + k];
            if (__ballot(diff) && lane == 0) atomicMin(&p.first_bad[ck.s], p.n_bins[ck.s]);
        }
    }
}

// a slice with a finding goes from AVR_SLICE_OK to AVR_SLICE_VERIFY_FAILED; any other status stays
template <class T>
__global__ __launch_bounds__(256) void k_estv_status(EstvParams<T> p) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.n_slices && p.first_bad[i] != kNone && p.status[i] == kOk) p.status[i] = kVerifyFailed;
}

#ifdef AVR_TEST_HOOKS
// Test build only (est_flip, avr_internal.h): one added to neg of one resolved record (neg <= 96: the field stays valid and non-zero)
__global__ void k_est_flip(uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins, uint32_t slice, uint32_t bin) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && bin < n_bins[slice]) recs[rec_off[slice] + bin] += 0x100u;
}
#endif

}  // namespace

template <class T>
static hipError_t est_verify(hipStream_t s, const Slices &keys, const uint16_t *recs, const uint32_t *group_first, uint32_t n_groups,
                             const uint8_t *est_in, const uint8_t *est_out, const avr_chunk_plan *pl, void *workspace, int32_t *status,
                             uint32_t *first_bad) {
    const uint32_t n_slices = keys.n_slices, total_chunks = pl->total_chunks;
    if (n_slices == 0 || n_groups == 0) return hipSuccess;
    EstvParams<T> p{};
    p.keys = keys.as<typename T::Rec>(); p.recs = recs; p.rec_off = keys.off; p.n_bins = keys.n_bins; p.group_first = group_first;
    p.est_in = reinterpret_cast<const uint16_t *>(est_in);
    p.est_out = reinterpret_cast<const uint16_t *>(est_out);
    p.chunk_base = pl->chunk_base; p.chunk_slice = pl->chunk_slice;
    const EstVerifyLayout L = est_verify_layout(n_slices, total_chunks, T::kStride);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    p.slice_group = reinterpret_cast<uint32_t *>(ws + L.slice_group);
    p.tab = reinterpret_cast<uint16_t *>(ws + L.tab);
    p.agg = reinterpret_cast<uint16_t *>(ws + L.agg);
    p.status = status; p.first_bad = first_bad;
    p.n_slices = n_slices; p.n_groups = n_groups; p.total_chunks = total_chunks;
    const uint32_t n_spans = (total_chunks + kSpan - 1) / kSpan;
    k_estv_prep<T><<<(n_slices + 255) / 256, 256, 0, s>>>(p);
    if (n_spans) {
        k_estv_last<T><<<n_spans, 64, 0, s>>>(p);
        k_estv_agg<T><<<n_spans, 256, 0, s>>>(p);
        k_estv_start<T><<<n_spans, 256, 0, s>>>(p);
        k_estv_check<T><<<n_spans, 64, 0, s>>>(p);
    }
    k_estv_status<T><<<(n_slices + 255) / 256, 256, 0, s>>>(p);
    return hipGetLastError();
}

hipError_t launch_est_verify(hipStream_t s, const Slices &keys, const uint16_t *recs, const uint32_t *group_first, uint32_t n_groups,
                             const uint8_t *est_in, const uint8_t *est_out, const avr_chunk_plan *pl, void *workspace, int32_t *status,
                             uint32_t *first_bad) {
    return keys.rec_bytes == 1 ? est_verify<Keys8>(s, keys, recs, group_first, n_groups, est_in, est_out, pl, workspace, status, first_bad)
                               : est_verify<Keys16>(s, keys, recs, group_first, n_groups, est_in, est_out, pl, workspace, status, first_bad);
}

#ifdef AVR_TEST_HOOKS
hipError_t launch_est_flip(hipStream_t s, uint16_t *recs, const uint64_t *rec_off, const uint32_t *n_bins, uint32_t slice, uint32_t bin) {
    hipLaunchKernelGGL(k_est_flip, dim3(1), dim3(64), 0, s, recs, rec_off, n_bins, slice, bin);
    return hipGetLastError();
}
#endif

}  // namespace avr
