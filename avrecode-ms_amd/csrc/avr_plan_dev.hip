// The device planner for gfx950 (MI355X): a batch's plan from lengths that lie in HBM, and its coded bytes compacted, with no host
// round trip (avr_plan_chunks_device, avr_plan_tiles_device, avr_compact_device, avr_finish_device; layouts and bounds in
// avr_plan_dev.h).  The per-slice rules are avr_plan.h's own functions.  Five kernels' worth of ideas, none of which lets a workgroup
// wait on another workgroup of its launch: every dependence between workgroups is a kernel boundary on the caller's stream.
//
//   scan      k_reduce / k_apply   an exclusive prefix sum over Q 64-bit quantities at once (the chunk plan sums seven per slice in one
//             sweep).  A workgroup of 256 threads takes 1024 entries, four to a thread: the threads' sums are scanned inside each wave by
//             shuffles and across the four waves through 4 x Q words of LDS.  Reduce per workgroup, then the workgroups' sums the same
//             way (as many levels as there are sums: 2^31 entries need three), then apply -- the prefix of a level is added while the
//             level below is scanned.  The entry that closes the array (index n) and the totals are written by the thread that holds
//             the last entry.
//   expand    k_expand             chunk_slice / blk_slice: one thread per CHUNK, which finds its slice by a binary search over
//             chunk_base (n + 1 entries, the first levels of which stay in cache); the stores of a wave are 256 contiguous bytes, and a
//             slice of four million chunks is four million threads' work, not one lane's.  The grid is sized by the caller's cap, the
//             loop ends at min(total, cap): nothing is written at or past the cap whatever n_bins holds.
//   sort      k_sort_hist / k_hist_reduce / k_hist_scan / k_sort_scatter   stable LSD radix sort of (~n_bins, index), eight bits a
//             pass.  At most 1024 workgroups, each with a run of consecutive keys in tiles of 256: a pass counts the digits per
//             workgroup ([digit][workgroup], LDS atomics), scans that table (two launches: sums per 1024, then each 1024 with the sums
//             in front of it), and scatters.  A key's rank among equal digits: inside its wave by ballots (eight ballots give the lanes
//             with the same digit, a popcount of those below gives the rank), across the tile's four waves by their counts in LDS,
//             across tiles by a running offset per digit in LDS -- keys keep the order they came in, which is what makes LSD passes a
//             sort and the whole stable.  Pass 0 reads n_bins itself, pass 3 writes `order`.
//   copy      k_compact_wide       a wave per slice: the destination is brought to an 8-byte boundary by up to seven single bytes, the
//             body goes in 8-byte words (aligned stores; aligned loads of the two source words a destination word straddles, funnel
//             shifted), up to seven bytes finish.  A wave's body step is 512 contiguous bytes on both sides.
//   finish    k_finish_lengths / k_finish_copy   avr_finish_device: the copy with the decompressor's epilogue in it (avr_finish.h: stop
//             byte, tail patch, emulation prevention).  Escaping changes lengths, so they are a pass of their own, a wave per slice: a
//             lane makes of its 8-byte word a map from the escape rule's three entry states to (exit state, escapes), the wave composes
//             the maps in lane order by shuffles and carries state and count from trip to trip.  The scan above makes dense_off of the
//             lengths; the second pass walks again, each lane knowing its entry state and the escapes in front of it, and stores an
//             escaped slice by bytes -- a slice without escapes goes the wide copy's way, the word with the special byte through
//             patched_word.
//
// Resource use by the compiler's report (-Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md, "Planning on the device".
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avr_finish.h"
#include "avr_internal.h"
#include "avr_plan.h"
#include "avr_plan_dev.h"

namespace avr {
namespace plan_dev {

template <int Q>
struct Vec { uint64_t v[Q]; };

template <int Q>
__device__ inline void vadd(Vec<Q> &a, const Vec<Q> &b) {
#pragma unroll
    for (int q = 0; q < Q; q++) a.v[q] += b.v[q];
}

__device__ inline uint64_t shfl_up64(uint64_t x, uint32_t d) {
    const uint32_t lo = uint32_t(__shfl_up(int(uint32_t(x)), d, 64)), hi = uint32_t(__shfl_up(int(uint32_t(x >> 32)), d, 64));
    return uint64_t(hi) << 32 | lo;
}

// The sum of `mine` over the threads in front of this one (thread order) and, in `total`, over the whole workgroup of 256.  Every
// thread of the workgroup calls it; lds: four entries, free again on return.
template <int Q>
__device__ inline Vec<Q> block_exclusive(const Vec<Q> &mine, Vec<Q> *lds, Vec<Q> &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Vec<Q> inc = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const uint64_t other = shfl_up64(inc.v[q], d);
            if (lane >= d) inc.v[q] += other;
        }
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    Vec<Q> ex;
#pragma unroll
    for (int q = 0; q < Q; q++) { ex.v[q] = inc.v[q] - mine.v[q]; total.v[q] = 0; }
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
        const Vec<Q> t = lds[w];
        if (w < wave) vadd(ex, t);
        vadd(total, t);
    }
    __syncthreads();
    return ex;
}

// ------------------------------------------------------------------ the scan
// Src: operator()(i) -> Vec<Q>, entry i's quantities.  Sink: put(i, prefix) for every i < n, finish(n, total) once.

template <int Q>
struct ArraySrc {
    const Vec<Q> *a;
    __device__ Vec<Q> operator()(uint64_t i) const { return a[i]; }
};
template <int Q>
struct ArraySink {                                               // in place: a thread has read its four entries before it writes them
    Vec<Q> *a;
    __device__ void put(uint64_t i, const Vec<Q> &prefix) const { a[i] = prefix; }
    __device__ void finish(uint64_t, const Vec<Q> &) const {}
};

template <int Q, class Src>
__global__ __launch_bounds__(256) void k_reduce(Src src, uint64_t n, Vec<Q> *sums) {
    __shared__ Vec<Q> lds[4];
    const uint64_t first = uint64_t(blockIdx.x) * kScanTile + threadIdx.x * 4u;
    Vec<Q> mine = {};
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
        if (first + j < n) vadd(mine, src(first + j));
    Vec<Q> total;
    block_exclusive(mine, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// `up`: the exclusive prefix of every workgroup's sum (the level above, scanned), or null where one workgroup has it all.
template <int Q, class Src, class Sink>
__global__ __launch_bounds__(256) void k_apply(Src src, Sink sink, uint64_t n, const Vec<Q> *up) {
    __shared__ Vec<Q> lds[4];
    const uint64_t first = uint64_t(blockIdx.x) * kScanTile + threadIdx.x * 4u;
    Vec<Q> item[4], mine = {};
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        item[j] = Vec<Q>{};
        if (first + j < n) item[j] = src(first + j);
        vadd(mine, item[j]);
    }
    Vec<Q> total;
    Vec<Q> at = block_exclusive(mine, lds, total);
    if (up) vadd(at, up[blockIdx.x]);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint64_t i = first + j;
        if (i < n) {
            sink.put(i, at);
            vadd(at, item[j]);
            if (i + 1 == n) sink.finish(n, at);
        }
    }
    if (n == 0 && blockIdx.x == 0 && threadIdx.x == 0) sink.finish(0, Vec<Q>{});
}

template <int Q, class Src, class Sink>
hipError_t scan(hipStream_t s, const Src &src, const Sink &sink, uint64_t n, uint8_t *ws_sums) {
    const ScanLevels lv = scan_levels(n, sizeof(Vec<Q>));
    const dim3 block(256);
    if (lv.count == 0) {
        hipLaunchKernelGGL((k_apply<Q, Src, Sink>), dim3(1), block, 0, s, src, sink, n, static_cast<const Vec<Q> *>(nullptr));
        return hipGetLastError();
    }
    Vec<Q> *sums[4];
    for (uint32_t j = 0; j < lv.count; j++) sums[j] = reinterpret_cast<Vec<Q> *>(ws_sums + lv.off[j]);
    hipLaunchKernelGGL((k_reduce<Q, Src>), dim3(uint32_t(lv.n[0])), block, 0, s, src, n, sums[0]);
    for (uint32_t j = 0; j + 1 < lv.count; j++)
        hipLaunchKernelGGL((k_reduce<Q, ArraySrc<Q>>), dim3(uint32_t(lv.n[j + 1])), block, 0, s, ArraySrc<Q>{sums[j]}, lv.n[j], sums[j + 1]);
    const uint32_t top = lv.count - 1;                            // at most 1024 sums: one workgroup
    hipLaunchKernelGGL((k_apply<Q, ArraySrc<Q>, ArraySink<Q>>), dim3(1), block, 0, s, ArraySrc<Q>{sums[top]}, ArraySink<Q>{sums[top]}, lv.n[top],
                       static_cast<const Vec<Q> *>(nullptr));
    for (uint32_t j = top; j-- > 0;)
        hipLaunchKernelGGL((k_apply<Q, ArraySrc<Q>, ArraySink<Q>>), dim3(uint32_t(lv.n[j + 1])), block, 0, s, ArraySrc<Q>{sums[j]}, ArraySink<Q>{sums[j]},
                           lv.n[j], static_cast<const Vec<Q> *>(sums[j + 1]));
    hipLaunchKernelGGL((k_apply<Q, Src, Sink>), dim3(uint32_t(lv.n[0])), block, 0, s, src, sink, n, static_cast<const Vec<Q> *>(sums[0]));
    return hipGetLastError();
}

// ------------------------------------------------------------------ the chunk plan

enum { kOut, kRec, kChunks, kDig, kRes, kBlocks, kBins };        // a slice's seven quantities

struct PlanSrc {
    const uint32_t *n_bins;
    uint32_t rec_round;
    __device__ Vec<kPlanSums> operator()(uint64_t i) const {
        const uint64_t nb = n_bins[i];
        Vec<kPlanSums> v;
        v.v[kOut] = slice_out_bytes(nb);
        v.v[kRec] = (nb + rec_round - 1) & ~uint64_t(rec_round - 1);
        v.v[kChunks] = slice_chunks(nb);
        v.v[kDig] = slice_digit_sums(nb);
        v.v[kRes] = slice_work_bytes(nb);
        v.v[kBlocks] = slice_blocks(nb);
        v.v[kBins] = nb;
        return v;
    }
};

struct PlanSink {
    avr_plan_arrays a;
    int level;
    avr_plan_totals *totals, *ws_totals;                         // the caller's, and the copy the expansion reads
    __device__ void put(uint64_t i, const Vec<kPlanSums> &p) const {
        a.out_off[i] = p.v[kOut];
        if (a.rec_off) a.rec_off[i] = p.v[kRec];
        if (level >= AVR_PLAN_CHUNKS) a.chunk_base[i] = uint32_t(p.v[kChunks]);
        if (level >= AVR_PLAN_CODES) a.dig_off[i] = p.v[kDig];
        if (level >= AVR_PLAN_K1P) {
            a.res_off[i] = p.v[kRes];
            a.blk_base[i] = uint32_t(p.v[kBlocks]);
        }
    }
    __device__ void finish(uint64_t n, const Vec<kPlanSums> &t) const {
        put(n, t);
        for (int copy = 0; copy < 2; copy++) {                    // every field of this call's, none of the tile plan's; a total above the
            avr_plan_totals *to = copy ? ws_totals : totals;     // level is 0, as fill_plan leaves the array empty
            to->total_bins = t.v[kBins];
            to->out_total = t.v[kOut];
            to->rec_total = a.rec_off ? t.v[kRec] : 0;
            to->total_chunks = level >= AVR_PLAN_CHUNKS ? t.v[kChunks] : 0;
            to->dig_total = level >= AVR_PLAN_CODES ? t.v[kDig] : 0;
            to->res_total = level >= AVR_PLAN_K1P ? t.v[kRes] : 0;
            to->total_blocks = level >= AVR_PLAN_K1P ? t.v[kBlocks] : 0;
        }
    }
};

// slice_of[k] = the slice whose run [base[i], base[i + 1]) holds k, for k < min(*total, cap).  Every slice has a chunk, so base rises
// strictly and the search has one answer.  (A total of 2^32 and more has wrapped base: the entries written are then of no use -- and
// avr_chunk_plan_from refuses the plan -- but they are indices below n written below the cap.)
__global__ __launch_bounds__(256) void k_expand(const uint32_t *base, uint32_t n, const uint64_t *total, uint64_t cap, uint32_t *slice_of) {
    const uint64_t end = *total < cap ? *total : cap;
    for (uint64_t k = uint64_t(blockIdx.x) * 256u + threadIdx.x; k < end; k += uint64_t(gridDim.x) * 256u) {
        uint32_t lo = 0, hi = n;                                 // the answer is in [lo, hi)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (uint64_t(base[mid]) <= k) lo = mid;
            else hi = mid;
        }
        slice_of[k] = lo;
    }
}

static void launch_expand(hipStream_t s, const uint32_t *base, uint32_t n, const uint64_t *total, uint64_t cap, uint32_t *slice_of) {
    if (n == 0 || cap == 0) return;
    const uint64_t blocks = (cap + 255) / 256;
    hipLaunchKernelGGL(k_expand, dim3(uint32_t(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, base, n, total, cap, slice_of);
}

// ------------------------------------------------------------------ the tile plan: the sort

__device__ inline uint32_t sort_key(const uint32_t *keys, const uint32_t *n_bins, uint64_t i) { return keys ? keys[i] : ~n_bins[i]; }   // longest first

__global__ __launch_bounds__(256) void k_sort_hist(const uint32_t *keys, const uint32_t *n_bins, uint32_t n, uint32_t per_block, uint32_t shift,
                                                   uint32_t *hist) {
    __shared__ uint32_t h[kSortDigits];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t begin = uint64_t(blockIdx.x) * per_block, end = begin + per_block < n ? begin + per_block : n;
    for (uint64_t i = begin + threadIdx.x; i < end; i += 256) atomicAdd(&h[(sort_key(keys, n_bins, i) >> shift) & 255u], 1u);
    __syncthreads();
    hist[threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// the table's sums per 1024 entries, then every 1024 scanned with the sums in front of it (at most 256 of them: one entry a thread)
__global__ __launch_bounds__(256) void k_hist_reduce(const uint32_t *hist, uint32_t entries, uint32_t *sums) {
    __shared__ Vec<1> lds[4];
    const uint32_t first = blockIdx.x * kScanTile + threadIdx.x * 4u;
    Vec<1> mine = {};
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
        if (first + j < entries) mine.v[0] += hist[first + j];
    Vec<1> total;
    block_exclusive(mine, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = uint32_t(total.v[0]);
}

__global__ __launch_bounds__(256) void k_hist_scan(uint32_t *hist, uint32_t entries, const uint32_t *sums) {
    __shared__ Vec<1> lds[4];
    Vec<1> before = {}, front, total;
    if (threadIdx.x < blockIdx.x) before.v[0] = sums[threadIdx.x];
    block_exclusive(before, lds, front);                         // front: the sum of the workgroups before this one
    const uint32_t first = blockIdx.x * kScanTile + threadIdx.x * 4u;
    uint32_t item[4];
    Vec<1> mine = {};
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        item[j] = first + j < entries ? hist[first + j] : 0u;
        mine.v[0] += item[j];
    }
    uint32_t at = uint32_t(block_exclusive(mine, lds, total).v[0] + front.v[0]);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (first + j < entries) hist[first + j] = at;
        at += item[j];
    }
}

__global__ __launch_bounds__(256) void k_sort_scatter(const uint32_t *keys_in, const uint32_t *n_bins, const uint32_t *vals_in, uint32_t n,
                                                      uint32_t per_block, uint32_t shift, const uint32_t *hist, uint32_t *keys_out,
                                                      uint32_t *vals_out) {
    __shared__ uint32_t run[kSortDigits];                        // where this workgroup's next key of each digit goes
    __shared__ uint32_t cnt[4][kSortDigits];                     // a tile's keys of each digit, per wave
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    run[t] = hist[t * gridDim.x + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) cnt[w][t] = 0;
    __syncthreads();
    const uint64_t begin = uint64_t(blockIdx.x) * per_block, end = begin + per_block < n ? begin + per_block : n;
    for (uint64_t tile = begin; tile < end; tile += kSortTile) { // the same trip count for every thread of the workgroup
        const uint64_t i = tile + t;
        const bool valid = i < end;
        const uint32_t key = valid ? sort_key(keys_in, n_bins, i) : 0u, d = (key >> shift) & 255u;
        uint64_t same = __ballot(valid);                         // the wave's lanes that hold a key with this lane's digit
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(valid && bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = uint32_t(__popcll(same & ((uint64_t(1) << lane) - 1)));
        if (valid && rank == 0) cnt[wave][d] = uint32_t(__popcll(same));
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + rank;
            for (uint32_t w = 0; w < wave; w++) pos += cnt[w][d];
            if (pos < n) {                                       // (always, for lengths that do not change under the call)
                if (keys_out) keys_out[pos] = key;
                vals_out[pos] = vals_in ? vals_in[i] : uint32_t(i);
            }
        }
        __syncthreads();
        run[t] += cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) cnt[w][t] = 0;
        __syncthreads();
    }
}

// a tile is as long as its first -- its longest -- slice
struct TileSrc {
    const uint32_t *n_bins, *order;
    uint32_t n, records_per_chunk;
    __device__ Vec<1> operator()(uint64_t t) const {
        const uint32_t first = order[t * 64];
        const uint64_t nb = first < n ? n_bins[first] : 0u;
        return Vec<1>{{(nb + records_per_chunk - 1) / records_per_chunk * 64}};
    }
};
struct TileSink {
    uint64_t *tile_off;
    avr_plan_totals *totals;
    __device__ void put(uint64_t t, const Vec<1> &p) const { tile_off[t] = p.v[0]; }
    __device__ void finish(uint64_t n_tiles, const Vec<1> &p) const {
        tile_off[n_tiles] = p.v[0];
        totals->tile_chunks = p.v[0];
    }
};

// ------------------------------------------------------------------ compaction

struct LenSrc {                                                  // what a slice has to give: its length, no more than its region
    const uint64_t *out_off;
    const uint32_t *out_len;
    __device__ Vec<1> operator()(uint64_t i) const {
        const uint64_t cap = out_off[i + 1] - out_off[i], len = out_len[i];
        return Vec<1>{{len < cap ? len : cap}};
    }
};
struct LenSink {
    uint64_t *dense_off;
    __device__ void put(uint64_t i, const Vec<1> &p) const { dense_off[i] = p.v[0]; }
    __device__ void finish(uint64_t n, const Vec<1> &p) const { dense_off[n] = p.v[0]; }
};

__global__ __launch_bounds__(256) void k_compact_wide(const uint8_t *out, const uint64_t *out_off, uint32_t n_slices, uint8_t *dense,
                                                      uint64_t dense_capacity, const uint64_t *dense_off) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slice = blockIdx.x * 4u + (threadIdx.x >> 6);  // the same for a wave's 64 lanes
    if (slice >= n_slices) return;
    const uint64_t d0 = dense_off[slice], d1 = dense_off[slice + 1], len = d1 - d0;
    if (len == 0 || d1 > dense_capacity || d1 < d0) return;      // a slice is copied whole or not at all
    const uint8_t *src = out + out_off[slice];
    uint8_t *dst = dense + d0;
    const uint64_t to_word = (8u - uint32_t(reinterpret_cast<uintptr_t>(dst) & 7u)) & 7u, head = to_word < len ? to_word : len;
    if (lane < head) dst[lane] = src[lane];
    const uint64_t words = (len - head) >> 3, tail = (len - head) & 7u;
    const uint8_t *s = src + head;
    uint64_t *d = reinterpret_cast<uint64_t *>(dst + head);
    const uint32_t skew = uint32_t(reinterpret_cast<uintptr_t>(s) & 7u);
    const uint64_t *sw = reinterpret_cast<const uint64_t *>(s - skew);    // the aligned word that holds s[0]: every word read below holds a byte of the slice
    if (skew == 0) {
#pragma unroll 4
        for (uint64_t w = lane; w < words; w += 64) d[w] = sw[w];
    } else {
        const uint32_t down = 8 * skew, up = 64 - down;
#pragma unroll 4
        for (uint64_t w = lane; w < words; w += 64) d[w] = sw[w] >> down | sw[w + 1] << up;
    }
    if (lane < tail) dst[head + 8 * words + lane] = src[head + 8 * words + lane];
}

// ------------------------------------------------------------------ the epilogue: compaction with the tail patch and the escapes

struct FinishIn {
    const uint8_t *out;
    const uint64_t *out_off;
    const uint32_t *out_len;
    const int32_t *status;                                       // or null: every slice is sound
    const uint32_t *finish;
};

struct FinishSlice {
    const uint64_t *base;                                        // the aligned word that holds the slice's first byte
    uint32_t skew, word;
    finish::Shape shape;
};

// false: the slice gives no bytes.  The same for a wave's 64 lanes.
__device__ inline bool finish_slice(const FinishIn &in, uint32_t slice, FinishSlice &f) {
    if (in.status && in.status[slice] != AVR_SLICE_OK) return false;
    const uint64_t cap = in.out_off[slice + 1] - in.out_off[slice], len = in.out_len[slice];
    const uint32_t L = uint32_t(len < cap ? len : cap);
    const uint8_t *src = in.out + in.out_off[slice];
    f.word = in.finish[slice];
    f.shape = finish::shape_of(L, L ? src[L - 1] : 0u, f.word);
    f.skew = uint32_t(reinterpret_cast<uintptr_t>(src) & 7u);
    f.base = reinterpret_cast<const uint64_t *>(src - f.skew);
    return true;
}

__device__ inline finish::Xfer shfl_up_xfer(const finish::Xfer &x, uint32_t d) {
    return finish::Xfer{uint32_t(__shfl_up(int(x.exit), d, 64)), uint32_t(__shfl_up(int(x.cnt), d, 64))};
}

// One walk over a slice's patched bytes, a word per lane and 512 bytes per trip: the lanes' runs composed in lane order, the state
// and the escapes carried from trip to trip.  kWrite: every lane escapes its run to where it belongs in dst[0, end).  Returns the
// slice's escapes; every lane of the wave calls it.
template <bool kWrite>
__device__ inline uint64_t finish_walk(const FinishSlice &f, uint32_t lane, uint8_t *dst, uint64_t end) {
    uint32_t z = finish::zeros_before(f.word);
    uint64_t escapes = 0;
    const uint64_t R = f.shape.R;
    for (uint64_t k0 = 0; k0 < R; k0 += finish::kTripBytes) {   // the same trip count for every lane
        const uint64_t k = k0 + 8u * lane;
        const uint32_t n = k < R ? (R - k < 8 ? uint32_t(R - k) : 8u) : 0u;
        const uint64_t word = n ? finish::patched_word(f.base, f.skew, k, f.shape) : 0;
        finish::Xfer inc = finish::run_of(word, n);
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const finish::Xfer front = shfl_up_xfer(inc, d);
            if (lane >= d) inc = finish::then(front, inc);
        }
        finish::Xfer ex = shfl_up_xfer(inc, 1);
        if (lane == 0) ex = finish::identity();
        if (kWrite) finish::emit_run(word, n, finish::exit_of(ex, z), dst, k + escapes + finish::count_of(ex, z), end);
        const finish::Xfer all{uint32_t(__shfl(int(inc.exit), 63, 64)), uint32_t(__shfl(int(inc.cnt), 63, 64))};
        escapes += finish::count_of(all, z);
        z = finish::exit_of(all, z);
    }
    return escapes;
}

// pass 1: lens[slice] = the bytes slice gives in the end
__global__ __launch_bounds__(256) void k_finish_lengths(FinishIn in, uint32_t n_slices, uint64_t *lens) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slice = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (slice >= n_slices) return;
    FinishSlice f;
    uint64_t len = 0;
    if (finish_slice(in, slice, f))
        len = finish::final_length(f.shape, AVR_FINISH_ESCAPE(f.word) ? finish_walk<false>(f, lane, nullptr, 0) : 0);
    if (lane == 0) lens[slice] = len;
}

// pass 2: a slice without escapes goes as k_compact_wide's slices go, the word that holds the special byte through patched_word; an
// escaped one by bytes
__global__ __launch_bounds__(256) void k_finish_copy(FinishIn in, uint32_t n_slices, uint8_t *dense, uint64_t dense_capacity, const uint64_t *dense_off) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slice = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (slice >= n_slices) return;
    const uint64_t d0 = dense_off[slice], d1 = dense_off[slice + 1], len = d1 - d0;
    if (len == 0 || d1 > dense_capacity || d1 < d0) return;      // a slice is written whole or not at all
    FinishSlice f;
    if (!finish_slice(in, slice, f)) return;
    uint8_t *dst = dense + d0;
    if (AVR_FINISH_ESCAPE(f.word)) {
        finish_walk<true>(f, lane, dst, len);
        return;
    }
    const uint64_t to_word = (8u - uint32_t(reinterpret_cast<uintptr_t>(dst) & 7u)) & 7u, head = to_word < len ? to_word : len;
    if (lane < head) dst[lane] = uint8_t(finish::patched_word(f.base, f.skew, 0, f.shape) >> (8 * lane));
    const uint64_t words = (len - head) >> 3, tail = (len - head) & 7u;
    uint64_t *d = reinterpret_cast<uint64_t *>(dst + head);
    // The words that lie whole in front of the special byte and of the slice's end go as k_compact_wide's do; the one behind them, if
    // there is one, through patched_word.
    const uint64_t plain = finish::plain_words(f.shape, head, words);
    const uint8_t *s = reinterpret_cast<const uint8_t *>(f.base) + f.skew + head;
    const uint32_t skew = uint32_t(reinterpret_cast<uintptr_t>(s) & 7u);
    const uint64_t *sw = reinterpret_cast<const uint64_t *>(s - skew);    // every word read below holds a byte of the slice
    if (skew == 0) {
#pragma unroll 4
        for (uint64_t w = lane; w < plain; w += 64) d[w] = sw[w];
    } else {
        const uint32_t down = 8 * skew, up = 64 - down;
#pragma unroll 4
        for (uint64_t w = lane; w < plain; w += 64) d[w] = sw[w] >> down | sw[w + 1] << up;
    }
    for (uint64_t w = plain + lane; w < words; w += 64) d[w] = finish::patched_word(f.base, f.skew, head + 8 * w, f.shape);
    if (lane < tail) dst[head + 8 * words + lane] = uint8_t(finish::patched_word(f.base, f.skew, head + 8 * words, f.shape) >> (8 * lane));
}

}  // namespace plan_dev

using namespace plan_dev;

hipError_t launch_plan_chunks(hipStream_t s, const uint32_t *n_bins, uint32_t n_slices, int level, const avr_plan_arrays &arrays, void *ws,
                              avr_plan_totals *totals) {
    const ChunksLayout L = chunks_layout(n_slices);
    uint8_t *w = static_cast<uint8_t *>(ws);
    avr_plan_totals *ws_totals = reinterpret_cast<avr_plan_totals *>(w + L.totals);
    if (hipError_t e = scan<kPlanSums>(s, PlanSrc{n_bins, arrays.rec_round}, PlanSink{arrays, level, totals, ws_totals}, n_slices, w + L.sums); e != hipSuccess)
        return e;
    if (level >= AVR_PLAN_CHUNKS) launch_expand(s, arrays.chunk_base, n_slices, &ws_totals->total_chunks, arrays.cap_chunks, arrays.chunk_slice);
    if (level >= AVR_PLAN_K1P) launch_expand(s, arrays.blk_base, n_slices, &ws_totals->total_blocks, arrays.cap_blocks, arrays.blk_slice);
    return hipGetLastError();
}

hipError_t launch_plan_tiles(hipStream_t s, const uint32_t *n_bins, uint32_t n_slices, uint32_t records_per_chunk, uint32_t *order,
                             uint64_t *tile_off, void *ws, avr_plan_totals *totals) {
    const TilesLayout L = tiles_layout(n_slices);
    uint8_t *w = static_cast<uint8_t *>(ws);
    if (n_slices) {
        const SortShape shape = sort_shape(n_slices);
        uint32_t *keys[2] = {reinterpret_cast<uint32_t *>(w + L.keys[0]), reinterpret_cast<uint32_t *>(w + L.keys[1])};
        uint32_t *vals[2] = {reinterpret_cast<uint32_t *>(w + L.vals[0]), reinterpret_cast<uint32_t *>(w + L.vals[1])};
        uint32_t *hist = reinterpret_cast<uint32_t *>(w + L.hist), *hist_sums = reinterpret_cast<uint32_t *>(w + L.hist_sums);
        const uint32_t entries = kSortDigits * shape.blocks, entry_tiles = (entries + kScanTile - 1) / kScanTile;
        const dim3 grid(shape.blocks), block(256);
        for (uint32_t pass = 0; pass < 4; pass++) {
            const uint32_t *k_in = pass ? keys[(pass - 1) & 1] : nullptr, *v_in = pass ? vals[(pass - 1) & 1] : nullptr;
            uint32_t *k_out = pass < 3 ? keys[pass & 1] : nullptr, *v_out = pass < 3 ? vals[pass & 1] : order;
            hipLaunchKernelGGL(k_sort_hist, grid, block, 0, s, k_in, n_bins, n_slices, shape.per_block, 8 * pass, hist);
            hipLaunchKernelGGL(k_hist_reduce, dim3(entry_tiles), block, 0, s, hist, entries, hist_sums);
            hipLaunchKernelGGL(k_hist_scan, dim3(entry_tiles), block, 0, s, hist, entries, hist_sums);
            hipLaunchKernelGGL(k_sort_scatter, grid, block, 0, s, k_in, n_bins, v_in, n_slices, shape.per_block, 8 * pass, hist, k_out, v_out);
        }
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return scan<1>(s, TileSrc{n_bins, order, n_slices, records_per_chunk}, TileSink{tile_off, totals}, (uint64_t(n_slices) + 63) / 64, w + L.sums);
}

// the copy alone, on offsets the caller has made (the batch makes them on the host, where its getters need them): `dense` holds dense_total bytes
hipError_t launch_compact(hipStream_t s, const OutputView &o, const uint64_t *dense_off, uint32_t n_slices, uint8_t *dense, uint64_t dense_total) {
    if (n_slices == 0) return hipSuccess;
    hipLaunchKernelGGL(k_compact_wide, dim3((n_slices + 3u) / 4u), dim3(256), 0, s, o.out, o.out_off, n_slices, dense, dense_total, dense_off);
    return hipGetLastError();
}

hipError_t launch_compact_wide(hipStream_t s, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, uint32_t n_slices,
                               uint8_t *dense, uint64_t dense_capacity, uint64_t *dense_off, void *ws) {
    const CompactLayout L = compact_layout(n_slices);
    if (hipError_t e = scan<1>(s, LenSrc{out_off, out_len}, LenSink{dense_off}, n_slices, static_cast<uint8_t *>(ws) + L.sums); e != hipSuccess) return e;
    return launch_compact(s, OutputView{out, out_off}, dense_off, n_slices, dense, dense_capacity);
}

// the lengths behind the patch and the escapes, their prefix sums, the bytes: three steps on `s`, each behind the one before
hipError_t launch_finish(hipStream_t s, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, const int32_t *status,
                         uint32_t n_slices, const uint32_t *finish, uint8_t *dense, uint64_t dense_capacity, uint64_t *dense_off, void *ws) {
    const FinishLayout L = finish_layout(n_slices);
    uint8_t *w = static_cast<uint8_t *>(ws);
    uint64_t *lens = reinterpret_cast<uint64_t *>(w + L.lens);
    const FinishIn in{out, out_off, out_len, status, finish};
    const dim3 grid((n_slices + 3u) / 4u), block(256);
    if (n_slices) hipLaunchKernelGGL(k_finish_lengths, grid, block, 0, s, in, n_slices, lens);
    if (hipError_t e = scan<1>(s, ArraySrc<1>{reinterpret_cast<const Vec<1> *>(lens)}, LenSink{dense_off}, n_slices, w + L.sums); e != hipSuccess) return e;
    if (n_slices) hipLaunchKernelGGL(k_finish_copy, grid, block, 0, s, in, n_slices, dense, dense_capacity, dense_off);
    return hipGetLastError();
}

}  // namespace avr
