// K2 verifier for gfx950 (MI355X): the coded bytes of every slice decoded back against the records they were made from.
//
//   k_range_verify   recoded_code::decoder over known records (arithmetic_code<uint64_t, uint8_t>::decoder,
//                    arithmetic_code.h:209-298; the per-lane decoder and the slice walk are in avr_verify.h)
//
// Mapping: k_range_encode's -- 64-thread workgroups, one lane per slice (64 slices to a workgroup over tiles; over the slice-major layout
// as few as still fill the chip, launch_range_verify), fl(1 / d) for the 256 divisors in LDS, a chunk's operands
// fetched before its first bin, the records two chunks ahead through ChunkSource<TILED> (tiles or the slice-major layout).  The coded
// bytes are a lane-private stream of about 0.1 byte a bin, read in aligned 8-byte words, one word ahead.
//
// Reads only: the kernel writes first_bad[slice] and, for a slice that fails, status[slice] -- never out, out_len, records or tiles.
// It reads `out` inside [out_off[i], out_off[i] + min(out_len[i], capacity)) rounded up to the 8-byte word, which lies inside the
// slice's region (offsets and so capacities are multiples of 8); what the region holds past the slice's length changes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "avr_coder.h"
#include "avr_internal.h"
#include "avr_verify.h"

namespace avr {

namespace {
template <bool TILED>
struct VerifySource {                                            // ChunkSource's chunks as the walk of avr_verify.h takes them
    ChunkSource<TILED> src;
    __device__ VerifySource(const void *recs, const uint64_t *off, uint32_t g, uint32_t slice) : src(recs, off, g, slice) {}
    __device__ __forceinline__ verify::Chunk8 load(uint32_t c) const {
        const uint4 v = src.load(c);
        return verify::Chunk8{{v.x, v.y, v.z, v.w}};
    }
};
}  // namespace

template <bool TILED>
__global__ __launch_bounds__(64) void k_range_verify(
    const void *recs, const uint64_t *off, const uint32_t *n_bins, const uint32_t *order, uint32_t n_slices,
    const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, int32_t *status, uint32_t *first_bad, uint32_t per_wave) {
    __shared__ double inv_d[256];                                // fl(1 / d)
    const uint32_t lane = threadIdx.x;
    for (uint32_t d = lane; d < 256; d += 64) inv_d[d] = d ? 1.0 / double(d) : 0.0;
    __syncthreads();
    const uint32_t g = blockIdx.x * per_wave + lane;            // per_wave slices to a workgroup: 64 over tiles (a tile is a wave's), see the launcher
    if (lane >= per_wave || g >= n_slices) return;
    const uint32_t slice = order ? order[g] : g;
    uint32_t bad = AVR_VERIFY_NONE;
    if (status[slice] == AVR_SLICE_OK) {                         // any other slice is skipped: its status stays, its bytes are not the slice's
        const uint64_t o0 = out_off[slice];
        const uint32_t cap = region_capacity(o0, out_off[slice + 1]), n = out_len[slice];
        const VerifySource<TILED> src(recs, off, g, slice);
        bad = verify::verify_slice(reinterpret_cast<const uint64_t *>(out + o0), n < cap ? n : cap, n_bins[slice], src, inv_d);
        if (bad != AVR_VERIFY_NONE) status[slice] = AVR_SLICE_VERIFY_FAILED;
    }
    if (first_bad) first_bad[slice] = bad;
}

hipError_t launch_range_verify(hipStream_t s, const Slices &in, const OutputView &o, uint32_t *first_bad) {
    const uint32_t n_slices = in.n_slices;
    if (n_slices == 0) return hipSuccess;
    // The lanes of a wave renormalise at different bins, and the wave walks that path whenever one of them does.  Slice-major batches of few
    // slices (K2p's shape) leave most of the chip idle anyway: there a wave takes as few slices as still give every SIMD of the chip
    // (1 024) a wave -- one slice up to 1 024 slices, 64 from 64 Ki on.  Tiles are laid out for 64 slices a wave.
    const uint32_t per_wave = in.tiled ? 64u : std::min(64u, (n_slices + 1023u) / 1024u);
    const dim3 grid((n_slices + per_wave - 1) / per_wave), block(64);
    auto kern = in.tiled ? k_range_verify<true> : k_range_verify<false>;
    hipLaunchKernelGGL(kern, grid, block, 0, s, in.recs, in.off, in.n_bins, in.order, n_slices, o.out, o.out_off, o.out_len, o.status, first_bad, per_wave);
    return hipGetLastError();
}

#ifdef AVR_TEST_HOOKS
// Test build only (verify_flip, avr_internal.h): bit 7 of byte 0 of one slice's output region complemented between the encode and the
// verifier, which is how a test sees a failure travel through the batch API.
__global__ void k_verify_flip(uint8_t *out, const uint64_t *out_off, uint32_t slice) {
    if (blockIdx.x == 0 && threadIdx.x == 0) out[out_off[slice]] ^= 0x80u;
}
hipError_t launch_verify_flip(hipStream_t s, const Output &o, uint32_t slice) {
    hipLaunchKernelGGL(k_verify_flip, dim3(1), dim3(64), 0, s, o.out, o.out_off, slice);
    return hipGetLastError();
}
#endif

}  // namespace avr
