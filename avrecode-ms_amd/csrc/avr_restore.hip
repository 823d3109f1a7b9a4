// Restore check for gfx950 (MI355X): does every coded K1 slice restore the payload it was made from?  The decompressor's epilogue --
// finish (the stop byte dropped), then the tail patch with the two values the container carries -- applied to the coded bytes as they
// lie on the device and compared with the payload the compressor holds.  The rule is in avr_restore.h, per 8-byte word.
//
//   k_restore_check   one wave per slice, four waves to a workgroup.  Lane l takes the aligned 8-byte words l, l + 64, ... of both
//                     strings (a wave's load is 512 contiguous bytes of each), forms the restored word, XORs it with the expected one
//                     and takes the index of the lowest differing byte; the wave takes the least by cross-lane shuffles; lane 0
//                     writes first_diff[slice] and, on a finding, the status.  No LDS, no atomics, no workspace.
//
// Reads only: of `out` the words inside [out_off[i], out_off[i] + min(out_len[i], capacity)) rounded up to the 8-byte word, which lies
// inside the slice's region (offsets and so capacities are multiples of 8), and never a word that starts at or past that length -- the
// region may hold anything there; of `expect` the words of [expect_off[i], expect_off[i] + expect_len[i]) rounded up the same way.
// All offsets are 64 bits wide.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avr_coder.h"
#include "avr_internal.h"
#include "avr_restore.h"

namespace avr {

__global__ __launch_bounds__(256) void k_restore_check(
    const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len, uint32_t n_slices, const uint8_t *expect,
    const uint64_t *expect_off, const uint32_t *expect_len, int32_t *status, uint32_t *first_diff) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slice = blockIdx.x * 4u + (threadIdx.x >> 6);         // the same for a wave's 64 lanes
    if (slice >= n_slices) return;
    const int32_t st = status[slice];
    const uint32_t E = expect_len[slice];
    // a slice takes part when the encoder finished it (a verifier may have failed it since) and the caller expects something of it
    if ((st != AVR_SLICE_OK && st != AVR_SLICE_VERIFY_FAILED) || E == AVR_EXPECT_NONE) {
        if (lane == 0) first_diff[slice] = AVR_VERIFY_NONE;
        return;
    }
    const uint64_t o0 = out_off[slice];
    const uint32_t cap = region_capacity(o0, out_off[slice + 1]), n = out_len[slice], L = n < cap ? n : cap;
    const uint8_t *o = out + o0, *e = expect + expect_off[slice];
    const restore::Shape s = restore::make_shape(L, E, L ? o[L - 1] : 0u, E >= 2 ? e[E - 1] : 0u);
    uint32_t best = restore::lane_first_diff(reinterpret_cast<const uint64_t *>(o), reinterpret_cast<const uint64_t *>(e), s, lane);
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const uint32_t other = uint32_t(__shfl_xor(int(best), d, 64));
        best = other < best ? other : best;
    }
    if (lane == 0) {
        const uint32_t found = restore::conclude(best, s);
        first_diff[slice] = found;
        if (found != AVR_VERIFY_NONE && st == AVR_SLICE_OK) status[slice] = AVR_SLICE_VERIFY_FAILED;
    }
}

hipError_t launch_restore_check(hipStream_t s, const OutputView &o, uint32_t n_slices, const uint8_t *expect, const uint64_t *expect_off,
                                const uint32_t *expect_len, uint32_t *first_diff) {
    if (n_slices == 0) return hipSuccess;
    const dim3 grid((n_slices + 3u) / 4u), block(256);
    hipLaunchKernelGGL(k_restore_check, grid, block, 0, s, o.out, o.out_off, o.out_len, n_slices, expect, expect_off, expect_len, o.status, first_diff);
    return hipGetLastError();
}

}  // namespace avr
