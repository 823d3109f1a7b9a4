// K1 verifier for gfx950 (MI355X): the coded bytes of every slice decoded back, as the CABAC stream of H.264 9.3 they are, against
// the records they were made from.
//
//   k_cabac_verify<FORM>   DecodeDecision / DecodeBypass / DecodeTerminate (9.3.3.2) over known records; the per-lane decoder and the
//                          slice walk are in avr_cabac_verify.h.  FORM (cabac_verify::Form): two-byte or one-byte records, in tiles or
//                          slice-major, or resolved codes.
//
// Mapping: 64-thread workgroups, one lane per slice -- 64 slices to a wave over tiles (a tile is a wave's); over the slice-major forms
// and codes as few as still give each of the chip's 1 024 SIMDs a wave (launch_cabac_verify), because a wave walks the
// renormalisation path, and the refill of the bit reader, whenever one of its lanes does.  One lane per slice is a slice's whole serial
// chain: a chunk-parallel verifier would have to start from the encoder's own per-chunk states and would check nothing of them.
//
// LDS: rangeTabLPS and the transitions (128 entries of 8 bytes, one ds_read_b64 a bin), and the slices' state bytes in the layout of
// k_cabac_encode -- dword (k, lane) holds contexts 4k .. 4k + 3 of the lane's slice, so the 64 lanes of a wave hit 64 banks whatever
// contexts their bins name -- in the CALLER's numbering, and one spare byte a lane behind them (where a bin without a context reads and
// writes, so that no bin branches on its kind): (n_states + 1 + 3) / 4 rows of 256 bytes, dynamic, 64.25 KiB at 1 024 contexts.
// The way in: the wave takes its slices in turn, lane k fetching row k of the slice's init_states (coalesced; a lane gathering its own
// slice row by row is one load a row with 64 lines in it).  The way out, where the caller has the encoder's final states: the same
// walk, lane k comparing row k, one ballot a slice.
//
// Reads only: the kernel writes first_bad[slice] and, for a slice that fails, status[slice] -- never out, out_len, records, tiles or states.
// It reads `out` inside [out_off[i], out_off[i] + min(out_len[i], capacity)) rounded up to the 8-byte word, which lies inside the
// slice's region (offsets and so capacities are multiples of 8); what the region holds past the slice's length changes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "avr_cabac_verify.h"
#include "avr_coder.h"
#include "avr_internal.h"

namespace avr {

namespace {
namespace cv = cabac_verify;

__device__ const CabacTables d_verify_tables = make_cabac_tables();

// Where the lane of processing slot g finds chunk c of its slice (16 bytes: eight two-byte records, sixteen one-byte records or codes).
template <int FORM>
struct RecSource {
    const uint4 *p;
    uint32_t stride;                                             // in chunks
    __device__ RecSource(const void *recs, const uint64_t *off, uint32_t g, uint32_t slice) {
        if (cv::form_tiled(FORM)) {                              // off = tile_off (16-byte units), one entry per 64 slots
            p = reinterpret_cast<const uint4 *>(recs) + off[g >> 6] + (g & 63);
            stride = 64;
        } else {                                                 // off = rec_off in records (two-byte form) or bytes (one-byte form, codes), indexed by slice
            p = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(recs) + off[slice] * (cv::form_wide(FORM) ? 2 : 1));
            stride = 1;
        }
    }
    __device__ __forceinline__ cv::Chunk16 load(uint32_t c) const {
        const uint4 v = p[size_t(c) * stride];
        return cv::Chunk16{{v.x, v.y, v.z, v.w}};
    }
};

struct LdsStates {                                               // the lane's column of the state rows: context k at dword (k >> 2, lane), byte k & 3
    uint8_t *col;
    __device__ __forceinline__ uint32_t get(uint32_t ctx) const { return col[((ctx >> 2) << 8) + (ctx & 3)]; }
    __device__ __forceinline__ void set(uint32_t ctx, uint32_t s) { col[((ctx >> 2) << 8) + (ctx & 3)] = uint8_t(s); }
};
}  // namespace

template <int FORM>
__global__ __launch_bounds__(64) void k_cabac_verify(
    const void *recs, const uint64_t *off, const uint32_t *n_bins, const uint32_t *order, uint32_t n_slices,
    const uint8_t *init_states, uint32_t n_states, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
    const uint8_t *final_states, int32_t *status, uint32_t *first_bad, uint32_t per_wave) {
    extern __shared__ uint32_t st32[];                           // state dwords [(n_states + 1 + 3) / 4][64]; none for codes
    __shared__ cv::TabEntry tab[128];
    constexpr bool kStates = FORM != cv::kCodes;
    const uint32_t lane = threadIdx.x;
    for (uint32_t s = lane; s < 128; s += 64) tab[s] = cv::TabEntry{d_verify_tables.packed[s][0], d_verify_tables.packed[s][1]};

    const uint32_t g = blockIdx.x * per_wave + lane;             // per_wave slices to a workgroup: 64 over tiles, see the launcher
    const bool in_range = lane < per_wave && g < n_slices;
    const uint32_t slice = in_range ? (order ? order[g] : g) : 0;
    // any slice whose status is not AVR_SLICE_OK is skipped: its status stays, its bytes are not the slice's
    const bool active = in_range && status[slice] == AVR_SLICE_OK;
    const uint64_t act = __ballot(active);
    uint8_t *st_wave = reinterpret_cast<uint8_t *>(st32);

    if (kStates && act) {                                        // the way in: slice by slice, lane k the state of row k
        for (uint32_t k0 = 0; k0 < n_states; k0 += 64) {
            const uint32_t k = k0 + lane, kc = k < n_states ? k : 0u;
            uint8_t *dst = st_wave + ((k >> 2) << 8) + (k & 3);
            for (uint32_t j0 = 0; j0 < per_wave; j0 += 16) {     // (every load is made, sixteen in flight: a lane without a slice has slice 0)
                uint8_t v[16];
#pragma unroll
                for (uint32_t u = 0; u < 16; u++) {
                    const uint8_t *row = init_states + size_t(uint32_t(__builtin_amdgcn_readlane(int(slice), int((j0 + u) & 63u)))) * n_states;
                    v[u] = row[kc];
                }
#pragma unroll
                for (uint32_t u = 0; u < 16; u++)
                    if (((act >> (j0 + u)) & 1u) && k < n_states) dst[(j0 + u) * 4] = v[u];
            }
        }
    }
    __syncthreads();

    // a lane without a slice to decode walks nothing: no bins, no bytes -- and makes no load
    const uint32_t nb = active ? n_bins[slice] : 0;
    const uint64_t o0 = in_range ? out_off[slice] : 0;
    const uint32_t cap = in_range ? region_capacity(o0, out_off[slice + 1]) : 0, n = active ? out_len[slice] : 0;
    const RecSource<FORM> src(recs, off, in_range ? g : blockIdx.x * per_wave, slice);
    LdsStates st{st_wave + lane * 4};
    uint32_t bad = cv::verify_slice<FORM>(reinterpret_cast<const uint64_t *>(out + o0), n < cap ? n : cap, nb, n_states, src, st, tab);

    bool differ = false;
    __syncthreads();                                             // lane k reads below what lane j's walk wrote (one wave a workgroup: free)
    if (kStates && final_states) {                               // the way out: the decoder's states against the encoder's, all n_states bytes
        const uint64_t sound = __ballot(active && bad == AVR_VERIFY_NONE);
        for (uint32_t j = 0; j < per_wave; j++) {
            if (!((sound >> j) & 1u)) continue;
            const uint8_t *row = final_states + size_t(uint32_t(__builtin_amdgcn_readlane(int(slice), int(j)))) * n_states;
            bool d = false;
            for (uint32_t k = lane; k < n_states; k += 64) d |= row[k] != st_wave[((k >> 2) << 8) + (k & 3) + j * 4];
            if (__ballot(d) && lane == j) differ = true;
        }
    }
    if (in_range) {
        if (active) {
            bad = cv::conclude(bad, nb, differ);
            if (bad != AVR_VERIFY_NONE) status[slice] = AVR_SLICE_VERIFY_FAILED;
        }
        if (first_bad) first_bad[slice] = bad;
    }
}

hipError_t launch_cabac_verify(hipStream_t s, const Slices &in, const StatesView &st, const OutputView &o, uint32_t *first_bad) {
    const uint32_t n_slices = in.n_slices, n_states = st.n_states;
    const cabac_verify::Form form = in.form;
    if (n_slices == 0) return hipSuccess;
    // launch_range_verify's rule: tiles are laid out for 64 slices a wave; slice-major batches of few slices (K1p's shape) leave most of
    // the chip idle anyway, so there a wave takes as few slices as still give every SIMD of the chip (1 024) a wave.
    const uint32_t per_wave = cabac_verify::form_tiled(form) ? 64u : std::min(64u, (n_slices + 1023u) / 1024u);
    const uint32_t lds = form == cabac_verify::kCodes ? 0u : ((n_states + 1 + 3) / 4) * 256u;
    auto kern = form == cabac_verify::kTiles2 ? k_cabac_verify<cabac_verify::kTiles2>
              : form == cabac_verify::kSlices2 ? k_cabac_verify<cabac_verify::kSlices2>
              : form == cabac_verify::kTiles8 ? k_cabac_verify<cabac_verify::kTiles8>
              : form == cabac_verify::kSlices8 ? k_cabac_verify<cabac_verify::kSlices8> : k_cabac_verify<cabac_verify::kCodes>;
    if (lds > 48 * 1024) {                                       // 1 024 contexts: 64.25 KiB a wave, as launch_cabac_encode raises its kernel's limit
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
    }
    const dim3 grid((n_slices + per_wave - 1) / per_wave), block(64);
    hipLaunchKernelGGL(kern, grid, block, lds, s, in.recs, in.off, in.n_bins, in.order, n_slices, st.init_states, n_states, o.out, o.out_off,
                       o.out_len, st.final_states, o.status, first_bad, per_wave);
    return hipGetLastError();
}

}  // namespace avr
