// What tests/k2_steps_host.cpp (on the CPU) and tests/k2_steps_dev.hip (one lane a case, on the GPU) run: the library's own
// `__host__ __device__` functions of csrc/avr_div.h and csrc/avr_k2p.h on the cases of tests/k2_steps_cases.h, the raw results into the
// case's own slot.  Nothing here is indexed or bounded by a computed value: a wrong value stays a wrong value.
#pragma once
#include "avr_div.h"
#include "avr_k2p.h"
#include "k2_steps_cases.h"

#if defined(__HIPCC__)
#define K2S_HD __host__ __device__ inline
#else
#define K2S_HD inline
#endif

namespace k2s {

// the entries of the kernels' reciprocal tables (fill_inv, ranges_fp_body: csrc/avr_k2p.hip), as they write them
K2S_HD TabGot run_table(uint32_t d) {
    const double inv = d ? 1.0 / double(d) : 0.0;
    return TabGot{inv, 0.5 * inv, 4294967296.0 * inv};
}

K2S_HD FpGot fp_got(const avr::k2p::RangeFP &f, uint32_t vmin_hi, uint32_t bits) {
    // fp_to_u64 of a state the form has left (H negative or huge) is not defined on the host: such a state shows in H and L
    const bool sane = f.H >= 0 && f.H < 4294967296.0 * 1048576.0 && f.L < 9e18 && f.L > -9e18;
    return FpGot{f.H, f.L, sane ? avr::k2p::fp_to_u64(f) : 0, vmin_hi, bits};
}

K2S_HD void run_case(const Case &c, CaseGot &g) {
    using namespace avr::k2p;
    const uint32_t total = ((c.rec >> 1) & 0x7fu) + ((c.rec >> 8) & 0x7fu);
    const double i1 = total ? 1.0 / double(total) : 0.0;                                     // the kernels' inv[total]
    const auto div = [i1](uint64_t r, uint32_t t) { return avr::div_u64_small_f64(r, double(t), i1); };    // as k_k2p_ranges has it
    {
        uint64_t range = c.range;
        uint32_t bytes = 0;
        const bool ok = range_step(range, bytes, c.rec, div);
        g.step = StepGot{range, bytes, ok ? 1u : 0u};
    }
    for (uint32_t k = 0; k < 3; k++) {
        uint64_t low = k == 0 ? 0 : k == 1 ? c.low : kFixedOne - 1, range = c.range, digits = 0;
        uint32_t n = 0;
        const bool ok = bin<true>(low, range, c.rec, div, [&](uint32_t d) {
            if (n < 7) digits |= uint64_t(d) << (9 * n);
            n++;
        });
        g.bin[k] = BinGot{low, range, digits, n, ok ? 1u : 0u};
    }
    RangeFP f = fp_from_u64(c.range);
    uint32_t vmin_hi = 0xffffffffu;
    const uint32_t bits = range_step_fp(f, vmin_hi, fp_operands(c.rec), fp_consts());
    g.fp = fp_got(f, vmin_hi, bits);
}

K2S_HD void run_chain(const Chain &c, ChainGot &g) {
    using namespace avr::k2p;
    RangeFP f = fp_from_u64(c.range);
    uint32_t vmin_hi = 0xffffffffu;
    const FpConsts K = fp_consts();
    for (uint32_t k = 0; k < kChainLen; k++) {
        const uint32_t bits = range_step_fp(f, vmin_hi, fp_operands(c.rec[k]), K);
        g.step[k] = fp_got(f, vmin_hi, bits);
    }
}

}  // namespace k2s
