// The cases of tests/k2_steps_cases.h through the DEVICE side of csrc/avr_div.h and csrc/avr_k2p.h (tests/k2_steps_run.h), one lane a
// case: the compiler's FP64 division for the reciprocals, the device's fma, trunc, floor and ldexp, its conversions between 64-bit
// integers and doubles.  Each lane reads its own case and writes its own result slot, nothing else; the raw results come back and the
// HOST compares them with the header's plain integers.  A stand-alone program: tests/test_gpu_k2_steps.py builds and runs it and
// expects "0 mismatches" and exit status 0.  The first HIP error ends it with status 2.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "k2_steps_run.h"

#define HIP_OK(call)                                                                                    \
    do {                                                                                                \
        const hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                         \
            fprintf(stderr, "k2_steps_dev: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
            exit(2);                                                                                    \
        }                                                                                               \
    } while (0)

using namespace k2s;

__global__ __launch_bounds__(256) void k_table(TabGot *out) {
    out[threadIdx.x] = run_table(threadIdx.x);                   // one block of 256 lanes, 256 slots
}

__global__ __launch_bounds__(256) void k_cases(const Case *in, CaseGot *out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    CaseGot g;
    run_case(in[i], g);
    out[i] = g;
}

__global__ __launch_bounds__(256) void k_chains(const Chain *in, ChainGot *out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    ChainGot g;
    run_chain(in[i], g);
    out[i] = g;
}

template <class In, class Out, class Kernel>
static void on_device(Kernel kernel, const std::vector<In> &in, std::vector<Out> &out) {
    const uint32_t n = uint32_t(in.size());
    out.resize(n);
    In *d_in = nullptr;
    Out *d_out = nullptr;
    HIP_OK(hipMalloc(&d_in, n * sizeof(In)));
    HIP_OK(hipMalloc(&d_out, n * sizeof(Out)));
    HIP_OK(hipMemcpy(d_in, in.data(), n * sizeof(In), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xee, n * sizeof(Out)));             // a slot no lane wrote compares wrong
    kernel<<<(n + 255) / 256, 256>>>(d_in, d_out, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), d_out, n * sizeof(Out), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
}

int main() {
    Report report;
    {
        TabGot *d_table = nullptr, got[256], mine[256];
        HIP_OK(hipMalloc(&d_table, sizeof got));
        HIP_OK(hipMemset(d_table, 0xee, sizeof got));
        k_table<<<1, 256>>>(d_table);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got, d_table, sizeof got, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_table));
        for (uint32_t d = 0; d < 256; d++) mine[d] = run_table(d);
        compare_table(got, mine, report);
    }
    std::vector<CaseGot> got;
    for (uint32_t rec = 0; rec < kRecords; rec += 4096) {        // 4 096 records: about 545 000 cases, 80 MB of results
        const std::vector<Case> cases = cases_of(rec, rec + 4096);
        on_device(k_cases, cases, got);
        compare_cases(cases, got.data(), report);
    }
    const std::vector<Chain> ch = chains();
    std::vector<ChainGot> chain_got;
    on_device(k_chains, ch, chain_got);
    compare_chains(ch, chain_got.data(), report);
    report.print();
    return report.mismatches() ? 1 : 0;
}
