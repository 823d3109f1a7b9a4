// The host plan timed for tools/plan_bench.py: fill_plan (every array of the K1p plan) and plan_tiles of csrc/avr_plan.h over lengths read
// from a file of raw uint32, `steps` times after `warmup`, each by std::chrono.  Prints "fill_plan_ms <median> <min> <max>" and the same
// for plan_tiles_ms.  Plain g++:  g++ -O2 -std=c++17 -I avrecode-ms_amd/csrc -o tools/_plan_host_time tools/plan_host_time.cpp
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "avr_plan.h"

static void report(const char *name, std::vector<double> v) {
    std::sort(v.begin(), v.end());
    std::printf("%s %.6f %.6f %.6f\n", name, v[v.size() / 2], v.front(), v.back());
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const int warmup = std::atoi(argv[2]), steps = std::atoi(argv[3]);
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f || steps < 1) return 2;
    std::fseek(f, 0, SEEK_END);
    std::vector<uint32_t> n_bins(size_t(std::ftell(f)) / 4);
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(n_bins.data(), 4, n_bins.size(), f) != n_bins.size()) return 2;
    std::fclose(f);
    std::vector<double> fill, tiles;
    uint64_t keep = 0;                                           // the results are used: nothing is optimised away
    for (int i = 0; i < warmup + steps; i++) {
        avr::HostPlan p;
        std::vector<uint32_t> order;
        std::vector<uint64_t> tile_off;
        const auto t0 = std::chrono::steady_clock::now();
        avr::fill_plan(p, n_bins.data(), n_bins.size(), avr::PlanFor::K1p);
        const auto t1 = std::chrono::steady_clock::now();
        avr::plan_tiles(n_bins, order, tile_off, 8);
        const auto t2 = std::chrono::steady_clock::now();
        keep += p.out_off.back() + p.chunk_slice.size() + tile_off.back() + (order.empty() ? 0 : order.back());
        if (i >= warmup) {
            fill.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            tiles.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
        }
    }
    report("fill_plan_ms", fill);
    report("plan_tiles_ms", tiles);
    std::printf("keep %llu\n", (unsigned long long)keep);
    return 0;
}
