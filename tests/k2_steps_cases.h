// One bin of the recoded range coder (K2) at chosen ranges: the cases, what plain 64-bit integers make of them, and the comparison.
// tests/k2_steps_host.cpp runs the cases through the host side of csrc/avr_div.h and csrc/avr_k2p.h, tests/k2_steps_dev.hip through
// the device side on the GPU (tests/k2_steps_run.h is what both run); either hands the raw results to compare_*() below.
//
// Nothing in this header comes from csrc/: the expectations are arithmetic_code.h:106-122 (put) and :147-180 (renormalize_and_emit_digit)
// with recode.cpp:823-827 (range / total * pos), said again in uint64_t /, *, - and shifts.  Deterministic: its own splitmix64.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

namespace k2s {

constexpr uint64_t kFixedOne = uint64_t(1) << 63;                // arithmetic_code.h:54-55
constexpr uint64_t kMinRange = uint64_t(1) << 51;                // :61-62: (fixed_one / digit_base) / 16
constexpr uint64_t kMsd = kFixedOne >> 8;                        // :120, :150: max_range / digit_base, the top digit's unit
constexpr uint32_t kRecords = 32768;                             // every bin | pos << 1 | neg << 8, pos and neg 0 .. 127: the record IS its index
constexpr uint32_t kChains = 250000, kChainLen = 8;
constexpr uint32_t kTwo39HiWord = 0x42600000u;                   // the high word of the double 2^39

struct SplitMix64 {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t n) { return next() % n; }
};

inline uint32_t pos_of(uint32_t rec) { return (rec >> 1) & 0x7fu; }
inline uint32_t neg_of(uint32_t rec) { return (rec >> 8) & 0x7fu; }
inline uint32_t total_of(uint32_t rec) { return pos_of(rec) + neg_of(rec); }

// ------------------------------------------------------------------------------------------------ the cases
struct Case {
    uint64_t range, low;                                         // low: seeded, below the range
    uint32_t rec, pad;
};

inline uint64_t clamped(uint64_t r) { return r < kMinRange ? kMinRange : r > kFixedOne ? kFixedOne : r; }

// The ranges of a record of total t: per exponent e = 51 .. 62 the ends of [2^e, 2^(e+1)), and, where t > 0, for two seeded q with
// q t in the interval the three ranges at which range / t is one unit from changing; two seeded values; and the coder's start, 2^63.
inline void ranges_of(uint32_t rec, std::vector<uint64_t> &out) {
    const uint64_t t = total_of(rec);
    SplitMix64 g{0x6b32d1ull * rec + 17};
    for (uint32_t e = 51; e <= 62; e++) {
        const uint64_t lo = uint64_t(1) << e, hi = lo + (lo - 1);
        out.push_back(lo);
        out.push_back(lo + 1);
        out.push_back(hi);
        for (uint32_t k = 0; k < 2 && t; k++) {
            const uint64_t q_lo = (lo + t - 1) / t, q_hi = hi / t, m = (q_lo + g.below(q_hi - q_lo + 1)) * t;
            out.push_back(clamped(m - 1));
            out.push_back(m);
            out.push_back(clamped(m + 1));
        }
        for (uint32_t k = 0; k < 2; k++) out.push_back(lo + g.below(hi - lo + 1));
    }
    out.push_back(kFixedOne);
}

inline std::vector<Case> cases_of(uint32_t rec_begin, uint32_t rec_end) {
    std::vector<Case> cases;
    std::vector<uint64_t> ranges;
    for (uint32_t rec = rec_begin; rec < rec_end; rec++) {
        ranges.clear();
        ranges_of(rec, ranges);
        SplitMix64 g{0x51ull * rec + 3};
        for (uint64_t r : ranges) cases.push_back(Case{r, g.below(r), rec, 0});
    }
    return cases;
}

// Chains of kChainLen records with pos, neg >= 1 from a range of the list: the redundant (H, L) states of the double-precision form
// that only a walk reaches.  Every 16th chain: records with min(pos, neg) == 1 and total >= 97 only, where a bin shifts out 16 bits.
struct Chain {
    uint64_t range;
    uint32_t rec[kChainLen];
};

inline std::vector<Chain> chains() {
    std::vector<Chain> out(kChains);
    std::vector<uint64_t> ranges;
    SplitMix64 g{0xc4a1};
    for (uint32_t c = 0; c < kChains; c++) {
        ranges.clear();
        ranges_of(uint32_t(g.below(kRecords)), ranges);
        out[c].range = ranges[g.below(ranges.size())];
        for (uint32_t k = 0; k < kChainLen; k++) {
            uint32_t pos = 1 + uint32_t(g.below(127)), neg = 1 + uint32_t(g.below(127));
            if (c % 16 == 15) {
                const uint32_t big = 96 + uint32_t(g.below(32));
                pos = g.below(2) ? 1 : big;
                neg = pos == 1 ? big : 1;
            }
            out[c].rec[k] = uint32_t(g.below(2)) | (pos << 1) | (neg << 8);
        }
    }
    return out;
}

// ------------------------------------------------------------------------------------------------ what the integers say
// A record of total 0 is the ABI's padding record: the quotient counts as 0 and the bin as 0, so that it changes nothing (the
// reference would divide by zero; the library refuses such a record inside a slice).
struct WantStep {
    uint64_t raw, range;                                         // the new range before and after its shifts
    uint32_t shifts;
    bool ok;                                                     // false: a bin of probability zero (arithmetic_code.h:116-118)
};

inline WantStep want_step(uint64_t range, uint32_t rec) {
    const uint64_t pos = pos_of(rec), total = total_of(rec);
    const uint32_t symbol = total ? rec & 1u : 0u;
    const uint64_t range_of_1 = total ? (range / total) * pos : 0;      // recode.cpp:825-826
    const uint64_t range_of_0 = range - range_of_1;                     // arithmetic_code.h:108
    WantStep w{symbol ? range_of_1 : range_of_0, 0, 0, true};           // :109-114
    w.range = w.raw;
    if (w.raw < kMinRange) {                                            // :115
        if (w.raw == 0) { w.ok = false; return w; }                     // :116-118
        while (w.range < kMsd) { w.range *= 256; w.shifts++; }          // :120-122, :179
    }
    return w;
}

struct WantBin {
    uint64_t low, range;
    uint32_t n, digit[8];                                        // 9 bits each: the carry on top of the byte
    bool ok;
};

inline WantBin want_bin(uint64_t low, uint64_t range, uint32_t rec) {
    const uint64_t pos = pos_of(rec), total = total_of(rec);
    const uint32_t symbol = total ? rec & 1u : 0u;
    const uint64_t range_of_1 = total ? (range / total) * pos : 0;
    const uint64_t range_of_0 = range - range_of_1;
    WantBin w{low, range, 0, {0, 0, 0, 0, 0, 0, 0, 0}, true};
    if (symbol) { w.low += range_of_0; w.range = range_of_1; }          // :109-111
    else w.range = range_of_0;                                          // :113
    if (w.range < kMinRange) {
        if (w.range == 0) { w.ok = false; return w; }
        while (w.range < kMsd) {                                        // renormalize_and_emit_digit<uint8_t>
            uint32_t carry = 0;
            if (w.low >= kFixedOne) { carry = 1; w.low -= kFixedOne; }  // :154-159
            const uint64_t digit = w.low / kMsd;                        // :164
            w.digit[w.n++] = (carry << 8) | uint32_t(digit);
            w.low -= digit * kMsd;                                      // :177
            w.low *= 256;                                               // :178
            w.range *= 256;                                             // :179
        }
    }
    return w;
}

// ------------------------------------------------------------------------------------------------ the raw results
struct TabGot { double inv, half, inv32; };                      // check 1: 1.0 / double(d), 0.5 * inv, 4294967296.0 * inv (d = 0: inv 0)
struct StepGot { uint64_t range; uint32_t bytes, ok; };          // check 2: range_step
struct BinGot { uint64_t low, range, digits; uint32_t n, ok; };  // check 3: bin<true>; digits: 9 bits each, the first lowest (7 fit)
struct FpGot {                                                   // check 4: range_step_fp
    double H, L;
    uint64_t u64;                                                // fp_to_u64 where it was run
    uint32_t vmin_hi, bits;
};
struct CaseGot {
    StepGot step;
    BinGot bin[3];                                               // from low = 0, the seeded low, 2^63 - 1 (the last forces the carry bit)
    FpGot fp;
};
struct ChainGot { FpGot step[kChainLen]; };                      // check 5: vmin_hi running over the chain, as in the kernel

inline uint64_t low_of(const Case &c, uint32_t k) { return k == 0 ? 0 : k == 1 ? c.low : kFixedOne - 1; }

// ------------------------------------------------------------------------------------------------ the comparison
struct Check {
    const char *name;
    uint64_t cases = 0, mismatches = 0;
    std::string first;
    void miss(const std::string &what) { if (!mismatches++) first = what; }
};

struct Report {
    Check table{"1 reciprocal table"}, step{"2 integer form (range_step)"}, bin{"3 full bin (bin<true>)"},
        fp{"4 double-precision form, one step"}, chain{"5 double-precision form, chains"};
    uint64_t mismatches() const { return table.mismatches + step.mismatches + bin.mismatches + fp.mismatches + chain.mismatches; }
    void print() const {
        for (const Check *c : {&table, &step, &bin, &fp, &chain}) {
            printf("check %s: %llu cases, %llu mismatches\n", c->name, (unsigned long long)c->cases, (unsigned long long)c->mismatches);
            if (c->mismatches) printf("  first: %s\n", c->first.c_str());
        }
        printf("k2_steps: %llu mismatches\n", (unsigned long long)mismatches());
    }
};

inline std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
inline std::string fmt(const char *f, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

inline uint64_t bits_of(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }

// `mine`: this program's own (host) values of the three expressions
inline void compare_table(const TabGot *got, const TabGot *mine, Report &r) {
    for (uint32_t d = 0; d < 256; d++) {
        r.table.cases++;
        if (bits_of(got[d].inv) != bits_of(mine[d].inv) || bits_of(got[d].half) != bits_of(mine[d].half) || bits_of(got[d].inv32) != bits_of(mine[d].inv32))
            r.table.miss(fmt("d=%u: inv %016llx half %016llx inv32 %016llx, the host's %016llx %016llx %016llx", d,
                             (unsigned long long)bits_of(got[d].inv), (unsigned long long)bits_of(got[d].half), (unsigned long long)bits_of(got[d].inv32),
                             (unsigned long long)bits_of(mine[d].inv), (unsigned long long)bits_of(mine[d].half), (unsigned long long)bits_of(mine[d].inv32)));
    }
}

// One step of the double-precision form against the integers; returns a description of what differs, or nothing.
inline std::string fp_differs(const FpGot &g, const WantStep &w) {
    const bool below = w.raw < (uint64_t(1) << 39);
    if ((g.vmin_hi < kTwo39HiWord) != below) return fmt("vmin_hi %08x with a new range %s 2^39", g.vmin_hi, below ? "below" : "of at least");
    if (below) return "";                                        // handed to the integer form: nothing else is promised
    const double two47 = 140737488355328.0;
    if (!(g.H >= 0) || !(g.H < 4503599627370496.0) || !(g.L <= two47 && g.L >= -two47)) return fmt("H %a L %a outside H >= 0, |L| <= 2^47", g.H, g.L);
    const uint64_t here = (uint64_t(g.H) << 32) + uint64_t(int64_t(g.L));
    if (here != w.range || g.u64 != w.range) return fmt("H %a L %a = %llu (fp_to_u64 there: %llu)", g.H, g.L, (unsigned long long)here, (unsigned long long)g.u64);
    if (g.bits != 8 * w.shifts) return fmt("%u bits shifted out", g.bits);
    return "";
}

inline void compare_cases(const std::vector<Case> &cases, const CaseGot *got, Report &r) {
    for (size_t i = 0; i < cases.size(); i++) {
        const Case &c = cases[i];
        const CaseGot &g = got[i];
        const std::string at = fmt("range %llu rec %#x (bin %u pos %u neg %u)", (unsigned long long)c.range, c.rec, c.rec & 1, pos_of(c.rec), neg_of(c.rec));
        const WantStep w = want_step(c.range, c.rec);
        r.step.cases++;
        if (g.step.range != (w.ok ? w.range : 0) || g.step.bytes != w.shifts || (g.step.ok != 0) != w.ok)
            r.step.miss(fmt("%s: range %llu bytes %u ok %u, expected %llu %u %d", at.c_str(), (unsigned long long)g.step.range, g.step.bytes, g.step.ok,
                            (unsigned long long)w.range, w.shifts, int(w.ok)));
        for (uint32_t k = 0; k < 3; k++) {
            const WantBin b = want_bin(low_of(c, k), c.range, c.rec);
            const BinGot &h = g.bin[k];
            r.bin.cases++;
            uint64_t digits = 0;
            for (uint32_t j = 0; j < b.n && j < 7; j++) digits |= uint64_t(b.digit[j]) << (9 * j);
            const bool same = b.ok ? (h.ok && h.low == b.low && h.range == b.range && h.n == b.n && h.digits == digits) : (!h.ok && h.range == 0);
            if (!same || b.n > 7)
                r.bin.miss(fmt("%s low %llu: low %llu range %llu n %u digits %#llx ok %u, expected %llu %llu %u %#llx %d", at.c_str(),
                               (unsigned long long)low_of(c, k), (unsigned long long)h.low, (unsigned long long)h.range, h.n, (unsigned long long)h.digits, h.ok,
                               (unsigned long long)b.low, (unsigned long long)b.range, b.n, (unsigned long long)digits, int(b.ok)));
        }
        r.fp.cases++;
        const std::string d = fp_differs(g.fp, w);
        if (!d.empty()) r.fp.miss(fmt("%s: %s, expected range %llu after %u shifts", at.c_str(), d.c_str(), (unsigned long long)w.range, w.shifts));
    }
}

inline void compare_chains(const std::vector<Chain> &chains, const ChainGot *got, Report &r) {
    for (size_t c = 0; c < chains.size(); c++) {
        uint64_t range = chains[c].range;
        r.chain.cases++;
        for (uint32_t k = 0; k < kChainLen; k++) {
            const WantStep w = want_step(range, chains[c].rec[k]);   // pos, neg >= 1 and range >= 2^51: the new range is 2^43 at least
            const std::string d = fp_differs(got[c].step[k], w);
            if (!d.empty()) {
                r.chain.miss(fmt("chain %zu (from range %llu) step %u rec %#x at range %llu: %s, expected range %llu after %u shifts", c,
                                 (unsigned long long)chains[c].range, k, chains[c].rec[k], (unsigned long long)range, d.c_str(), (unsigned long long)w.range, w.shifts));
                break;
            }
            range = w.range;
        }
    }
}

}  // namespace k2s
