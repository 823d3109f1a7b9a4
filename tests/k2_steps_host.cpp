// The cases of tests/k2_steps_cases.h through the host side of csrc/avr_div.h and csrc/avr_k2p.h (tests/k2_steps_run.h), compared with
// the header's plain integers.  A stand-alone program: tests/test_k2_steps.py builds it with the address and undefined-behaviour
// sanitizers and expects "0 mismatches" and exit status 0.
#include <cstdio>
#include <vector>

#include "k2_steps_run.h"

int main() {
    using namespace k2s;
    Report report;
    TabGot table[256];
    for (uint32_t d = 0; d < 256; d++) table[d] = run_table(d);
    compare_table(table, table, report);                         // (on the host the table is its own reference: the count is what it shows)
    std::vector<CaseGot> got;
    for (uint32_t rec = 0; rec < kRecords; rec += 4096) {
        const std::vector<Case> cases = cases_of(rec, rec + 4096);
        got.resize(cases.size());
        for (size_t i = 0; i < cases.size(); i++) run_case(cases[i], got[i]);
        compare_cases(cases, got.data(), report);
    }
    const std::vector<Chain> ch = chains();
    std::vector<ChainGot> chain_got(ch.size());
    for (size_t c = 0; c < ch.size(); c++) run_chain(ch[c], chain_got[c]);
    compare_chains(ch, chain_got.data(), report);
    report.print();
    return report.mismatches() ? 1 : 0;
}
