// kept_ranges_check.cpp — faucet_amd/host/kept_ranges.h alone.  It judges nothing itself: for every case on stdin it prints the bounds, and
// tests/test_multi_scan_kept_cpu.py compares them with a restatement in plain Python.
//
//   a case, one line:   <n ranks> <group> <G batches> <T of each batch ...> <reads of each batch ...>
//   its answer:         <n + 1 bounds>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "kept_ranges.h"

int main() {
    unsigned long long n = 0, group = 0, G = 0;
    while (scanf("%llu %llu %llu", &n, &group, &G) == 3) {
        std::vector<uint64_t> T((size_t)G), reads((size_t)G);
        for (uint64_t& t : T) { unsigned long long v = 0; if (scanf("%llu", &v) != 1) return 2; t = v; }
        for (uint64_t& r : reads) { unsigned long long v = 0; if (scanf("%llu", &v) != 1) return 2; r = v; }
        const std::vector<uint64_t> b = faucet_host::kept_scan_ranges(T, reads, (int)n, group);
        for (size_t i = 0; i < b.size(); i++) printf(i ? " %llu" : "%llu", (unsigned long long)b[i]);
        printf("\n");
    }
    return 0;
}
