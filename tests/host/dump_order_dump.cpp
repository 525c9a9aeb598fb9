// What the standard library itself says about a set of keys, for tests/test_dump_order_ref_cpu.py to pin tests/dump_order_ref.py on:
//   dump_order_dump KEYS.bin [SCHEDULE_N]
// KEYS.bin holds n little-endian uint64 keys.  Prints two lines:
//   schedule COUNT:BUCKETS ...     DumpOrder::schedule(SCHEDULE_N, default n): asked of the library's own rehash policy object
//   order I ...                    the iteration order of a real std::unordered_map filled with the keys in file order, as indices into the file
#include <stdio.h>
#include <stdlib.h>

#include "junction_order.h"

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: dump_order_dump KEYS.bin [SCHEDULE_N]\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint64_t> keys;
    uint64_t buf[4096];
    for (size_t got; (got = fread(buf, 8, 4096, f)) > 0;) keys.insert(keys.end(), buf, buf + got);
    fclose(f);
    const size_t n = keys.size();
    printf("schedule");
    for (const DumpOrder::Rehash& r : DumpOrder::schedule(argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : n))
        printf(" %llu:%llu", (unsigned long long)r.count, (unsigned long long)r.buckets);
    printf("\n");
    std::unordered_map<uint64_t, uint32_t> real;
    for (size_t i = 0; i < n; i++) real.insert(std::pair<uint64_t, uint32_t>(keys[i], (uint32_t)i));
    if (real.size() != n) { fprintf(stderr, "repeated keys\n"); return 1; }
    printf("order");
    for (const auto& kv : real) printf(" %u", kv.second);
    printf("\n");
    return 0;
}
