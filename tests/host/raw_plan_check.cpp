// raw_plan_check <file>: fgpu_raw_plan (faucet_amd/csrc/raw_plan.cpp) as a stand-alone CPU program, for tests/test_raw_contigs_ref_cpu.py, which
// builds it under -fsanitize=address,undefined.  TEST ONLY.
// The file: u64 junctions, u64 calls, i32 k, i32 read_length, u64 cap; then the keys, the fgpu_junction records, the fgpu_contig and the
// fgpu_build_call arrays as the C ABI lays them out.  Printed: "status <s> n <records>", the six counts of fgpu_raw_info, and one line per
// record that was written: number, pieces, then text word, bases and flip of each piece.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/faucet_gpu.h"

template <class T>
static bool get(FILE* f, std::vector<T>& v, uint64_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t head[2], cap = 0;
    int32_t kr[2];
    if (fread(head, 8, 2, f) != 2 || fread(kr, 4, 2, f) != 2 || fread(&cap, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> keys;
    std::vector<fgpu_junction> recs;
    std::vector<fgpu_contig> contigs;
    std::vector<fgpu_build_call> calls;
    if (!get(f, keys, head[0]) || !get(f, recs, head[0]) || !get(f, contigs, head[1]) || !get(f, calls, head[1])) return 2;
    fclose(f);
    std::vector<fgpu_fasta_seq> out(cap);
    uint64_t n = 0;
    fgpu_raw_info info;
    memset(&info, 0, sizeof(info));
    const int status = fgpu_raw_plan(keys.data(), recs.data(), head[0], contigs.data(), calls.data(), head[1], kr[0], kr[1], out.data(), cap, &n, &info);
    printf("status %d n %llu\n", status, (unsigned long long)n);
    printf("info %llu %llu %llu %llu %llu %llu\n", (unsigned long long)info.records, (unsigned long long)info.bubble_records, (unsigned long long)info.node_contigs,
           (unsigned long long)info.isolated_kept, (unsigned long long)info.isolated_dropped, (unsigned long long)info.nodes);
    if (status == FGPU_PLAN_OK || status == FGPU_PLAN_SHORT)
        for (uint64_t i = 0; i < n && i < cap; i++) {
            const fgpu_fasta_seq& s = out[i];
            printf("%u %d", s.number, (int)s.pieces);
            for (int p = 0; p < s.pieces; p++) printf(" %llu %u %d", (unsigned long long)s.text_word[p], s.len[p], (int)s.flip[p]);
            printf("\n");
        }
    return 0;
}
