// tips_plan_check <file>: fgpu_tips_plan (faucet_amd/csrc/tips_plan.cpp) as a stand-alone CPU program, for tests/test_detip_plan_cpu.py, which
// builds it under -fsanitize=address,undefined.  TEST ONLY.
// The file is raw_plan_check's: u64 junctions, u64 calls, i32 k, i32 read_length, u64 cap; then the keys, the fgpu_junction records, the
// fgpu_contig and the fgpu_build_call arrays as the C ABI lays them out.  The plan is asked twice: with no room at all, which says how much is
// needed ("sizing <status>"), then with exactly that much, or with `cap` entries per array where cap is smaller (cap = 2^64 - 1: no limit).
// Printed: "status <s>", "sizes" (nodes, contigs, pieces, records, pieces of records), "info" (fgpu_tips_info field by field), then with status 0
//   N <key hex> <cov x 4> <slot x 5>
//   C <record> <node1 hex or -> <node2 hex or -> <bases> <ind1> <ind2> <isolated> : <call> <flip> ...
//   P <number> : <call> <flip> ...
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
static void put_pieces(const fgpu_join_piece* p, uint64_t a, uint64_t b) {
    for (uint64_t i = a; i < b; i++) printf(" %u %u", p[i].call, p[i].flip);
    printf("\n");
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
    fgpu_tips_out out;
    fgpu_tips_info info;
    memset(&out, 0, sizeof(out));
    memset(&info, 0, sizeof(info));
    const int sizing = fgpu_tips_plan(keys.data(), recs.data(), head[0], contigs.data(), calls.data(), head[1], kr[0], kr[1], &out, &info);
    printf("sizing %d\n", sizing);
    auto room = [&](uint64_t need) { return need < cap ? need : cap; };
    std::vector<fgpu_tips_node> nodes(room(out.n_nodes));
    std::vector<fgpu_tips_contig> tigs(room(out.n_contigs));
    std::vector<uint64_t> list_first(tigs.size() + 1), print_first(room(out.n_print) + 1);
    std::vector<fgpu_join_piece> pieces(room(out.n_pieces)), print_pieces(room(out.n_print_pieces));
    std::vector<uint32_t> number(print_first.size() - 1);
    memset(&out, 0, sizeof(out));
    out.nodes = nodes.data(); out.nodes_cap = nodes.size();
    out.contigs = tigs.data(); out.list_first = list_first.data(); out.contigs_cap = tigs.size();
    out.pieces = pieces.data(); out.pieces_cap = pieces.size();
    out.print_first = print_first.data(); out.print_number = number.data(); out.print_cap = number.size();
    out.print_pieces = print_pieces.data(); out.print_pieces_cap = print_pieces.size();
    memset(&info, 0, sizeof(info));
    const int status = fgpu_tips_plan(keys.data(), recs.data(), head[0], contigs.data(), calls.data(), head[1], kr[0], kr[1], &out, &info);
    printf("status %d\n", status);
    printf("sizes %llu %llu %llu %llu %llu\n", (unsigned long long)out.n_nodes, (unsigned long long)out.n_contigs, (unsigned long long)out.n_pieces,
           (unsigned long long)out.n_print, (unsigned long long)out.n_print_pieces);
    printf("info %llu %llu %llu %llu %llu %llu %llu %u %u %llu %llu %llu %llu %llu %llu\n", (unsigned long long)info.nodes_before, (unsigned long long)info.tips,
           (unsigned long long)info.back_tips, (unsigned long long)info.collapsed[0], (unsigned long long)info.collapsed[1], (unsigned long long)info.degenerate[0],
           (unsigned long long)info.degenerate[1], info.validated, info.changed, (unsigned long long)info.print.records, (unsigned long long)info.print.bubble_records,
           (unsigned long long)info.print.node_contigs, (unsigned long long)info.print.isolated_kept, (unsigned long long)info.print.isolated_dropped,
           (unsigned long long)info.print.nodes);
    if (status != FGPU_PLAN_OK) return 0;
    for (const auto& n : nodes)
        printf("N %llx %d %d %d %d %d %d %d %d %d\n", (unsigned long long)n.key, n.cov[0], n.cov[1], n.cov[2], n.cov[3], n.slot[0], n.slot[1], n.slot[2], n.slot[3], n.slot[4]);
    for (size_t c = 0; c < tigs.size(); c++) {
        const fgpu_tips_contig& t = tigs[c];
        char e1[24] = "-", e2[24] = "-";
        if (t.has1) snprintf(e1, sizeof(e1), "%llx", (unsigned long long)t.node1);
        if (t.has2) snprintf(e2, sizeof(e2), "%llx", (unsigned long long)t.node2);
        printf("C %zu %s %s %u %d %d %d :", c, e1, e2, t.len, t.ind1, t.ind2, t.isolated);
        put_pieces(pieces.data(), list_first[c], list_first[c + 1]);
    }
    for (size_t r = 0; r < number.size(); r++) {
        printf("P %u :", number[r]);
        put_pieces(print_pieces.data(), print_first[r], print_first[r + 1]);
    }
    return 0;
}
