// fastg_plan_check fmt | plan <file> <raw|detip|dechimera> [<change> <contig>]: CleanGraph::fastg_records (faucet_amd/csrc/clean_graph.h: ContigGraph::printGraph's
// walk) and the name function of faucet_amd/csrc/fastg_name.h as a stand-alone CPU program, for tests/test_fastg_plan_cpu.py, which builds it under
// -fsanitize=address,undefined and runs it directly.  TEST ONLY.
// fmt: fgpu_fastg_g against snprintf("%g") of (double) sum / (double) n -- every (sum, n) with n <= 300 and sum <= 255 n, 10^6 seeded pairs with n up to
// 2^32 - 1, and the traps named in main.  Prints "checked <pairs> mismatches <m>" and the first mismatches.
// plan: the file is chimera_plan_check's -- u64 junctions, u64 calls, i32 k, i32 read_length, u64 cap (not read); the keys, the fgpu_junction records, the
// fgpu_contig, fgpu_build_call and fgpu_cov_summary arrays -- and behind them per call u32 bases and that many letters.  The graph is made the way
// the device makes it: raw -- of_build with the summaries; detip -- of_build WITHOUT them, delete_tips_and_clean, set_cov; dechimera -- then
// remove_chimeras_and_clean.  Printed: "status <s>", "info <node_records> <isolated_printed> <isolated_listed> <nodes>", per contig the graph holds,
// numbered as CleanGraph::graph_records numbers them (the nodes' slots in nodeMap's order, then isolated_contigs),
//   C <tig> <bases> <sum> <n> : <call> <flip> ...
// per record of the file
//   R <tig> <neighbours of the primed header> <record> <primed> ... <neighbours of the other> <record> <primed> ...
// and "TEXT <bytes>" with the whole file behind it, rendered on the host: the pieces' letters joined as ContigJuncList::concatenate joins them, the
// names by fgpu_fastg_name.  A change is made to the graph by hand right before the walk, on the contig numbered <contig> as the C lines number
// them: dead -- the contig is deleted where it hangs; noend -- its ind1 becomes another index; gone -- the node at its second end is erased;
// nowhere -- the slot at its first end is emptied, so that the walk prints it nowhere while it is still a neighbour at its second end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../faucet_amd/csrc/clean_graph.h"
#include "../../faucet_amd/csrc/cov_summary.h"
#include "../../faucet_amd/csrc/fastg_name.h"
#include "../../include/faucet_gpu.h"

typedef unsigned long long ull;

static uint64_t checked = 0, mismatches = 0;
static void check(uint64_t sum, uint32_t n) {
    char want[64], got[32];
    snprintf(want, sizeof(want), "%g", (double)sum / (double)n);
    const uint32_t len = fgpu_fastg_g(sum, n, got);
    checked++;
    if (len > 11 || len != strlen(want) || memcmp(want, got, len) != 0) {
        if (mismatches++ < 20) printf("mismatch %llu / %u: %%g says %s, the function %.*s\n", (ull)sum, n, want, (int)(len > 31 ? 31 : len), got);
    }
}
static int fmt() {
    for (uint32_t n = 1; n <= 300; n++)
        for (uint64_t sum = 0; sum <= 255ULL * n; sum++) check(sum, n);
    uint64_t x = 0x9E3779B97F4A7C15ULL;                                       // splitmix64
    auto next = [&]() {
        uint64_t z = (x += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    };
    for (int i = 0; i < 1000000; i++) {
        const uint32_t bits = 1 + (uint32_t)(next() % 32);                    // every magnitude of n alike
        uint32_t n = (uint32_t)(next() >> (64 - bits));
        if (!n) n = 1;
        const uint64_t r = next();
        const uint64_t sum = (i & 3) == 0 ? r % (n < 1000 ? n : 1000) : r % (255ULL * n + 1);     // (one in four: the small averages, where the exponent form begins)
        check(sum, n);
    }
    const uint64_t traps[][2] = {{200001, 200000}, {1601, 16}, {1, 100000}, {0, 7}, {0, 4294967295ULL}, {255, 1}, {23, 2}, {1, 4294967295ULL},
                                 {255ULL * 4294967295ULL, 4294967295ULL}, {1, 10000}, {9999995, 10000000}, {99999950, 1000000}, {1, 10}, {999999, 10000000}};
    for (const auto& t : traps) check(t[0], (uint32_t)t[1]);
    printf("checked %llu mismatches %llu\n", (ull)checked, (ull)mismatches);
    return 0;
}

template <class T>
static bool get(FILE* f, std::vector<T>& v, uint64_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
static std::string revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}

int main(int argc, char** argv) {
    using namespace fgpu_graph;
    if (argc >= 2 && !strcmp(argv[1], "fmt")) return fmt();
    if (argc < 4 || strcmp(argv[1], "plan")) return 2;
    const std::string step = argv[3], change = argc > 5 ? argv[4] : "";
    const uint64_t changed = argc > 5 ? strtoull(argv[5], nullptr, 10) : 0;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint64_t head[2], cap = 0;
    int32_t kr[2];
    if (fread(head, 8, 2, f) != 2 || fread(kr, 4, 2, f) != 2 || fread(&cap, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> keys;
    std::vector<fgpu_junction> recs;
    std::vector<fgpu_contig> contigs;
    std::vector<fgpu_build_call> calls;
    std::vector<fgpu_cov_summary> covs;
    if (!get(f, keys, head[0]) || !get(f, recs, head[0]) || !get(f, contigs, head[1]) || !get(f, calls, head[1]) || !get(f, covs, head[1])) return 2;
    std::vector<std::string> letters(head[1]);
    for (auto& s : letters) {
        uint32_t len;
        if (fread(&len, 4, 1, f) != 1) return 2;
        s.resize(len);
        if (len && fread(&s[0], 1, len, f) != len) return 2;
    }
    fclose(f);
    const int32_t k = kr[0];
    const fgpu_cov_summary none = {0, 0, 0, 0, {0, 0}};
    const fgpu_cov_summary* cv = covs.empty() ? &none : covs.data();
    CleanGraph cg;
    int st = cg.of_build(keys.data(), recs.data(), head[0], contigs.data(), calls.data(), head[1], step == "raw" ? cv : nullptr, k, kr[1]);
    if (st == FGPU_PLAN_OK && step != "raw") {
        fgpu_tips_info tips;
        memset(&tips, 0, sizeof(tips));
        st = cg.delete_tips_and_clean(tips);
        if (st == FGPU_PLAN_OK) st = cg.set_cov(cv, head[1]);
        if (st == FGPU_PLAN_OK && step == "dechimera") {
            fgpu_chimera_info inf;
            memset(&inf, 0, sizeof(inf));
            st = cg.remove_chimeras_and_clean(inf);
        }
    }
    if (st != FGPU_PLAN_OK) { printf("status %d\n", st); return 0; }
    std::vector<int64_t> numbered;                                            // the contigs the graph holds, as graph_records numbers them
    {
        std::vector<char> seen(cg.tigs.size(), 0);
        auto take = [&](int64_t c) {
            if (c == NONE || seen[c]) return;
            seen[c] = 1;
            numbered.push_back(c);
        };
        for (const auto& kv : cg.g.node_map)
            for (int i = 0; i < 5; i++) take(kv.second.contigs[i]);
        for (int64_t c : cg.isolated) take(c);
    }
    if (!change.empty()) {
        if (changed >= numbered.size()) return 2;
        Tig& t = cg.tigs[numbered[changed]];
        if (change == "dead") t.alive = false;
        else if (change == "noend") t.ind1 = (t.ind1 + 1) % 5 == t.ind2 ? (t.ind1 + 2) % 5 : (t.ind1 + 1) % 5;
        else if (change == "gone") { if (!t.has2) return 2; cg.g.node_map.erase(t.node2); }
        else if (change == "nowhere") {                                       // the slot at its first end lets go of it: it hangs at its second end only
            if (!t.has1 || !t.has2 || t.node1 == t.node2 || t.ind1 > 4) return 2;
            cg.g.node_map.find(t.node1)->second.contigs[t.ind1] = NONE;
        }
        else return 2;
    }
    const bool unset_before = cg.unset;
    FastgPlan plan;
    const CleanGraph& read_only = cg;
    st = read_only.fastg_records(plan);
    if (cg.unset != unset_before) { printf("the walk changed the graph\n"); return 1; }
    printf("status %d\n", st);
    if (st != FGPU_PLAN_OK) return 0;
    printf("info %llu %llu %llu %llu\n", (ull)plan.info.node_records, (ull)plan.info.isolated_printed, (ull)plan.info.isolated_listed, (ull)plan.info.nodes);
    for (int64_t c : numbered) {
        const Tig& t = cg.tigs[c];
        printf("C %lld %llu %llu %u :", (long long)c, (ull)t.len, (ull)t.cov.sum, t.cov.n);
        for (const auto& p : t.list) printf(" %u %u", p.call, p.flip);
        printf("\n");
    }
    if (plan.nbr_first.size() != 2 * plan.tig.size() + 1 || plan.nbr_first.back() != plan.nbr.size()) { printf("no CSR\n"); return 1; }
    for (size_t r = 0; r < plan.tig.size(); r++) {
        printf("R %lld", (long long)plan.tig[r]);
        for (int h = 0; h < 2; h++) {
            const uint64_t a = plan.nbr_first[2 * r + h], b = plan.nbr_first[2 * r + h + 1];
            printf(" %llu", (ull)(b - a));
            for (uint64_t e = a; e < b; e++) printf(" %u %u", plan.nbr[e] & ~FGPU_FASTG_PRIMED, plan.nbr[e] >> 31);
        }
        printf("\n");
    }
    // the whole file on the host
    std::vector<std::string> names(plan.tig.size()), seqs(plan.tig.size());
    for (size_t r = 0; r < plan.tig.size(); r++) {
        const Tig& t = cg.tigs[plan.tig[r]];
        char buf[FGPU_FASTG_NAME_STRIDE];
        const uint32_t len = fgpu_fastg_name((uint64_t)plan.tig[r], (uint32_t)t.len, t.cov.sum, t.cov.n, buf);
        if (len > FGPU_FASTG_NAME_MAX) { printf("a name of %u characters\n", len); return 1; }
        names[r].assign(buf, len);
        for (size_t p = 0; p < t.list.size(); p++) {                          // ContigJuncList::concatenate: first.substr(0, len - k) + second
            if (t.list[p].call >= letters.size()) return 2;
            const std::string s = t.list[p].flip ? revcomp(letters[t.list[p].call]) : letters[t.list[p].call];
            seqs[r] += p + 1 < t.list.size() ? s.substr(0, s.size() - (size_t)k) : s;
        }
        if (seqs[r].size() != t.len) { printf("record %zu joins to %zu bases, the graph says %llu\n", r, seqs[r].size(), (ull)t.len); return 1; }
    }
    std::string text;
    for (size_t r = 0; r < plan.tig.size(); r++)
        for (int h = 0; h < 2; h++) {
            text += ">" + names[r] + (h == 0 ? "'" : "");
            const uint64_t a = plan.nbr_first[2 * r + h], b = plan.nbr_first[2 * r + h + 1];
            for (uint64_t e = a; e < b; e++) {
                text += e == a ? ":" : ",";
                text += names[plan.nbr[e] & ~FGPU_FASTG_PRIMED];
                if (plan.nbr[e] >> 31) text += "'";
            }
            text += ";\n";
            text += h == 0 ? seqs[r] : revcomp(seqs[r]);
            text += "\n";
        }
    printf("TEXT %zu\n", text.size());
    fwrite(text.data(), 1, text.size(), stdout);
    return 0;
}
