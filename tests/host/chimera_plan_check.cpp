// chimera_plan_check plan <file> | live <file> [refusal] | fold <file>: fgpu_chimera_plan (faucet_amd/csrc/tips_plan.cpp over clean_graph.h) and the summary operations of
// faucet_amd/csrc/cov_summary.h as a stand-alone CPU program, for tests/test_dechimera_plan_cpu.py, which builds it under
// -fsanitize=address,undefined.  TEST ONLY.
// plan: the file is tips_plan_check's -- u64 junctions, u64 calls, i32 k, i32 read_length, u64 cap; the keys, the fgpu_junction records, the
// fgpu_contig and the fgpu_build_call arrays as the C ABI lays them out -- and behind them one fgpu_cov_summary per call.  The plan is asked twice:
// with no room at all, which says how much is needed ("sizing <status>"), then with exactly that much, or with `cap` entries per array where cap
// is smaller (cap = 2^64 - 1: no limit).  Printed: "status <s>", "sizes" (nodes, contigs, pieces, records, pieces of records), "info"
// (fgpu_chimera_info field by field), "tips" (fgpu_tips_info of the first step, without its print part), then with status 0
//   N <key hex> <cov x 4> <slot x 5>
//   C <record> <node1 hex or -> <node2 hex or -> <bases> <ind1> <ind2> <isolated> : <call> <flip> ...
//   P <number> : <call> <flip> ...
// live: plan's file and plan's output, byte for byte, made the way the device makes it (fgpu_stage3_detip, then fgpu_stage3_dechimera on the graph
// that call left): CleanGraph::of_build WITHOUT summaries, delete_tips_and_clean, the first step's print_records and graph_records (dropped),
// set_cov, remove_chimeras_and_clean, the second step's records.  Behind plan's lines, one line per contig the graph holds, numbered as the C
// lines are:
//   S0 <number> <sum> <n> <first> <last> : <call> <flip> ...     right behind set_cov: the summary it folded and the list it folded it over
//   S <number> <sum> <n> <first> <last>                          behind the step: the summary of contig record <number>
// With a refusal, "refused <status> ..." is printed behind the sizing line: no_summaries -- the step on a graph that was never given summaries;
// zero_entries -- set_cov with the middle call's n set to 0, and then the run goes on with the right summaries; short_calls -- set_cov with
// n_calls = the largest call a live list names (one short of it).
// fold: a text file, per line "L" or "R" and then per piece "<flip> <n> <n coverage entries>".  Every piece's summary is taken from its entries,
// reversed where flip is 1, and the summaries are folded with fgpu_cov_concatenate from the left (L: ((a b) c) d) or from the right (R: a (b (c
// d))).  Printed per line: "<sum> <n> <first> <last> <average %.17g>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../faucet_amd/csrc/clean_graph.h"
#include "../../faucet_amd/csrc/cov_summary.h"
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
typedef unsigned long long ull;

static int fold(FILE* f) {
    char way;
    while (fscanf(f, " %c", &way) == 1) {
        std::vector<fgpu_cov_summary> pieces;
        for (;;) {
            const int c = fgetc(f);
            if (c == '\n' || c == EOF) break;
            if (c == ' ') continue;
            ungetc(c, f);
            unsigned flip, n;
            if (fscanf(f, "%u %u", &flip, &n) != 2) return 2;
            fgpu_cov_summary s;
            memset(&s, 0, sizeof(s));
            for (unsigned i = 0; i < n; i++) {
                unsigned v;
                if (fscanf(f, "%u", &v) != 1) return 2;
                s.sum += v;
                if (i == 0) s.first = (uint8_t)v;
                s.last = (uint8_t)v;
            }
            s.n = n;
            pieces.push_back(flip ? fgpu_cov_reverse(s) : s);
        }
        if (pieces.empty()) return 2;
        fgpu_cov_summary r;
        if (way == 'L') {
            r = pieces[0];
            for (size_t i = 1; i < pieces.size(); i++) r = fgpu_cov_concatenate(r, pieces[i]);
        } else {
            r = pieces.back();
            for (size_t i = pieces.size() - 1; i-- > 0;) r = fgpu_cov_concatenate(pieces[i], r);
        }
        printf("%llu %u %u %u %.17g\n", (ull)r.sum, r.n, r.first, r.last, fgpu_cov_average(r));
    }
    return 0;
}

// ---- live: what fgpu_stage3_detip and fgpu_stage3_dechimera (faucet_amd/csrc/stage3_emit.hip) do with one CleanGraph, call by call
enum Refusal { NO_REFUSAL, NO_SUMMARIES, ZERO_ENTRIES, SHORT_CALLS };
static Refusal refusal = NO_REFUSAL;
static std::string s_lines;         // the S0 and S lines of the call that has room, printed behind everything else

// one line per contig the graph holds, numbered as graph_records numbers them (the nodes' slots in nodeMap's order, then isolated_contigs)
static void summaries(const fgpu_graph::CleanGraph& cg, const char* head, bool lists) {
    std::vector<char> seen(cg.tigs.size(), 0);
    uint64_t number = 0;
    auto line = [&](int64_t c) {
        if (c == fgpu_graph::NONE || seen[c]) return;
        seen[c] = 1;
        const fgpu_graph::Tig& t = cg.tigs[c];
        char buf[128];
        snprintf(buf, sizeof(buf), "%s %llu %llu %u %u %u", head, (ull)number++, (ull)t.cov.sum, t.cov.n, t.cov.first, t.cov.last);
        s_lines += buf;
        if (lists) {
            s_lines += " :";
            for (const auto& p : t.list) {
                snprintf(buf, sizeof(buf), " %u %u", p.call, p.flip);
                s_lines += buf;
            }
        }
        s_lines += "\n";
    };
    for (const auto& kv : cg.g.node_map)
        for (int i = 0; i < 5; i++) line(kv.second.contigs[i]);
    for (int64_t c : cg.isolated) line(c);
}

// a step's two serialisers as tips_plan.cpp calls them: the print records, then the graph left
static int records(fgpu_graph::CleanGraph& cg, fgpu_tips_out* out, fgpu_raw_info& print) {
    const int printed = cg.print_records(out, print);
    if (printed == FGPU_PLAN_UNSET) return printed;
    const int graph = cg.graph_records(out);
    return printed == FGPU_PLAN_OK && graph == FGPU_PLAN_OK ? FGPU_PLAN_OK : FGPU_PLAN_SHORT;
}

// fgpu_chimera_plan's arguments and results, by the device's path: the graph is built WITHOUT summaries, detipped, serialised, and only then
// given the summaries (CleanGraph::set_cov), and the second step runs on that same object
static int live_plan(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls, uint64_t n_calls,
                     const fgpu_cov_summary* cov_calls, int32_t k, int32_t read_length, fgpu_tips_out* out, fgpu_tips_info* tips_info, fgpu_chimera_info* info) {
    using namespace fgpu_graph;
    const bool say = tips_info != nullptr;                           // (the second of main's two calls)
    out->n_nodes = out->n_contigs = out->n_pieces = out->n_print = out->n_print_pieces = 0;
    CleanGraph cg;
    if (int st = cg.of_build(keys, recs, n_junctions, contigs, calls, n_calls, nullptr, k, read_length)) return st;
    fgpu_tips_info tips;
    fgpu_chimera_info inf;
    memset(&tips, 0, sizeof(tips));
    memset(&inf, 0, sizeof(inf));
    if (int st = cg.delete_tips_and_clean(tips)) return st;
    {   // the first step's records: asked for their sizes, then written into exactly that room, and dropped
        fgpu_tips_out need;
        memset(&need, 0, sizeof(need));
        if (records(cg, &need, tips.print) == FGPU_PLAN_UNSET) return FGPU_PLAN_UNSET;
        std::vector<fgpu_tips_node> nodes(need.n_nodes);
        std::vector<fgpu_tips_contig> tigs(need.n_contigs);
        std::vector<uint64_t> list_first(tigs.size() + 1), print_first(need.n_print + 1);
        std::vector<fgpu_join_piece> pieces(need.n_pieces), print_pieces(need.n_print_pieces);
        std::vector<uint32_t> number(need.n_print);
        fgpu_tips_out first;
        memset(&first, 0, sizeof(first));
        first.nodes = nodes.data(); first.nodes_cap = nodes.size();
        first.contigs = tigs.data(); first.list_first = list_first.data(); first.contigs_cap = tigs.size();
        first.pieces = pieces.data(); first.pieces_cap = pieces.size();
        first.print_first = print_first.data(); first.print_number = number.data(); first.print_cap = number.size();
        first.print_pieces = print_pieces.data(); first.print_pieces_cap = print_pieces.size();
        if (records(cg, &first, tips.print) != FGPU_PLAN_OK) return FGPU_PLAN_INPUT;
    }
    if (refusal == NO_SUMMARIES) {
        const int st = cg.remove_chimeras_and_clean(inf);
        if (say) { printf("refused %d\n", st); }
        return st;
    }
    if (refusal == ZERO_ENTRIES && n_calls) {                        // one summary of no entries, in the middle: refused, and nothing written ...
        std::vector<fgpu_cov_summary> bad(cov_calls, cov_calls + n_calls);
        bad[n_calls / 2].n = 0;
        const int st = cg.set_cov(bad.data(), n_calls);
        if (say) { printf("refused %d have_cov %d\n", st, (int)cg.have_cov); }
        if (st == FGPU_PLAN_OK) return FGPU_PLAN_INPUT;
    }                                                                // ... so the right summaries behind it give what they give alone
    if (refusal == SHORT_CALLS) {                                    // n_calls one short of the largest call a list of the graph names
        uint64_t largest = 0;
        bool any = false;
        for (const Tig& t : cg.tigs)
            for (const auto& p : t.list)
                if (t.alive) { any = true; largest = p.call > largest ? p.call : largest; }
        const int st = any ? cg.set_cov(cov_calls, largest) : FGPU_PLAN_OK;
        if (say) { printf("refused %d have_cov %d named %d\n", st, (int)cg.have_cov, (int)any); }
        return st ? st : FGPU_PLAN_INPUT;
    }
    if (int st = cg.set_cov(cov_calls, n_calls)) return st;
    if (say) summaries(cg, "S0", true);
    if (int st = cg.remove_chimeras_and_clean(inf)) return st;
    const int st = records(cg, out, inf.print);
    if (st == FGPU_PLAN_UNSET) return st;
    if (say) summaries(cg, "S", false);
    if (tips_info) *tips_info = tips;
    if (info) *info = inf;
    return st;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    if (!strcmp(argv[1], "fold")) {
        const int rc = fold(f);
        fclose(f);
        return rc;
    }
    const bool live = !strcmp(argv[1], "live");
    if (live && argc > 3) {
        refusal = !strcmp(argv[3], "no_summaries") ? NO_SUMMARIES : !strcmp(argv[3], "zero_entries") ? ZERO_ENTRIES : !strcmp(argv[3], "short_calls") ? SHORT_CALLS : NO_REFUSAL;
        if (refusal == NO_REFUSAL) return 2;
    }
    const auto plan = live ? live_plan : fgpu_chimera_plan;
    uint64_t head[2], cap = 0;
    int32_t kr[2];
    if (fread(head, 8, 2, f) != 2 || fread(kr, 4, 2, f) != 2 || fread(&cap, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> keys;
    std::vector<fgpu_junction> recs;
    std::vector<fgpu_contig> contigs;
    std::vector<fgpu_build_call> calls;
    std::vector<fgpu_cov_summary> covs;
    if (!get(f, keys, head[0]) || !get(f, recs, head[0]) || !get(f, contigs, head[1]) || !get(f, calls, head[1]) || !get(f, covs, head[1])) return 2;
    fclose(f);
    fgpu_tips_out out;
    fgpu_tips_info tips;
    fgpu_chimera_info info;
    memset(&out, 0, sizeof(out));
    const int sizing = plan(keys.data(), recs.data(), head[0], contigs.data(), calls.data(), head[1], covs.data(), kr[0], kr[1], &out, nullptr, nullptr);
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
    memset(&tips, 0, sizeof(tips));
    memset(&info, 0, sizeof(info));
    const int status = plan(keys.data(), recs.data(), head[0], contigs.data(), calls.data(), head[1], covs.data(), kr[0], kr[1], &out, &tips, &info);
    printf("status %d\n", status);
    printf("sizes %llu %llu %llu %llu %llu\n", (ull)out.n_nodes, (ull)out.n_contigs, (ull)out.n_pieces, (ull)out.n_print, (ull)out.n_print_pieces);
    printf("info %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", (ull)info.nodes_before, (ull)info.removed, (ull)info.cut_near, (ull)info.cut_far, (ull)info.cut_both,
           (ull)info.collapsed[0], (ull)info.collapsed[1], (ull)info.degenerate[0], (ull)info.degenerate[1], (ull)info.collapsed_after_cut);
    for (int i = 0; i < 6; i++) printf(" %llu", (ull)info.skipped[i]);
    printf(" %u %u %llu %llu %llu %llu %llu %llu\n", info.validated, info.changed, (ull)info.print.records, (ull)info.print.bubble_records, (ull)info.print.node_contigs,
           (ull)info.print.isolated_kept, (ull)info.print.isolated_dropped, (ull)info.print.nodes);
    printf("tips %llu %llu %llu %llu %llu %llu %llu %u %u\n", (ull)tips.nodes_before, (ull)tips.tips, (ull)tips.back_tips, (ull)tips.collapsed[0], (ull)tips.collapsed[1],
           (ull)tips.degenerate[0], (ull)tips.degenerate[1], tips.validated, tips.changed);
    if (status != FGPU_PLAN_OK) { fputs(s_lines.c_str(), stdout); return 0; }
    for (const auto& n : nodes)
        printf("N %llx %d %d %d %d %d %d %d %d %d\n", (ull)n.key, n.cov[0], n.cov[1], n.cov[2], n.cov[3], n.slot[0], n.slot[1], n.slot[2], n.slot[3], n.slot[4]);
    for (size_t c = 0; c < tigs.size(); c++) {
        const fgpu_tips_contig& t = tigs[c];
        char e1[24] = "-", e2[24] = "-";
        if (t.has1) snprintf(e1, sizeof(e1), "%llx", (ull)t.node1);
        if (t.has2) snprintf(e2, sizeof(e2), "%llx", (ull)t.node2);
        printf("C %zu %s %s %u %d %d %d :", c, e1, e2, t.len, t.ind1, t.ind2, t.isolated);
        put_pieces(pieces.data(), list_first[c], list_first[c + 1]);
    }
    for (size_t r = 0; r < number.size(); r++) {
        printf("P %u :", number[r]);
        put_pieces(print_pieces.data(), print_first[r], print_first[r + 1]);
    }
    fputs(s_lines.c_str(), stdout);
    return 0;
}
