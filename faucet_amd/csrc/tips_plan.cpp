// tips_plan.cpp — which piece lists ContigGraph::deleteTipsAndClean, and removeChimerasAndClean behind it, leave of a build's contigs, and which
// of them printContigs prints: the two host-only entry points over clean_graph.h, which holds the graph, the steps and the two serialisers (and
// cites the reference line by line).  No HIP, no text, no coverage list: a stand-alone CPU program can compile this file in
// (tests/host/tips_plan_check.cpp, tests/host/chimera_plan_check.cpp, under the sanitizers).
#include <cstdint>
#include <cstring>

#include "clean_graph.h"

namespace {

using namespace fgpu_graph;

bool bad_out(fgpu_tips_out* out) {
    if (!out) return true;
    out->n_nodes = out->n_contigs = out->n_pieces = out->n_print = out->n_print_pieces = 0;
    return (out->contigs_cap && out->contigs && !out->list_first) || (out->print_cap && out->print_number && !out->print_first);
}

// the print records, then the graph left: FGPU_PLAN_OK, FGPU_PLAN_UNSET (nothing of `out` is to be used) or FGPU_PLAN_SHORT
int records(CleanGraph& cg, fgpu_tips_out* out, fgpu_raw_info& print) {
    const int printed = cg.print_records(out, print);
    if (printed == FGPU_PLAN_UNSET) return printed;
    const int graph = cg.graph_records(out);
    return printed == FGPU_PLAN_OK && graph == FGPU_PLAN_OK ? FGPU_PLAN_OK : FGPU_PLAN_SHORT;
}

}  // namespace

extern "C" int fgpu_tips_plan(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls,
                              uint64_t n_calls, int32_t k, int32_t read_length, fgpu_tips_out* out, fgpu_tips_info* info) {
    if (bad_out(out)) return FGPU_PLAN_INPUT;
    CleanGraph cg;
    if (int st = cg.of_build(keys, recs, n_junctions, contigs, calls, n_calls, nullptr, k, read_length)) return st;
    fgpu_tips_info inf;
    memset(&inf, 0, sizeof(inf));
    if (int st = cg.delete_tips_and_clean(inf)) return st;
    const int st = records(cg, out, inf.print);
    if (st == FGPU_PLAN_UNSET) return st;
    if (info) *info = inf;
    return st;
}

extern "C" int fgpu_chimera_plan(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls,
                                 uint64_t n_calls, const fgpu_cov_summary* cov_calls, int32_t k, int32_t read_length, fgpu_tips_out* out,
                                 fgpu_tips_info* tips_info, fgpu_chimera_info* info) {
    if (bad_out(out) || (n_calls && !cov_calls)) return FGPU_PLAN_INPUT;
    static const fgpu_cov_summary none = {0, 0, 0, 0, {0, 0}};
    CleanGraph cg;
    if (int st = cg.of_build(keys, recs, n_junctions, contigs, calls, n_calls, cov_calls ? cov_calls : &none, k, read_length)) return st;
    fgpu_tips_info tips;
    fgpu_chimera_info inf;
    memset(&tips, 0, sizeof(tips));
    memset(&inf, 0, sizeof(inf));
    if (int st = cg.delete_tips_and_clean(tips)) return st;
    if (int st = cg.remove_chimeras_and_clean(inf)) return st;
    const int st = records(cg, out, inf.print);
    if (st == FGPU_PLAN_UNSET) return st;
    if (tips_info) *tips_info = tips;
    if (info) *info = inf;
    return st;
}
