// host_dechimera.cpp — the host's part of fgpu_stage3_dechimera timed piece by piece, for scripts/stage3_dechimera_times.py: the graph of a build made
// and detipped without coverages (as fgpu_stage3_detip leaves it alive in the context; neither is part of the step), then what the call does on the
// host, each under a clock of its own -- the summaries folded into the live contigs (set_cov), removeChimerasAndClean, printContigs' two passes
// (print_records, into room that suffices).  Measurement only: the script compiles it into a temporary shared object over clean_graph.h itself;
// nothing of the product links it.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../faucet_amd/csrc/clean_graph.h"

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ms[0..4]: graph, detip, set_cov, the step, print_records.  counts[0..2]: chimeric extensions removed, nodes left, records.  A plan status.
extern "C" int host_dechimera_times(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls,
                                    uint64_t n_calls, const fgpu_cov_summary* cov_calls, int32_t k, int32_t read_length, double* ms, uint64_t* counts) {
    fgpu_graph::CleanGraph cg;
    fgpu_tips_info tips;
    fgpu_chimera_info inf;
    memset(&tips, 0, sizeof(tips));
    memset(&inf, 0, sizeof(inf));
    double t = now_ms();
    if (int st = cg.of_build(keys, recs, n_junctions, contigs, calls, n_calls, nullptr, k, read_length)) return st;
    ms[0] = now_ms() - t; t = now_ms();
    if (int st = cg.delete_tips_and_clean(tips)) return st;
    ms[1] = now_ms() - t; t = now_ms();
    if (int st = cg.set_cov(cov_calls, n_calls)) return st;
    ms[2] = now_ms() - t; t = now_ms();
    if (int st = cg.remove_chimeras_and_clean(inf)) return st;
    ms[3] = now_ms() - t; t = now_ms();
    std::vector<uint64_t> first(n_calls + 1);                        // (the room the call gives it, made under the clock as there)
    std::vector<uint32_t> numbers(n_calls);
    std::vector<fgpu_join_piece> pieces(2 * n_calls);
    fgpu_tips_out out;
    memset(&out, 0, sizeof(out));
    out.print_first = first.data(); out.print_number = numbers.data(); out.print_cap = numbers.size();
    out.print_pieces = pieces.data(); out.print_pieces_cap = pieces.size();
    const int st = cg.print_records(&out, inf.print);
    ms[4] = now_ms() - t;
    counts[0] = inf.removed; counts[1] = inf.print.nodes; counts[2] = inf.print.records;
    return st;
}
