// raw_plan.cpp — which contigs ContigGraph::printContigs prints, and in which order: host logic only (no HIP, no text), so that a
// stand-alone CPU program can compile it in (tests/host/raw_plan_check.cpp, under the sanitizers).
//
// The reference's graph, made from the calls of a finished fgpu_stage3_build instead of from Contig objects, is build_graph.h's (shared with
// tips_plan.cpp); here its two printing passes:
//   printAndMarkBubbleContigs, isBubbleNode        src/ContigGraph.cpp:1543-1580, :490-503, allSame :153-162
//   getNewConcatenatedContig, Contig::getSide      src/ContigGraph.cpp:1509-1530, src/Contig.cpp:243-253
//   printUnmarkedUnitigs                           src/ContigGraph.cpp:1605-1645
#include <cstdint>
#include <vector>

#include "build_graph.h"

namespace {

using namespace fgpu_graph;

struct Plan {
    fgpu_fasta_seq* out = nullptr;
    uint64_t cap = 0, n = 0;
    void put(const fgpu_contig* c, int64_t a, bool flip_a, int64_t b, bool flip_b) {
        if (n < cap) {
            fgpu_fasta_seq s = {};
            s.text_word[0] = c[a].text_word; s.len[0] = c[a].len; s.flip[0] = flip_a ? 1 : 0;
            s.pieces = 1;
            if (b != NONE) { s.text_word[1] = c[b].text_word; s.len[1] = c[b].len; s.flip[1] = flip_b ? 1 : 0; s.pieces = 2; }
            s.number = (uint32_t)(n + 1);
            out[n] = s;
        }
        n++;
    }
};

}  // namespace

extern "C" int fgpu_raw_plan(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls,
                             uint64_t n_calls, int32_t k, int32_t read_length, fgpu_fasta_seq* out, uint64_t cap, uint64_t* n_out, fgpu_raw_info* info) {
    if ((cap && !out) || !n_out) return FGPU_PLAN_INPUT;
    *n_out = 0;
    Graph g;
    if (int st = of_build(keys, recs, n_junctions, contigs, calls, n_calls, k, g)) return st;
    auto& node_map = g.node_map;
    auto& ends = g.ends;
    const std::vector<uint64_t>& isolated = g.isolated;
    // ---- printAndMarkBubbleContigs
    Plan plan;
    plan.out = out;
    plan.cap = cap;
    fgpu_raw_info inf = {};
    inf.nodes = node_map.size();
    for (auto& kv : node_map) {
        const uint64_t node = kv.first;
        Node& nd = kv.second;
        int paths = 0;
        for (int i = 0; i < 4; i++) paths += nd.cov[i] > 0;
        if (paths != 2) continue;                            // isBubbleNode
        bool first_far = true, same = true, far_has = false;
        uint64_t far_key = 0;
        for (int i = 0; i < 4; i++) {
            if (!(nd.cov[i] > 0)) continue;
            if (nd.contigs[i] == NONE) return FGPU_PLAN_UNSET;          // tig->otherEndNode(node) on a null tig
            const Ends& e = ends[nd.contigs[i]];
            const int side = side_of(e, node);
            const bool has = side == 1 ? e.has2 : side == 2 ? e.has1 : false;
            const uint64_t key = side == 1 ? e.node2 : e.node1;
            if (first_far) { far_has = has; far_key = has ? key : 0; first_far = false; }
            else same = has == far_has && (!has || key == far_key);
        }
        if (!same || !far_has) continue;                     // allSame (:153-162): two null nodes are not the same
        const int64_t back = nd.contigs[4];
        if (back == NONE) return FGPU_PLAN_UNSET;                       // back->getSeq() on a null back
        if (!(contigs[back].len < 250)) continue;
        bool back_mark = false;
        for (int i = 0; i < 4; i++) {
            const int64_t tig = nd.contigs[i];
            if (tig == NONE || ends[tig].mark) continue;
            if (!ends[back].mark) {
                plan.put(contigs, back, side_of(ends[back], node) == 1, tig, side_of(ends[tig], node) == 2);
                inf.bubble_records++;
                back_mark = true;
                ends[tig].mark = true;
            }
        }
        if (back_mark) ends[back].mark = true;
    }
    // ---- printUnmarkedUnitigs
    for (auto& kv : node_map) {
        Node& nd = kv.second;
        for (int i = 0; i < 5; i++) {
            const int64_t tig = nd.contigs[i];
            if (tig == NONE || ends[tig].mark) continue;
            plan.put(contigs, tig, false, NONE, false);
            inf.node_contigs++;
            ends[tig].mark = true;
        }
    }
    for (uint64_t f : isolated) {
        const uint64_t len = (uint64_t)contigs[f + 1].len - (uint64_t)k + contigs[f].len;
        if (len >= (uint64_t)(int64_t)read_length) {                   // (size_t >= int: the int goes to unsigned)
            plan.put(contigs, (int64_t)(f + 1), true, (int64_t)f, false);
            inf.isolated_kept++;
        } else {
            inf.isolated_dropped++;
        }
    }
    inf.records = plan.n;
    *n_out = plan.n;
    if (info) *info = inf;
    return plan.n > cap ? FGPU_PLAN_SHORT : FGPU_PLAN_OK;
}
