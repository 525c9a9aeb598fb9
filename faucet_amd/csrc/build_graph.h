// build_graph.h — the reference's ContigGraph as JunctionMap::buildContigGraph returns it, made from the calls of a finished fgpu_stage3_build
// instead of from Contig objects: host logic only (no HIP, no text), shared by raw_plan.cpp (which prints it) and tips_plan.cpp (which cleans it
// first).
//   nodeMap / ContigGraph::createContigNode        src/ContigGraph.cpp:1656, called at utils/JunctionMap.cpp:42 and :66
//   ContigNode(Junction), setCoverage              src/ContigNode.cpp:13-19, utils/JunctionMap.cpp:43-47
//   Contig::setEnds                                src/Contig.cpp:123-133, called at utils/JunctionMap.cpp:60, :67, :73
//   addIsolatedContig(backward->concatenate(..))   utils/JunctionMap.cpp:120
// nodeMap is a real std::unordered_map<uint64_t, ...> that takes the same inserts in the same order: the passes over it go in the container's
// own iteration order, which is the library's business (faucet_amd/host/junction_order.h restates it for the dump order of the junctions;
// here the container itself is asked).
#ifndef FGPU_BUILD_GRAPH_H
#define FGPU_BUILD_GRAPH_H
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../../include/faucet_gpu.h"

namespace fgpu_graph {

const int64_t NONE = -1;

struct Node {
    uint8_t cov[4];
    int64_t contigs[5];      // call numbers (Contig*), NONE = nullptr
};

// k-mer -> row of the map: looked up, never iterated, so its order is nobody's business (open addressing, at most half full)
struct Rows {
    std::vector<uint64_t> key;
    std::vector<uint32_t> row;           // 0 = free, else row + 1
    uint64_t mask = 0;
    static uint64_t mix(uint64_t x) { x ^= x >> 31; x *= 0x9E3779B97F4A7C15ULL; return x ^ (x >> 29); }
    Rows(const uint64_t* keys, uint64_t n) {
        uint64_t slots = 16;
        while (slots < 2 * n) slots <<= 1;
        mask = slots - 1;
        key.assign(slots, 0);
        row.assign(slots, 0);
        for (uint64_t r = 0; r < n; r++) {
            uint64_t at = mix(keys[r]) & mask;
            while (row[at]) at = (at + 1) & mask;
            key[at] = keys[r];
            row[at] = (uint32_t)(r + 1);
        }
    }
    int64_t find(uint64_t x) const {
        for (uint64_t at = mix(x) & mask; row[at]; at = (at + 1) & mask)
            if (key[at] == x) return (int64_t)row[at] - 1;
        return NONE;
    }
};

struct Ends {                // Contig::node1_p, node2_p (keys of nodeMap, has = 0: nullptr)
    uint64_t node1 = 0, node2 = 0;
    bool has1 = false, has2 = false, mark = false;
};

// Contig::getSide(node): 1 if node1_p is the node (tested first), 2 if node2_p is, -1 otherwise
inline int side_of(const Ends& e, uint64_t node) {
    if (e.has1 && e.node1 == node) return 1;
    if (e.has2 && e.node2 == node) return 2;
    return -1;
}

struct Graph {
    std::unordered_map<uint64_t, Node> node_map;             // nodeMap
    std::vector<Ends> ends;                                  // per call
    std::vector<uint64_t> isolated;                          // the forward call of each linear region; the backward one follows it
};

// FGPU_PLAN_OK, or FGPU_PLAN_INPUT where the arrays are not a finished build of this map
inline int of_build(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls,
                    uint64_t n_calls, int32_t k, Graph& g) {
    if ((n_junctions && (!keys || !recs)) || (n_calls && (!contigs || !calls)) || k < 1 || k > 31 || n_calls >= (1ULL << 32) || n_junctions >= (1ULL << 32) - 1)
        return FGPU_PLAN_INPUT;
    for (uint64_t c = 0; c < n_calls; c++)
        if (contigs[c].status != 0 || contigs[c].len < (uint32_t)k || contigs[c].ind1 < 0 || contigs[c].ind1 > 4 || contigs[c].ind2 < 0 || contigs[c].ind2 > 4 ||
            calls[c].phase > FGPU_BUILD_LINEAR_BACKWARD)
            return FGPU_PLAN_INPUT;
    const Rows row_of(keys, n_junctions);
    g.ends.assign(n_calls, Ends());
    auto create_node = [&](uint64_t kmer, const fgpu_junction& j) -> Node* {
        Node nd;
        for (int i = 0; i < 4; i++) nd.cov[i] = j.cov[i];
        for (int i = 0; i < 5; i++) nd.contigs[i] = NONE;
        return &g.node_map.insert(std::make_pair(kmer, nd)).first->second;
    };
    // ---- buildBranchingPaths: the loop over the map in map order; the calls that were made come in the same order
    uint64_t c = 0;
    for (uint64_t r = 0; r < n_junctions; r++) {
        int paths = 0;
        for (int i = 0; i < 4; i++) paths += recs[r].cov[i] > 0;
        if (paths <= 1) continue;
        const uint64_t kmer = keys[r];
        Node* start = create_node(kmer, recs[r]);
        bool homopolymer = true;                             // isHomoPolymer(print_kmer(kmer)): every base is the first one
        const int first = (int)((kmer >> (2 * (k - 1))) & 3);
        for (int b = 0; b < k; b++) homopolymer = homopolymer && (int)((kmer >> (2 * b)) & 3) == first;
        if (homopolymer) start->cov[first] = 0;
        for (; c < n_calls && calls[c].phase == FGPU_BUILD_BRANCHING && calls[c].start_kmer == kmer; c++) {
            Ends& e = g.ends[c];
            const int i1 = contigs[c].ind1, i2 = contigs[c].ind2;
            e.node1 = kmer; e.has1 = true;
            if (calls[c].far_is_junction && calls[c].far_is_start) {
                e.node2 = kmer; e.has2 = true;
                start->contigs[i1] = (int64_t)c;
                start->contigs[i2] = (int64_t)c;
            } else if (calls[c].far_is_junction) {
                const int64_t far = row_of.find(calls[c].far_kmer);
                if (far == NONE) return FGPU_PLAN_INPUT;
                Node* other = create_node(calls[c].far_kmer, recs[far]);      // (may rehash: pointers to the container's nodes stay valid)
                e.node2 = calls[c].far_kmer; e.has2 = true;
                start->contigs[i1] = (int64_t)c;
                other->contigs[i2] = (int64_t)c;
            } else {
                start->contigs[i1] = (int64_t)c;
            }
        }
    }
    if (c < n_calls && calls[c].phase == FGPU_BUILD_BRANCHING) return FGPU_PLAN_INPUT;      // a start that is no complex junction of this map, or out of order
    // ---- buildLinearRegions: forward, backward, forward, backward
    for (; c < n_calls; c += 2) {
        if (calls[c].phase != FGPU_BUILD_LINEAR_FORWARD || c + 1 >= n_calls || calls[c + 1].phase != FGPU_BUILD_LINEAR_BACKWARD ||
            calls[c + 1].start_kmer != calls[c].start_kmer)
            return FGPU_PLAN_INPUT;
        g.isolated.push_back(c);
    }
    return FGPU_PLAN_OK;
}

}  // namespace fgpu_graph
#endif
