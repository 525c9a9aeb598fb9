/* chimera_driver <bloom file> <bloom size request> <n_hash> <k> <j> <junctions file> <max read length> <fasta out> <graph out>
 *
 * TEST INFRASTRUCTURE ONLY (tests/golden/make_chimera_golden.py builds it against the compiled reference's objects; never shipped, never linked
 * into the product).  What the reference's graph is after the first two steps of ContigGraph::cleanGraph: a map reloaded with
 * JunctionMap::buildFromFile, JunctionMap::buildContigGraph, ContigGraph::setReadLength(max read length), ContigGraph::deleteTipsAndClean,
 * ContigGraph::removeChimerasAndClean, then ContigGraph::printContigs into <fasta out>.  Into <graph out>, before the print: "return <0|1>
 * <0|1>" (what the two steps returned), then the graph as tests/golden/detip_driver.cpp tables it --
 *   N <node k-mer, hex> <cov A> <cov C> <cov T> <cov G>          per node, in nodeMap's own iteration order
 *   S <slot> <bases> <ind1> <ind2> <node1> <node2> <avg>         per slot of that node that holds a contig; an end is the node's k-mer in hex,
 *                                                                "-" for none, "?" for a pointer to no node of the map; avg = getAvgCoverage
 *                                                                as %.17g
 *   I <bases> <ind1> <ind2> <avg>                                per isolated contig, in the list's order
 * What the steps print themselves (the counts of tips, of chimeric contigs and of nodes) goes to stdout, where the script reads it; a line
 * "== chimeras" is put between the two steps' output.  The map is reloaded from the same file as tests/golden/raw_contigs_driver.cpp reloads
 * it from, so its iteration order is the stored raw_contigs_<name>.order.gz.  nodeMap and isolated_contigs are private: the compile line
 * carries -fno-access-control.  No reference source text is copied here; this file only includes the reference headers. */
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unordered_map>
#include <vector>

#include "src/ContigGraph.h"
#include "utils/Bloom.h"
#include "utils/JChecker.h"
#include "utils/JunctionMap.h"
#include "utils/Kmer.h"

static void put_end(FILE* f, const std::unordered_map<const ContigNode*, unsigned long long>& key_of, const ContigNode* p) {
    if (!p) { fprintf(f, " -"); return; }
    auto at = key_of.find(p);
    if (at == key_of.end()) fprintf(f, " ?");
    else fprintf(f, " %llx", at->second);
}

int main(int argc, char** argv) {
    if (argc < 10) {
        fprintf(stderr, "usage: %s <bloom> <size request> <n_hash> <k> <j> <junctions> <max read length> <fasta out> <graph out>\n", argv[0]);
        return 2;
    }
    const int k = atoi(argv[4]), j = atoi(argv[5]), max_read_length = atoi(argv[7]);
    setSizeKmer(k);
    Bloom bloom((uint64_t)atoll(argv[2]), k);
    bloom.set_number_of_hash_func(atoi(argv[3]));
    bloom.load(argv[1]);
    JChecker jc(j, &bloom);
    JunctionMap jm(&bloom, &jc, max_read_length);
    jm.buildFromFile(argv[6]);
    ContigGraph* graph = jm.buildContigGraph();
    graph->setReadLength(max_read_length);
    const bool detipped = graph->deleteTipsAndClean();
    printf("== chimeras\n");
    const bool dechimered = graph->removeChimerasAndClean();
    fflush(stdout);
    FILE* f = fopen(argv[9], "w");
    if (!f) return 2;
    fprintf(f, "return %d %d\n", detipped ? 1 : 0, dechimered ? 1 : 0);
    std::unordered_map<const ContigNode*, unsigned long long> key_of;
    for (auto& kv : graph->nodeMap) key_of[&kv.second] = (unsigned long long)kv.first;
    for (auto& kv : graph->nodeMap) {
        ContigNode& nd = kv.second;
        fprintf(f, "N %llx %d %d %d %d\n", (unsigned long long)kv.first, (int)nd.cov[0], (int)nd.cov[1], (int)nd.cov[2], (int)nd.cov[3]);
        for (int i = 0; i < 5; i++) {
            Contig* c = nd.contigs[i];
            if (!c) continue;
            fprintf(f, "S %d %llu %d %d", i, (unsigned long long)c->getSeq().length(), (int)c->ind1, (int)c->ind2);
            put_end(f, key_of, c->node1_p);
            put_end(f, key_of, c->node2_p);
            fprintf(f, " %.17g\n", c->getAvgCoverage());
        }
    }
    for (auto& c : graph->isolated_contigs) fprintf(f, "I %llu %d %d %.17g\n", (unsigned long long)c.getSeq().length(), (int)c.ind1, (int)c.ind2, c.getAvgCoverage());
    fclose(f);
    graph->printContigs(argv[8]);
    fflush(stdout);
    return 0;
}
