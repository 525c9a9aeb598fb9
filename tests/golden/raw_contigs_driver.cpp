/* raw_contigs_driver <bloom file> <bloom size request> <n_hash> <k> <j> <junctions file> <max read length> <fasta out> <order out>
 *
 * TEST INFRASTRUCTURE ONLY (tests/golden/make_raw_contigs_golden.py builds it against the compiled reference's objects; never shipped, never
 * linked into the product).  The file the reference's main would write as <prefix>.raw_contigs.fasta (src/Faucet.cpp:314, commented out
 * there): a map reloaded with JunctionMap::buildFromFile, JunctionMap::buildContigGraph, ContigGraph::setReadLength(max read length),
 * ContigGraph::printContigs.  The reloaded map does not iterate in the file's line order, and buildContigGraph depends on the order, so the
 * map's own iteration order is written out first, one hex k-mer per line: that is the order a test hands to fgpu_stage3_set_junctions.
 * No reference source text is copied here; this file only includes the reference headers and calls public functions. */
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "src/ContigGraph.h"
#include "utils/Bloom.h"
#include "utils/JChecker.h"
#include "utils/JunctionMap.h"
#include "utils/Kmer.h"

int main(int argc, char** argv) {
    if (argc < 10) {
        fprintf(stderr, "usage: %s <bloom> <size request> <n_hash> <k> <j> <junctions> <max read length> <fasta out> <order out>\n", argv[0]);
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
    FILE* order = fopen(argv[9], "w");
    if (!order) return 2;
    for (auto& kv : jm.junctionMap) fprintf(order, "%llx\n", (unsigned long long)kv.first);
    fclose(order);
    ContigGraph* graph = jm.buildContigGraph();
    graph->setReadLength(max_read_length);
    graph->printContigs(argv[8]);
    fflush(stdout);
    return 0;
}
