// join_driver.cpp — golden generator only (tests/golden/make_join_golden.py): the compiled reference's ContigJuncList over piece lists.
// Reads from stdin: k, the number of lists, and per list its pieces (flip, sequence, distances, coverages); per piece with flip != 0 it calls
// ContigJuncList::reverse, then ContigJuncList::concatenate left to right as Contig::concatenate does, and prints per list the sequence,
// the two lists and getAvgCoverage() with 17 significant digits.  Public members of the reference only.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "utils/ContigJuncList.h"
#include "utils/Kmer.h"

static ContigJuncList read_piece(int* flip) {
    std::string seq;
    size_t nd, nc;
    std::cin >> *flip >> seq >> nd;
    ContigJuncList::junc_list dist(nd);
    for (size_t i = 0; i < nd; i++) { int v; std::cin >> v; dist[i] = (unsigned char)v; }
    std::cin >> nc;
    ContigJuncList::junc_list cov(nc);
    for (size_t i = 0; i < nc; i++) { int v; std::cin >> v; cov[i] = (unsigned char)v; }
    return ContigJuncList(seq, dist, cov);
}

int main() {
    int k;
    size_t n;
    std::cin >> k >> n;
    setSizeKmer(k);
    for (size_t i = 0; i < n; i++) {
        size_t m;
        std::cin >> m;
        ContigJuncList acc;
        for (size_t p = 0; p < m; p++) {
            int flip;
            ContigJuncList piece = read_piece(&flip);
            if (flip) piece.reverse();
            acc = p ? acc.concatenate(piece) : piece;
        }
        printf("%s\n", acc.getSeq().c_str());
        for (ContigJuncList::const_iterator it = acc.begin_distances(); it != acc.end_distances(); ++it) printf("%d ", (int)*it);
        printf("\n");
        for (ContigJuncList::const_iterator it = acc.begin_coverages(); it != acc.end_coverages(); ++it) printf("%d ", (int)*it);
        printf("\n%.17g\n", acc.getAvgCoverage());
    }
    return std::cin.fail() ? 1 : 0;
}
