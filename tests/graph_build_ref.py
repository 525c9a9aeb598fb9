"""JunctionMap::buildContigGraph (utils/JunctionMap.cpp:11-129) restated in plain Python over a callable find_neighbor(alive, kmer, index), for
tests/test_graph_build_ref_cpu.py and tests/test_gpu_stage3_build.py: the getContig calls the reference makes, in its order, each on the map as
it stands at that moment.

`alive` is a list of booleans over the map's junctions in map order (the order of the keys: the reference's iteration order); a junction the
reference has erased (killJunction, :210-216 and :90-102) is False from then on, and find_neighbor answers as findNeighbor does on a map
without it.  The chain of one call is tests/contig_ref.py's get_contig.  Every call the reference COULD make has a time t: the branching
starts in map order, one slot for destroyComplexJunctions, two per junction with one path out.

Build.calls: one Call per getContig call that is made (t, phase, start, the Contig, Contig::getSideKmer(2) and what :56 / :58 say of it);
skipped_claim: (t, row, index) of the starts that had a contig already (:50); skipped_dead: the times of the starts that were gone when the
iterator came by;
status 0: the build ran to its end, 1 / 3: the call at stop_t (call number len(calls)) trips an assert / never returns.
"""
import collections

from tests import contig_ref as R

BRANCHING, LINEAR_FORWARD, LINEAR_BACKWARD = range(3)
Call = collections.namedtuple("Call", "t phase start contig far_kmer far_is_junction far_is_start")
Build = collections.namedtuple("Build", "calls status stop_t skipped_claim skipped_dead killed_by n_times")


def kmer_of(s):
    """getKmerFromRead (utils/Kmer.cpp:435-441)"""
    x = 0
    for ch in s:
        x = (x << 2) | R.NT.index(ch)
    return x


def side_kmer_2(string, ind2, k):
    """Contig::getSideKmer(2) (src/Contig.cpp:235-239): the last k-mer of the string, reverse-complemented unless ind2 is 4"""
    x = kmer_of(string[len(string) - k:])
    return x if ind2 == 4 else R.revcomp(x, k)


def build_contig_graph(find_neighbor, keys, cov, k):
    keys = [int(x) for x in keys]
    cov = [[int(v) for v in c] for c in cov]
    row_of = {x: r for r, x in enumerate(keys)}
    cov_of = dict(zip(keys, cov))
    alive = [True] * len(keys)
    claimed = set()                                                    # (row, i): ContigNode::contigs[i] is set
    calls, skipped_claim, skipped_dead, killed_by = [], [], [], {}
    t = 0

    def get_contig(start, index, own_cov):
        c = R.get_contig(lambda km, ix: find_neighbor(alive, km, ix), cov_of, k, start, index)
        if c.status == 0:
            c = c._replace(coverages=[R.coverage(own_cov, index)] + c.coverages[1:])      # :148 reads the caller's copy of the junction
            for x in c.kills:                                                              # :210-216
                if x != start and alive[row_of[x]]:
                    alive[row_of[x]] = False
                    killed_by[row_of[x]] = t
        return c

    def stopped(status):
        return Build(calls, status, t, skipped_claim, skipped_dead, killed_by, None)

    # ---- buildBranchingPaths, :34-82
    for r, (kmer, c0) in enumerate(zip(keys, cov)):
        if R.paths_out(c0) <= 1:                                                           # :40
            continue
        own = list(c0)
        s = R.print_kmer(kmer, k)
        if len(set(s)) == 1:                                                               # :43-47
            own[R.NT.index(s[0])] = 0
        for i in range(5):
            if not (own[i] if i < 4 else sum(own)) > 0:                                    # :50, getCoverage is an int
                continue
            if (r, i) in claimed:
                skipped_claim.append((t, r, i))
                t += 1
                continue
            c = get_contig(kmer, i, own)                                                   # :52
            if c.status:
                return stopped(c.status)
            far = side_kmer_2(c.string, c.ind2, k)                                         # :54
            is_j = far in row_of and alive[row_of[far]]                                    # :56
            claimed.add((r, c.ind1))                                                       # setEnds, src/Contig.cpp:127-129
            if is_j:
                claimed.add((row_of[far], c.ind2))                                         # :60 (the start node itself) or :65-67; src/Contig.cpp:130-132
            calls.append(Call(t, BRANCHING, kmer, c, far, int(is_j), int(is_j and far == kmer)))
            t += 1
    # ---- destroyComplexJunctions, :90-102
    for r, c0 in enumerate(cov):
        if R.paths_out(c0) > 1:
            alive[r] = False
    t += 1
    # ---- buildLinearRegions, :104-129
    for r, (kmer, c0) in enumerate(zip(keys, cov)):
        if R.paths_out(c0) != 1:                                                           # (complex ones are gone; :126 only prints)
            continue
        if not alive[r]:
            skipped_dead += [t, t + 1]
            t += 2
            continue
        forward = [i for i in range(4) if c0[i] > 0][-1]                                  # :111-115
        for phase, i in ((LINEAR_FORWARD, forward), (LINEAR_BACKWARD, 4)):                 # :114, :118
            c = get_contig(kmer, i, c0)
            if c.status:
                return stopped(c.status)
            far = side_kmer_2(c.string, c.ind2, k)
            is_j = far in row_of and alive[row_of[far]]
            calls.append(Call(t, phase, kmer, c, far, int(is_j), int(is_j and far == kmer)))
            t += 1
    return Build(calls, 0, t, skipped_claim, skipped_dead, killed_by, t)
