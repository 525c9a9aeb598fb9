"""JunctionMap::getContig (utils/JunctionMap.cpp:133-221) restated in plain Python over a callable find_neighbor(kmer, index), for
tests/test_contig_ref_cpu.py and tests/test_gpu_stage3_contigs.py.

Within one getContig call the map is static (the kills happen behind the loop, :210-216), so a chain is a pure function of (map, filter,
start): the loop below asks `find_neighbor` for one segment after the other exactly as :157-197 does and keeps what :199-208 hands to the
Contig.  `find_neighbor(kmer, index)` returns one recorded answer of the reference's own findNeighbor (a line of
tests/golden/stage3_neighbors_*.jsonl.gz: kmer, node, rindex, dist, len, contig -- or abort) and raises NotRecorded where the fixture
has none.

status (fgpu_contig.status, include/faucet_gpu.h): 0 the reference returns; 1 a call of the chain trips one of the reference's asserts;
2 the start is not in the map or the index is not 0..4; 3 the chain runs into a cycle that does not hold the start k-mer, where the
reference's while(!done) never returns.  A chain state is (junction, entered forward or backward), at most two per junction, and the
start state: a chain that has made more than 2 * junctions + 1 hops has been in one state twice.
"""
import collections

NT = "ACTG"                                    # the reference's code (utils/Kmer.cpp): A 0, C 1, T 2, G 3; the complement is code ^ 2

Contig = collections.namedtuple("Contig", "status ind1 ind2 end_kmer end_node string distances coverages kills")


class NotRecorded(LookupError):
    """the fixture holds no answer for this (k-mer, index)"""


def print_kmer(x, k):
    return "".join(NT[(x >> (2 * i)) & 3] for i in range(k - 1, -1, -1))


def revcomp(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | ((x & 3) ^ 2)
        x >>= 2
    return r


def revcomp_string(s):
    return "".join(NT[NT.index(c) ^ 2] for c in reversed(s))


def coverage(cov, index):
    """Junction::getCoverage (utils/Junction.cpp:48-53), as the unsigned char getContig stores (:148, :169)"""
    return (int(cov[index]) if index < 4 else sum(int(c) for c in cov)) & 0xFF


def paths_out(cov):
    """Junction::numPathsOut (utils/Junction.cpp:24-32)"""
    return sum(1 for c in cov if c > 0)


def opposite_index(cov, index):
    """Junction::getOppositeIndex (utils/Junction.cpp:11-22): 4 after a forward entry -- whatever that extension's coverage is --, the first
    covered extension after a backward one"""
    if index < 4:
        return 4
    return next(i for i in range(4) if cov[i] > 0)


def failed(status):
    return Contig(status, 0, 0, 0, 0, "", [], [], [])


def get_contig(find_neighbor, cov_of, k, start, start_index):
    """getContig(junctionMap[start], start, start_index); cov_of: {k-mer: the four coverages} of the map"""
    if start not in cov_of or not 0 <= start_index <= 4:
        return failed(2)
    kmer, index = start, start_index
    coverages = [coverage(cov_of[start], start_index)]                                   # :148
    string = print_kmer(revcomp(start, k) if index == 4 else start, k)                  # :149-151
    distances, kills = [], []
    hops = 0
    while True:                                                                          # :157
        if hops > 2 * len(cov_of) + 1:
            return failed(3)
        hops += 1
        r = find_neighbor(kmer, index)                                                   # :158
        if r.get("abort"):
            return failed(1)
        if r["len"] > k:                                                                 # :160-162
            string += r["contig"][k:]
        distances.append(r["dist"] & 0xFF)                                               # :163
        end = int(r["kmer"], 16)
        if not r["node"]:                                                                # :193-196
            break
        nxt = cov_of[end]                                                                # :167
        coverages.append(coverage(nxt, r["rindex"]))                                     # :169
        if paths_out(nxt) != 1:                                                          # :188-191
            break
        kmer, index = end, opposite_index(nxt, r["rindex"])                              # :172-174
        if end == start:                                                                 # :177-180
            break
        kills.append(end)                                                                # :185
    return Contig(0, start_index, r["rindex"] if r["node"] else 4, end, int(bool(r["node"])), string, distances, coverages, kills)   # :199-208


def recorded(calls):
    """find_neighbor over a fixture's recorded calls"""
    table = {(int(e["start"], 16), e["index"]): e for e in calls}

    def find_neighbor(kmer, index):
        try:
            return table[(kmer, index)]
        except KeyError:
            raise NotRecorded((kmer, index)) from None
    return find_neighbor


def branching_starts_ref(keys, cov, k):
    """the getContig calls of buildBranchingPaths (utils/JunctionMap.cpp:36-50) on a map that does not change: (k-mer, index) in map order"""
    out = []
    for key, c in zip(keys, cov):
        c = [int(v) for v in c]
        if paths_out(c) > 1:
            s = print_kmer(int(key), k)
            if len(set(s)) == 1:                                                         # isHomoPolymer: setCoverage(firstBase, 0), :43-47
                c[NT.index(s[0])] = 0
            out += [(int(key), i) for i in range(5) if (c[i] if i < 4 else sum(c)) > 0]        # getCoverage is an int here
    return out


def linear_starts_ref(keys, cov):
    """the getContig calls of buildLinearRegions (:105-118): the covered extension(s), then 4, of every junction with one path out"""
    out = []
    for key, c in zip(keys, cov):
        if paths_out(c) == 1:
            out += [(int(key), i) for i in range(4) if c[i] > 0] + [(int(key), 4)]
    return out
