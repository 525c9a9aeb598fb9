"""ContigGraph::printContigs (src/ContigGraph.cpp:1532-1645) on the graph JunctionMap::buildContigGraph returns, restated in plain Python over
the calls tests/graph_build_ref.py produces, for tests/test_raw_contigs_ref_cpu.py and the GPU tests of the raw contigs: the file the
reference names <prefix>.raw_contigs.fasta.

The graph: nodeMap takes ContigGraph::createContigNode's inserts (src/ContigGraph.cpp:1656) in the reference's order -- the start of every
complex junction the branching loop visits (utils/JunctionMap.cpp:42) and the far junction of a call whose far_is_junction holds and whose
far_is_start does not (:66); inserting a key that is there changes nothing -- and is gone over in the iteration order of libstdc++'s
std::unordered_map, replayed by tests/dump_order_ref.py (pinned to a real container by tests/test_dump_order_ref_cpu.py).  A node copies its
junction's four coverages (the homopolymer rule :43-47 zeroes one of a node visited as a start); Contig::setEnds (src/Contig.cpp:123-133)
stores the contig in contigs[ind1] of the start node and contigs[ind2] of the far node.  Every linear region is
backward->concatenate(forward, 1, 1) (:120), pushed onto isolated_contigs in call order.

The print: printAndMarkBubbleContigs (:1543-1580, isBubbleNode :490-503, getNewConcatenatedContig :1509-1530), then printUnmarkedUnitigs
(:1605-1645); every record ">Contig<n>\\n<canon_contig(seq)>\\n" (utils/Kmer.cpp:345-351: the comparison is one of strings of LETTERS).

plan(...) -> (records, info); a record is (number, kind, pieces), pieces = one or two (call number, flip); strings_of / fasta_of turn
them into sequences.  UnsetContig: the reference would read a contig pointer nobody set."""
import collections

from tests import contig_ref as R
from tests import dump_order_ref as D
from tests import graph_build_ref as G

BUBBLE, NODE, ISOLATED = "bubble", "node", "isolated"
Record = collections.namedtuple("Record", "number kind pieces")


class UnsetContig(Exception):
    pass


class NotABuild(Exception):
    """the calls are not a finished build: a linear forward call without its backward one (a build that stopped between the two)"""


class _Node:
    def __init__(self, cov):
        self.cov = [int(v) for v in cov[:4]]
        self.contigs = [None] * 5


class _Ends:
    def __init__(self):
        self.node1 = self.node2 = None
        self.mark = False

    def side(self, node):                                                  # Contig::getSide, src/Contig.cpp:243-253
        return 1 if self.node1 == node else 2 if self.node2 == node else -1

    def other(self, node):                                                 # Contig::otherEndNode, :182-193
        return self.node2 if self.node1 == node else self.node1 if self.node2 == node else None


def graph_of(calls, keys, cov, k):
    """(nodes in the container's iteration order as [(kmer, _Node)], ends per call, isolated as [(backward call, forward call)])"""
    keys = [int(x) for x in keys]
    row_of = {x: r for r, x in enumerate(keys)}
    nodes, inserted = {}, []
    ends = [_Ends() for _ in calls]

    def create(kmer):
        if kmer not in nodes:
            nodes[kmer] = _Node(cov[row_of[kmer]])
            inserted.append(kmer)
        return nodes[kmer]

    of_start = collections.defaultdict(list)
    for c, w in enumerate(calls):
        if w.phase == G.BRANCHING:
            of_start[w.start].append(c)
    for r, kmer in enumerate(keys):                                        # buildBranchingPaths
        if R.paths_out([int(v) for v in cov[r]]) <= 1:
            continue
        start = create(kmer)
        s = R.print_kmer(kmer, k)
        if len(set(s)) == 1:
            start.cov[R.NT.index(s[0])] = 0
        for c in of_start.get(kmer, ()):
            w, e = calls[c], ends[c]
            e.node1 = kmer
            if w.far_is_junction and w.far_is_start:
                e.node2 = kmer
                start.contigs[w.contig.ind1] = c
                start.contigs[w.contig.ind2] = c
            elif w.far_is_junction:
                other = create(w.far_kmer)
                e.node2 = w.far_kmer
                start.contigs[w.contig.ind1] = c
                other.contigs[w.contig.ind2] = c
            else:
                start.contigs[w.contig.ind1] = c
    linear = [c for c, w in enumerate(calls) if w.phase != G.BRANCHING]
    if len(linear) % 2 or not all(calls[f].phase == G.LINEAR_FORWARD and calls[b].phase == G.LINEAR_BACKWARD and calls[f].start == calls[b].start
                                  for f, b in zip(linear[::2], linear[1::2])):
        raise NotABuild()
    isolated = [(b, f) for f, b in zip(linear[::2], linear[1::2])]
    order = D.replay(inserted, *D.libstdcxx_schedule(len(inserted))) if inserted else []
    return [(inserted[i], nodes[inserted[i]]) for i in order], ends, isolated


def plan(calls, keys, cov, k, read_length):
    nodes, ends, isolated = graph_of(calls, keys, cov, k)
    length = [len(w.contig.string) for w in calls]
    records = []
    count = collections.Counter()

    def put(kind, pieces):
        records.append(Record(len(records) + 1, kind, pieces))
        count[kind] += 1

    for kmer, nd in nodes:                                                 # printAndMarkBubbleContigs
        out = [i for i in range(4) if nd.cov[i] > 0]
        if len(out) != 2:
            continue
        if any(nd.contigs[i] is None for i in out):
            raise UnsetContig("isBubbleNode reads contigs[%s] of node %x" % ([i for i in out if nd.contigs[i] is None], kmer))
        far = [ends[nd.contigs[i]].other(kmer) for i in out]
        if far[0] != far[1] or far[0] is None:                             # allSame, :153-162: two null nodes are not the same
            continue
        back = nd.contigs[4]
        if back is None:
            raise UnsetContig("printAndMarkBubbleContigs reads contigs[4] of node %x" % kmer)
        if not length[back] < 250:
            continue
        back_mark = False
        for i in range(4):
            c = nd.contigs[i]
            if c is None or ends[c].mark:
                continue
            if not ends[back].mark:
                put(BUBBLE, ((back, ends[back].side(kmer) == 1), (c, ends[c].side(kmer) == 2)))
                back_mark = True
                ends[c].mark = True
        if back_mark:
            ends[back].mark = True
    for kmer, nd in nodes:                                                 # printUnmarkedUnitigs
        for i in range(5):
            c = nd.contigs[i]
            if c is None or ends[c].mark:
                continue
            put(NODE, ((c, False),))
            ends[c].mark = True
    dropped = 0
    for b, f in isolated:
        if length[b] - k + length[f] >= read_length:
            put(ISOLATED, ((b, True), (f, False)))
        else:
            dropped += 1
    info = dict(records=len(records), bubble_records=count[BUBBLE], node_contigs=count[NODE], isolated_kept=count[ISOLATED], isolated_dropped=dropped,
                nodes=len(nodes))
    return records, info


def join(strings, flips, k):
    """ContigJuncList::concatenate's sequence (utils/ContigJuncList.cpp:121) of the oriented pieces"""
    s = [R.revcomp_string(x) if f else x for x, f in zip(strings, flips)]
    return s[0] if len(s) == 1 else s[0][:len(s[0]) - k] + s[1]


def canon_contig(s):
    rc = R.revcomp_string(s)
    return s if s <= rc else rc


def strings_of(records, calls, k):
    return [join([calls[c].contig.string for c, _ in r.pieces], [f for _, f in r.pieces], k) for r in records]


def fasta_of(numbers, strings):
    return "".join(">Contig%d\n%s\n" % (n, canon_contig(s)) for n, s in zip(numbers, strings)).encode()


def raw_contigs(calls, keys, cov, k, read_length):
    """(the file's bytes, info, records)"""
    records, info = plan(calls, keys, cov, k, read_length)
    return fasta_of([r.number for r in records], strings_of(records, calls, k)), info, records


def pack_text(strings):
    """(2-bit words in the library's layout -- A 0, C 1, T 2, G 3, 32 bases per word, first base lowest, every string from a word of its own --,
    first word of each string)"""
    import numpy as np
    words, first = [], []
    for s in strings:
        first.append(len(words))
        for at in range(0, len(s), 32):
            words.append(sum(R.NT.index(ch) << (2 * i) for i, ch in enumerate(s[at:at + 32])))
    return np.array(words, dtype=np.uint64), first


def arrays_of(calls):
    """the calls as fgpu_stage3_build_take hands them over: (fgpu_contig array, fgpu_build_call array, text words); the segment and coverage
    fields stay 0 -- the plan does not read them"""
    import numpy as np
    from faucet_amd import api
    text, first = pack_text([w.contig.string for w in calls])
    contigs, recs = np.zeros(len(calls), dtype=api.CONTIG_DTYPE), np.zeros(len(calls), dtype=api.BUILD_DTYPE)
    for i, w in enumerate(calls):
        c = w.contig
        contigs[i]["end_kmer"], contigs[i]["text_word"], contigs[i]["len"] = c.end_kmer, first[i], len(c.string)
        contigs[i]["ind1"], contigs[i]["ind2"], contigs[i]["end_node"] = c.ind1, c.ind2, c.end_node
        recs[i]["start_kmer"], recs[i]["far_kmer"], recs[i]["time"], recs[i]["phase"] = w.start, w.far_kmer, w.t, w.phase
        recs[i]["far_is_junction"], recs[i]["far_is_start"] = w.far_is_junction, w.far_is_start
    return contigs, recs, text


def plan_lines(records, contigs):
    """the records as tests/host/raw_plan_check.cpp prints fgpu_raw_plan's"""
    return ["%d %d" % (r.number, len(r.pieces)) + "".join(" %d %d %d" % (int(contigs[c]["text_word"]), int(contigs[c]["len"]), int(f)) for c, f in r.pieces)
            for r in records]
