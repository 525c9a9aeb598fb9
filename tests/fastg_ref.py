"""ContigGraph::printGraph restated in plain Python, over a graph table in the Stage-3 drivers' format (tests/golden/detip_driver.cpp,
chimera_driver.cpp: "N <key> <cov x 4>", per slot that holds a contig "S <slot> <bases> <ind1> <ind2> <node1> <node2> <getAvgCoverage %.17g>",
per isolated contig "I <bases> <ind1> <ind2> <avg>") and one sequence per contig.  For tests/test_fastg_*.py and tests/test_gpu_fastg*.py.

    ContigGraph::printGraph, printContigFastG     src/ContigGraph.cpp:1470-1503   four lines per contig: getFastGHeader(true), getSeq(),
                                                                                  getFastGHeader(false), revcomp_string(getSeq())
    ContigIterator                                src/ContigIterator.cpp          which contigs, in which order
    Contig::getFastGName, getFastGHeader          src/Contig.cpp:378-385, :387-411
    Contig::getNeighbors                          src/Contig.cpp:290-302          RC: node1_p->getFastGNeighbors(ind1), else node2_p / ind2
    ContigNode::getFastGNeighbors                 src/ContigNode.cpp:179-202      index 4: the set slots 0..3 in order; else slot 4 if set;
                                                                                  primed iff getSide(this, slot) == 2
    Contig::getSide(node, index), getMinIndex     src/Contig.cpp:255-265, :178-180

The table names no contig, so a contig is what its S lines say: two S lines are one contig when they carry the same fields and stand in the two
slots those fields name ((node1, ind1) and (node2, ind2)).  Contigs are numbered in order of first appearance, S lines first, then I lines:
`seqs[c]` and `ids[c]` go by that number.  `<this>`, a heap address in the reference, is "0x%x" % ids[c].  The coverage goes through operator<<
of a double: "%g" of the table's %.17g value read back, which is that double."""
import collections

Contig = collections.namedtuple("Contig", "bases ind1 ind2 node1 node2 avg isolated")
Record = collections.namedtuple("Record", "contig primed_neighbours neighbours")      # neighbours: [(contig, primed)]

COMPLEMENT = str.maketrans("ACGT", "TGCA")


class Unset(Exception):
    """the reference goes through a pointer that is null or gone, or getSide finds neither end"""


def revcomp(s):
    return s.translate(COMPLEMENT)[::-1]


class Graph:
    """nodes: [(key, cov)] in nodeMap's order; slots: {(key, slot): contig}; contigs: [Contig]; isolated: [contig] in list order"""

    def __init__(self, table):
        self.nodes, self.slots, self.contigs, self.isolated = [], {}, [], []
        fields_at = {}
        key = None

        def end(x):
            return None if x == "-" else int(x, 16)

        for ln in table.splitlines():
            f = ln.split()
            if not f:                                        # (an empty map's table is an empty line)
                continue
            if f[0] == "N":
                key = int(f[1], 16)
                self.nodes.append((key, [int(v) for v in f[2:6]]))
            elif f[0] == "S":
                slot = int(f[1])
                t = Contig(int(f[2]), int(f[3]), int(f[4]), end(f[5]), end(f[6]), float(f[7]), False)
                here, places = (key, slot), [(t.node1, t.ind1), (t.node2, t.ind2)]
                same = [p for p in places if p != here and here in places and p in fields_at and fields_at[p] == f[2:8]]
                if same:
                    self.slots[here] = self.slots[same[0]]
                else:
                    self.slots[here] = len(self.contigs)
                    self.contigs.append(t)
                fields_at[here] = f[2:8]
            elif f[0] == "I":
                self.isolated.append(len(self.contigs))
                self.contigs.append(Contig(int(f[1]), int(f[2]), int(f[3]), None, None, float(f[4]), True))
        self.keys = {k for k, _ in self.nodes}

    def side_at(self, c, node, index):                       # Contig::getSide(node, index)
        t = self.contigs[c]
        if t.node1 == node and t.ind1 == index:
            return 1
        if t.node2 == node and t.ind2 == index:
            return 2
        raise Unset("getSide(%x, %d) finds neither end" % (node, index))

    def fastg_neighbours(self, node, index):                 # ContigNode::getFastGNeighbors
        if node not in self.keys:
            raise Unset("a node that is gone: %x" % node)
        out = []
        for i in (range(4) if index == 4 else (4,)):
            c = self.slots.get((node, i))
            if c is not None:
                out.append((c, self.side_at(c, node, i) == 2))
        return out

    def neighbours(self, c, rc):                             # Contig::getNeighbors
        t = self.contigs[c]
        node, index = (t.node1, t.ind1) if rc else (t.node2, t.ind2)
        return [] if node is None else self.fastg_neighbours(node, index)

    def walk(self):                                          # ContigIterator
        for key, _ in self.nodes:
            for index in range(5):
                c = self.slots.get((key, index))
                if c is None:
                    continue
                t = self.contigs[c]
                if t.node1 is None or t.node2 is None:
                    yield c
                elif t.node1 == t.node2:
                    if index == min(t.ind1, t.ind2):
                        yield c
                elif self.side_at(c, key, index) == 1:
                    yield c


def name(t, ident, rc):                                      # Contig::getFastGName
    return "NODE_0x%x_length_%d_cov_%s" % (ident, t.bases, "%g" % t.avg) + ("'" if rc else "")


def records(graph, read_length):
    """([Record] in file order, info as fgpu_fastg_info)"""
    out = [Record(c, graph.neighbours(c, True), graph.neighbours(c, False)) for c in graph.walk()]
    info = dict(node_records=len(out), isolated_printed=0, isolated_listed=len(graph.isolated), nodes=len(graph.nodes))
    for c in graph.isolated:
        if graph.contigs[c].bases >= read_length % (1 << 64):                # (size_t >= int: the int goes to unsigned)
            out.append(Record(c, graph.neighbours(c, True), graph.neighbours(c, False)))
            info["isolated_printed"] += 1
    return out, info


def header(graph, ids, c, rc, neighbours):                   # Contig::getFastGHeader
    s = ">" + name(graph.contigs[c], ids[c], rc)
    if not neighbours:
        return s + ";"
    return s + ":" + ",".join(name(graph.contigs[n], ids[n], p) for n, p in neighbours) + ";"


def render(graph, recs, seqs, ids):
    lines = []
    for r in recs:
        assert len(seqs[r.contig]) == graph.contigs[r.contig].bases, (r.contig, len(seqs[r.contig]), graph.contigs[r.contig].bases)
        lines += [header(graph, ids, r.contig, True, r.primed_neighbours), seqs[r.contig], header(graph, ids, r.contig, False, r.neighbours), revcomp(seqs[r.contig])]
    return "".join(ln + "\n" for ln in lines).encode()


def print_graph(table, seqs, ids, read_length):
    """(the file's bytes, info, the graph, the records) of a graph table"""
    graph = Graph(table)
    recs, info = records(graph, read_length)
    return render(graph, recs, seqs, ids), info, graph, recs


def stdout_lines(info):                                      # what printGraph says (src/ContigGraph.cpp:1471, :1483, :1492, :1495)
    return ["Printing unitig FASTG.", "printed %d node-connected unitigs" % info["node_records"], "printed %d isolated contigs" % info["isolated_listed"],
            "Done printing graph."]


def halves(text):
    """the order- and orientation-free form of a FASTG file: the multiset of (own (length, cov text), tuple of the neighbours' (length, cov text),
    sequence) over every header/sequence pair"""
    def lc(nm):
        f = nm.rstrip("'").split("_")
        return f[3], f[5]
    out = collections.Counter()
    lines = text.decode().splitlines()
    for hdr, seq in zip(lines[::2], lines[1::2]):
        assert hdr[0] == ">" and hdr[-1] == ";", hdr
        own, _, rest = hdr[1:-1].partition(":")
        out[(lc(own), tuple(lc(n) for n in rest.split(",")) if rest else (), seq)] += 1
    return out
