"""What the FASTG tests share (tests/test_fastg_plan_cpu.py, test_fastg_reference_cpu.py, test_gpu_fastg.py, test_gpu_fastg_cli.py): the stand-alone
check program (tests/host/fastg_plan_check.cpp) built and run, the graph table of a build BEFORE any step in the drivers' format (from the graph
tests/raw_contigs_ref.graph_of holds, which tests/detip_plan_ref.py starts from), and the expected file of a table: tests/fastg_ref.py over the
reference's table, with the sequences tests/detip_ref.join makes of the host plan's piece lists and the plan's contig numbers as <this>."""
import os
import struct
import subprocess

import numpy as np

from tests import dechimera_golden as G
from tests import detip_golden as D
from tests import detip_ref as J
from tests import fastg_ref as F
from tests import raw_contigs_ref as P

ROOT = D.ROOT
SOURCE = os.path.join(ROOT, "tests", "host", "fastg_plan_check.cpp")
STEPS = ("raw", "detip", "dechimera")


def compile_check(exe):
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", SOURCE, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, timeout=300, env=dict(os.environ, **G.SANITIZER_ENV))
    err = r.stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err and r.returncode == 0, (r.returncode, err[-3000:])
    return r.stdout


def run_fmt(exe):
    """(pairs checked, mismatches, the program's lines)"""
    lines = _run([exe, "fmt"]).decode().splitlines()
    f = lines[-1].split()
    assert f[0] == "checked" and f[2] == "mismatches", lines[-1]
    return int(f[1]), int(f[3]), lines


class Plan:
    """what `fastg_plan_check plan` printed: status; info (fgpu_fastg_info as a dict); contigs [(tig, bases, sum, n, pieces)] as the graph numbers
    them; records [(tig, primed header's neighbours, other header's)], a neighbour = (record, primed); text: the file rendered on the host"""

    def __init__(self, out):
        head, sep, self.text = out.partition(b"TEXT ")
        lines = head.decode().splitlines()
        self.status = int(lines[0].split()[1])
        self.info, self.contigs, self.records = None, [], []
        if self.status != 0:
            assert not sep and len(lines) == 1, lines
            return
        self.info = dict(zip(("node_records", "isolated_printed", "isolated_listed", "nodes"), (int(v) for v in lines[1].split()[1:])))
        for ln in lines[2:]:
            left, _, tail = ln.partition(":")
            f = left.split()
            if f[0] == "C":
                v = [int(x) for x in tail.split()]
                self.contigs.append((int(f[1]), int(f[2]), int(f[3]), int(f[4]), list(zip(v[::2], (bool(x) for x in v[1::2])))))
            else:
                assert f[0] == "R", ln
                v = [int(x) for x in f[2:]]
                n0 = v[0]
                first = [(v[1 + 2 * i], bool(v[2 + 2 * i])) for i in range(n0)]
                rest = v[1 + 2 * n0:]
                second = [(rest[1 + 2 * i], bool(rest[2 + 2 * i])) for i in range(rest[0])]
                assert len(rest) == 1 + 2 * rest[0], ln
                self.records.append((int(f[1]), first, second))
        size, _, self.text = self.text.partition(b"\n")
        assert int(size) == len(self.text)


def run_plan(exe, path, keys, recs, calls, k, read_length, step, change=()):
    """the program over a tests/graph_build_ref.py build (`calls`) of the map (keys, recs)"""
    contigs, cl, _ = P.arrays_of(calls)
    with open(path, "wb") as f:
        f.write(struct.pack("<QQiiQ", len(keys), len(contigs), k, read_length, G.NO_LIMIT))
        for a in (np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(recs), contigs, cl, G.summaries_of(calls)):
            f.write(a.tobytes())
        for w in calls:
            s = w.contig.string.encode()
            f.write(struct.pack("<I", len(s)) + s)
    return Plan(_run([exe, "plan", path, step, *[str(x) for x in change]]))


def raw_table(calls, keys, cov, k):
    """the graph JunctionMap::buildContigGraph returns, as the drivers would write it (no first and no counts line: tests/fastg_ref.py reads neither)"""
    nodes, ends, isolated = P.graph_of(calls, keys, cov, k)
    triples = D.triples_of(calls)

    def end(x):
        return "-" if x is None else "%x" % x

    def avg(c):
        v = calls[c].contig.coverages
        return "%.17g" % (float(sum(v)) / float(len(v)))

    out = []
    for key, nd in nodes:
        out.append("N %x %d %d %d %d" % (key, *nd.cov))
        for i, c in enumerate(nd.contigs):
            if c is not None:
                t = calls[c].contig
                out.append("S %d %d %d %d %s %s %s" % (i, len(t.string), t.ind1, t.ind2, end(ends[c].node1), end(ends[c].node2), avg(c)))
    for b, f in isolated:                                                      # backward->concatenate(forward, 1, 1)
        j = J.join(triples, [[(b, True), (f, False)]], k)[0]
        out.append("I %d %d %d %s" % (len(j[0]), calls[b].contig.ind2, calls[f].contig.ind2, "%.17g" % j[3]))
    return "".join(ln + "\n" for ln in out)


def names_of(text):
    """(length, coverage text) of every record of a FASTG file, as a multiset: its unprimed headers' own names"""
    import collections
    out = collections.Counter()
    for hdr in text.decode().splitlines()[2::4]:
        f = hdr[1:].split(":")[0].rstrip(";").split("_")
        out[(f[3], f[5])] += 1
    return out


def golden_reads():
    """the goldens that have reads"""
    from tests.golden_util import GOLDEN
    return sorted(n for n in os.listdir(GOLDEN) if os.path.exists(os.path.join(GOLDEN, n, "case.json")) and
                  any(os.path.exists(os.path.join(GOLDEN, n, r)) for r in ("reads.fa.gz", "reads.fq.gz")))


def reference_final_graph(name, d):
    """`faucet_ref` run from a golden's reads WITH cleaning, in directory d: (why not | None, reads path, arguments, its .cleaned_graph_unitigs.fastg,
    the Map of its .bloom / .junctions, chimera_driver's table on them).  why not: "not run" -- the reference did not finish --, or "changed" -- a later
    step changed the graph: the multiset of (length, %g coverage) of the final file's records is not that of the table's contigs, the isolated ones
    below the read length left out as printGraph leaves them out.  Decided from reference data only."""
    import collections

    from tests import stage3_fuzz_cases as S
    from tests.golden_util import Case
    c = Case(name)
    os.makedirs(str(d), exist_ok=True)
    reads = os.path.join(str(d), "reads.fq" if c.fastq else "reads.fa")
    with open(reads, "wb") as f:
        f.write(c.reads_text())
    args = [a for a in c.meta["args"] if a != "--no_cleaning"]
    ref = os.path.join(str(d), "ref")
    final = os.path.join(ref, "out.cleaned_graph_unitigs.fastg")
    try:
        r = S.reference_run(reads, args, ref)
    except S.NotReturned:
        return "not run", reads, args, None, None, None
    if r.returncode != 0 or not os.path.exists(final):
        return "not run", reads, args, None, None, None
    m = S.map_from(ref, r.stdout, args)
    try:
        table = S.chimera_answers_of(m)[1]
    except S.NotReturned:
        return "changed", reads, args, None, m, None
    with open(final, "rb") as f:
        text = f.read()
    printed = [t for t in F.Graph(table).contigs if not t.isolated or t.bases >= m.max_read_length]
    same = names_of(text) == collections.Counter((str(t.bases), "%g" % t.avg) for t in printed)
    return None if same else "changed", reads, args, text, m, table


def expected(table, plan_contigs, calls, k, read_length):
    """tests/fastg_ref.print_graph of a reference table: (bytes, info, graph, records); contig c of the table is plan_contigs[c] = (tig, bases, sum, n,
    pieces) -- its letters are the pieces joined, <this> its tig; lengths and averages have to be the table's"""
    joined = J.join(D.triples_of(calls), [t[4] for t in plan_contigs], k) if plan_contigs else []
    graph = F.Graph(table)
    assert [(t.bases, "%.17g" % t.avg) for t in graph.contigs] == [(len(j[0]), "%.17g" % j[3]) for j in joined], "the plan's contigs are not the table's"
    assert [(t[1], t[2], t[3]) for t in plan_contigs] == [(len(j[0]), sum(j[2]), len(j[2])) for j in joined]
    recs, info = F.records(graph, read_length)
    return F.render(graph, recs, [j[0] for j in joined], [t[0] for t in plan_contigs]), info, graph, recs
