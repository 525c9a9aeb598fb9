"""The goldens of ContigGraph::deleteTipsAndClean (tests/golden/detip_<name>.fasta.gz and .graph.gz, made by tests/golden/make_detip_golden.py
from the compiled reference) and what a plan (fgpu_tips_plan's outputs: nodes, contig records, piece lists, print records) comes to in their
terms, for tests/test_detip_plan_cpu.py, tests/test_gpu_detip.py and the script itself.

The graph table (tests/golden/detip_driver.cpp writes it): "return <0|1>", then per node in nodeMap's order "N <key> <cov x 4>" and per slot that
holds a contig "S <slot> <bases> <ind1> <ind2> <node1> <node2> <getAvgCoverage %.17g>", then per isolated contig "I <bases> <ind1> <ind2> <avg>",
then "counts <tips> <nodes left> <nodes validateNoneCollapsible removed, or -1 where it did not run>" as the reference printed them."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np

from tests import detip_ref as J
from tests import raw_contigs_ref as P
from tests.golden_util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY = os.path.join(GOLDEN, "detip_summary.json")
INFO_KEYS = ("nodes_before", "tips", "back_tips", "collapsed_0", "collapsed_1", "degenerate_0", "degenerate_1", "validated", "changed", "records",
             "bubble_records", "node_contigs", "isolated_kept", "isolated_dropped", "nodes")
SOURCES = [os.path.join(ROOT, "tests", "host", "tips_plan_check.cpp"), os.path.join(ROOT, "faucet_amd", "csrc", "tips_plan.cpp")]
NO_LIMIT = (1 << 64) - 1


def summary():
    if not os.path.exists(SUMMARY):                  # (only while tests/golden/make_detip_golden.py is making it)
        return {"fixtures": {}, "not_returned": {}, "reached": {}}
    with open(SUMMARY) as f:
        return json.load(f)


def golden(name, kind):
    with gzip.open(os.path.join(GOLDEN, f"detip_{name}.{kind}.gz"), "rb") as f:
        return f.read()


def compile_check(exe, sanitize):
    flags = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined"] if sanitize else []
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", *flags, *SOURCES, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


class Plan:
    """what tips_plan_check printed: sizing, status, sizes, info (a dict over INFO_KEYS), nodes [(key, cov, slots)], contigs [(node1, node2, bases,
    ind1, ind2, isolated, pieces)] (a node: its key, or None), records [(number, pieces)]; pieces = [(call, flip)]"""

    def __init__(self, text):
        lines = text.splitlines()
        self.sizing, self.status = int(lines[0].split()[1]), int(lines[1].split()[1])
        self.sizes = [int(v) for v in lines[2].split()[1:]]
        self.info = dict(zip(INFO_KEYS, (int(v) for v in lines[3].split()[1:])))
        self.nodes, self.contigs, self.records = [], [], []

        def pieces(s):
            v = [int(x) for x in s.split()]
            return list(zip(v[::2], (bool(x) for x in v[1::2])))

        for ln in lines[4:]:
            head, _, tail = ln.partition(":")
            f = head.split()
            if f[0] == "N":
                self.nodes.append((int(f[1], 16), [int(v) for v in f[2:6]], [int(v) for v in f[6:11]]))
            elif f[0] == "C":
                assert int(f[1]) == len(self.contigs)
                self.contigs.append((None if f[2] == "-" else int(f[2], 16), None if f[3] == "-" else int(f[3], 16), int(f[4]), int(f[5]), int(f[6]),
                                     int(f[7]), pieces(tail)))
            else:
                self.records.append((int(f[1]), pieces(tail)))


def run_check(exe, path, keys, recs, contigs, calls, k, read_length, cap=NO_LIMIT, sanitized=True):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQiiQ", len(keys), len(contigs), k, read_length, cap))
        for a in (np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(recs), contigs, calls):
            f.write(a.tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1"))
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return Plan(r.stdout)


def triples_of(calls):
    """the calls of a tests/graph_build_ref.py build as tests/detip_ref.py's contigs"""
    return [(w.contig.string, list(w.contig.distances), list(w.contig.coverages)) for w in calls]


def fasta_of(records, joined):
    """the file of print records [(number, pieces)] whose lists join to `joined` (tests/detip_ref.join's results)"""
    return P.fasta_of([n for n, _ in records], [j[0] for j in joined])


def table_of(nodes, contigs, joined, changed):
    """the graph table without its counts line, from a plan's nodes and contig records and what the records' lists join to: `joined[c]` =
    (bases, getAvgCoverage) of contig record c"""
    def end(x):
        return "-" if x is None else "%x" % x
    out = ["return %d" % changed]
    for key, cov, slots in nodes:
        out.append("N %x %d %d %d %d" % (key, *cov))
        for i, c in enumerate(slots):
            if c >= 0:
                n1, n2, _, i1, i2 = contigs[c][:5]
                out.append("S %d %d %d %d %s %s %s" % (i, joined[c][0], i1, i2, end(n1), end(n2), "%.17g" % joined[c][1]))
    for c, t in enumerate(contigs):
        if t[5]:
            out.append("I %d %d %d %s" % (joined[c][0], t[3], t[4], "%.17g" % joined[c][1]))
    return "\n".join(out) + "\n"


def counts_line(info):
    """the last line of the table from a plan's info"""
    return "counts %d %d %d\n" % (info["tips"], info["nodes"], info["collapsed_1"] + info["degenerate_1"] if info["validated"] else -1)


def files_of_plan(plan, calls, k):
    """(FASTA bytes, graph table text) a Plan comes to over the calls of a tests/graph_build_ref.py build, the text by tests/detip_ref.join"""
    triples = triples_of(calls)
    printed = J.join(triples, [p for _, p in plan.records], k) if plan.records else []
    graph = J.join(triples, [t[6] for t in plan.contigs], k) if plan.contigs else []
    for t, j in zip(plan.contigs, graph):
        assert t[2] == len(j[0]), (t, len(j[0]))                           # the plan's joined length, from the len fields alone
    table = table_of(plan.nodes, plan.contigs, [(len(j[0]), j[3]) for j in graph], plan.info["changed"]) + counts_line(plan.info)
    return fasta_of(plan.records, printed), table
