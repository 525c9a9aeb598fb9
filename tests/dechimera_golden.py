"""The goldens of ContigGraph::removeChimerasAndClean behind deleteTipsAndClean (tests/golden/dechimera_<name>.fasta.gz and .graph.gz, made by
tests/golden/make_chimera_golden.py from the compiled reference) and what a plan (fgpu_chimera_plan's outputs) comes to in their terms, for
tests/test_dechimera_plan_cpu.py, tests/test_gpu_dechimera.py and the script itself.  Built on tests/detip_golden.py, whose Plan, table and file
functions it uses.

The graph table (tests/golden/chimera_driver.cpp writes it) is the detip goldens' with "return <detip 0|1> <dechimera 0|1>" as its first line and
"counts <chimeric contigs removed> <nodes left> <nodes validateNoneCollapsible removed behind the step, or -1 where it did not run>" as its last."""
import gzip
import json
import os
import re
import struct
import subprocess

import numpy as np

from tests import detip_golden as D
from tests import detip_ref as J
from tests.golden_util import GOLDEN

ROOT = D.ROOT
SUMMARY = os.path.join(GOLDEN, "dechimera_summary.json")
INFO_KEYS = ("nodes_before", "removed", "cut_near", "cut_far", "cut_both", "collapsed_0", "collapsed_1", "degenerate_0", "degenerate_1", "collapsed_after_cut",
             "skipped_0", "skipped_1", "skipped_2", "skipped_3", "skipped_4", "skipped_5", "validated", "changed", "records", "bubble_records", "node_contigs",
             "isolated_kept", "isolated_dropped", "nodes")
TIPS_KEYS = D.INFO_KEYS[:9]
SOURCES = [os.path.join(ROOT, "tests", "host", "chimera_plan_check.cpp"), os.path.join(ROOT, "faucet_amd", "csrc", "tips_plan.cpp")]
NO_LIMIT = D.NO_LIMIT
SANITIZER_ENV = dict(ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")


def summary():
    if not os.path.exists(SUMMARY):                  # (only while tests/golden/make_chimera_golden.py is making it)
        return {"fixtures": {}, "not_returned": {}, "reached": {}, "not_reached": []}
    with open(SUMMARY) as f:
        return json.load(f)


def golden(name, kind):
    with gzip.open(os.path.join(GOLDEN, f"dechimera_{name}.{kind}.gz"), "rb") as f:
        return f.read()


def compile_check(exe, sanitize):
    flags = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined"] if sanitize else []
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", *flags, *SOURCES, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


class Plan(D.Plan):
    """what chimera_plan_check printed (`text`): tests/detip_golden.Plan with info over INFO_KEYS and tips_info, the first step's account, over TIPS_KEYS"""

    def __init__(self, text):
        self.text = text
        lines = text.splitlines()
        super().__init__("\n".join(lines[:4] + lines[5:]))
        self.info = dict(zip(INFO_KEYS, (int(v) for v in lines[3].split()[1:])))
        assert len(lines[3].split()) == len(INFO_KEYS) + 1 and lines[4].startswith("tips ")
        self.tips_info = dict(zip(TIPS_KEYS, (int(v) for v in lines[4].split()[1:])))


def summaries_of(calls):
    """one COV_SUMMARY_DTYPE record per call of a tests/graph_build_ref.py build, by numpy: what fgpu_stage3_cov_calls gives on the device"""
    from faucet_amd import api
    out = np.zeros(len(calls), dtype=api.COV_SUMMARY_DTYPE)
    for c, w in enumerate(calls):
        v = list(w.contig.coverages)
        out[c] = (sum(v), len(v), v[0] if v else 0, v[-1] if v else 0, (0, 0))
    return out


def run_check(exe, path, keys, recs, contigs, calls, covs, k, read_length, cap=NO_LIMIT, mode=("plan",)):
    """mode: ("plan",) or ("live",) or ("live", <refusal>) -- the Plan of what the program printed (a Live in live mode)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<QQiiQ", len(keys), len(contigs), k, read_length, cap))
        for a in (np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(recs), contigs, calls, covs):
            f.write(a.tobytes())
    r = subprocess.run([exe, mode[0], path, *mode[1:]], capture_output=True, text=True, timeout=120, env=dict(os.environ, **SANITIZER_ENV))
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return Plan(r.stdout) if mode[0] == "plan" else Live(r.stdout)


class Live(Plan):
    """what `chimera_plan_check live` printed: `text`, its output without the S0, S and refused lines (what `plan` prints); s0 [(summary, pieces)]
    right behind set_cov and s [summary] behind the step, per contig the graph holds, summary = (sum, n, first, last); refused: the words behind
    "refused", or None"""

    def __init__(self, text):
        lines = text.splitlines(keepends=True)
        own = [ln for ln in lines if ln.split(" ", 1)[0] in ("S0", "S", "refused")]
        self.text = "".join(ln for ln in lines if ln.split(" ", 1)[0] not in ("S0", "S", "refused"))
        super().__init__(self.text)
        self.s0, self.s, self.refused = [], [], None
        for ln in own:
            head, _, tail = ln.partition(":")
            f = head.split()
            if f[0] == "refused":
                self.refused = f[1:]
                continue
            which = self.s0 if f[0] == "S0" else self.s
            assert int(f[1]) == len(which), ln
            v = [int(x) for x in tail.split()]
            summary = tuple(int(x) for x in f[2:6])
            which.append((summary, list(zip(v[::2], (bool(x) for x in v[1::2])))) if f[0] == "S0" else summary)


def run_fold(exe, path, lines):
    """lines: (way 'L' | 'R', [(flip, [coverage entries])]) -> [(sum, n, first, last, average as %.17g)]"""
    with open(path, "w") as f:
        for way, pieces in lines:
            f.write(way + "".join(" %d %d %s" % (int(fl), len(v), " ".join(map(str, v))) for fl, v in pieces) + "\n")
    r = subprocess.run([exe, "fold", path], capture_output=True, text=True, timeout=120, env=dict(os.environ, **SANITIZER_ENV))
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return [(int(a), int(b), int(c), int(d), e) for a, b, c, d, e in (ln.split() for ln in r.stdout.splitlines())]


def counts_said(said):
    """the counts line from what tests/golden/chimera_driver.cpp's run printed: the reference's own sentences behind "== chimeras" (the one place
    that reads them: tests/golden/make_chimera_golden.py and tests/stage3_fuzz_cases.py both come here)"""
    said = said.split("== chimeras\n", 1)[1]
    chim = re.search(r"removed (\d+) chimeric contigs\.\s+(\d+) nodes left", said)
    removed = re.search(r"removed (\d+) collapsible nodes\.\s+(\d+) nodes left", said)
    return "counts %s %s %s\n" % (chim.group(1), removed.group(2) if removed else chim.group(2), removed.group(1) if removed else -1)


def counts_line(info):
    return "counts %d %d %d\n" % (info["removed"], info["nodes"], info["collapsed_1"] + info["degenerate_1"] if info["validated"] else -1)


def table_of(nodes, contigs, joined, detipped, info):
    """the graph table of a plan: tests/detip_golden.table_of's with both return values in front and this step's counts behind"""
    body = D.table_of(nodes, contigs, joined, 0).split("\n", 1)[1]
    return "return %d %d\n" % (detipped, info["changed"]) + body + counts_line(info)


def files_of(nodes, contigs, records, info, tips_changed, calls, k):
    """(FASTA bytes, graph table text) of a plan's outputs over the calls of a tests/graph_build_ref.py build, the text and the coverage lists by
    tests/detip_ref.join"""
    triples = D.triples_of(calls)
    printed = J.join(triples, [p for _, p in records], k) if records else []
    graph = J.join(triples, [t[6] for t in contigs], k) if contigs else []
    for t, j in zip(contigs, graph):
        assert t[2] == len(j[0]), (t, len(j[0]))
    return D.fasta_of(records, printed), table_of(nodes, contigs, [(len(j[0]), j[3]) for j in graph], tips_changed, info)


def files_of_plan(plan, calls, k):
    return files_of(plan.nodes, plan.contigs, plan.records, plan.info, plan.tips_info["changed"], calls, k)
