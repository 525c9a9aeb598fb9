#!/usr/bin/env python3
"""The reference's graph and contig file after the first step of ContigGraph::cleanGraph, deleteTipsAndClean (src/ContigGraph.cpp:168-175), for
the Stage-3 fixtures:
    make -C oracle ref && python tests/golden/make_detip_golden.py
tests/golden/detip_driver.cpp (our own text: it includes the reference's headers; nodeMap and isolated_contigs are private, so its compile line
carries -fno-access-control) is built by oracle/Makefile (target ref) against the compiled reference's objects under oracle/_ref/obj;
the binary goes to oracle/_ref/ and is never committed.  For every fixture of tests/stage3_variants.py the driver reloads the map as
tests/golden/raw_contigs_driver.cpp does (so the map's order is the stored raw_contigs_<name>.order.gz), builds the graph, runs the step, writes
the graph as a table and prints the contigs.  Stored: detip_<name>.fasta.gz and detip_<name>.graph.gz (the table, and as its last line the counts
the reference printed; tests/detip_golden.py says how it reads).  The 13 unvaried fixtures must return; a variant is kept only where the reference
exits 0 within the time limit (the others are listed in detip_summary.json under not_returned), and the kept set must be the raw goldens'.
The script fails unless the set holds: a fixture on which every node goes and records remain (twohash_k31_L150), two empty files
(twohash_k31_L150__drop70, s3_k8__drop70), a change with return value 0 (s3_k24_long__drop30), no change at all (c1_k21__mrl10, whose file is the
raw golden), a bubble record over joined lists, an isolated contig made by a collapse, and a back tip deleted uncounted -- the last three judged
from fgpu_tips_plan's own account of the fixture, once its files equal the reference's."""
import glob
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from tests import stage3_variants as V  # noqa: E402
from tests.golden_util import Case  # noqa: E402
from make_raw_contigs_golden import OUT, TIME_LIMIT  # noqa: E402
from make_raw_contigs_golden import build_driver as raw_build_driver  # noqa: E402

DRIVER = os.path.join(OUT, "detip_driver")


def written_here(path):
    return os.path.relpath(path, HERE).startswith("detip_") and not path.endswith(".cpp")


def check_sizes():
    """no file this script writes is larger than the largest file under tests/golden that it does not write"""
    sizes = {os.path.join(d, f): os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(HERE) for f in fs}
    limit = max(n for p, n in sizes.items() if not written_here(p))
    too_large = {os.path.relpath(p, HERE): n for p, n in sizes.items() if written_here(p) and n > limit}
    assert not too_large, (limit, too_large)


def build_driver():
    raw_build_driver(DRIVER)


def reference_files(c, bloom, lines, max_read_length):
    """(fasta bytes, graph table with its counts line) of the driver on this filter and map, or (None, why) where the reference does not return"""
    with tempfile.TemporaryDirectory() as td:
        b, j, fa, gr = (os.path.join(td, n) for n in ("b.bloom", "j.junctions", "out.fasta", "out.graph"))
        open(b, "wb").write(bloom.tobytes())
        open(j, "w").write("\n".join(lines) + "\n")
        try:
            r = subprocess.run([DRIVER, b, str(len(bloom) * 8 - 1), str(c.counters["n_hash"]), str(c.k), str(c.j), j, str(max_read_length), fa, gr],
                               capture_output=True, timeout=TIME_LIMIT)
        except subprocess.TimeoutExpired:
            return None, "no return within %d s" % TIME_LIMIT
        if r.returncode != 0:
            return None, "exit %d" % r.returncode
        said = r.stdout.decode(errors="replace")
        tips = re.search(r"Deleted (\d+) tips\. (\d+) nodes left", said)
        removed = re.search(r"removed (\d+) collapsible nodes\.\s+(\d+) nodes left", said)
        counts = "counts %s %s %s\n" % (tips.group(1), removed.group(2) if removed else tips.group(2), removed.group(1) if removed else -1)
        return open(fa, "rb").read(), open(gr).read() + counts


def main():
    from tests import detip_golden as D
    from tests import raw_contigs_ref as P
    from tests import test_raw_contigs_ref_cpu as T
    build_driver()
    for p in glob.glob(os.path.join(HERE, "detip_*.gz")):
        os.remove(p)
    kept, not_returned = {}, {}
    for name in V.fixture_names():
        c = Case(name.split("__")[0])
        bloom, lines, mrl = V.inputs_of(name, c)
        fasta, table = reference_files(c, bloom, lines, mrl)
        if fasta is None:
            assert "__" in name, (name, table)              # the unvaried fixtures return
            not_returned[name] = table
            print(name, "not kept:", table)
            continue
        assert "?" not in table, name                        # no contig of the table ends on a node that is gone
        for kind, data in (("fasta", fasta), ("graph", table.encode())):
            with gzip.GzipFile(os.path.join(HERE, f"detip_{name}.{kind}.gz"), "wb", mtime=0) as f:
                f.write(data)
        tips, nodes, removed = (int(v) for v in table.splitlines()[-1].split()[1:])
        seqs = fasta.decode().split("\n")[1::2]
        kept[name] = dict(k=c.k, read_length=mrl, bytes=len(fasta), records=len(seqs), longest=max(map(len, seqs), default=0), tips=tips, nodes=nodes,
                          removed=removed, changed=int(table.split()[1]), same_as_raw=int(fasta == T.golden_fasta(name)))
    assert sorted(kept) == T.NAMES, sorted(set(kept) ^ set(T.NAMES))
    # ---- what the kept set has to reach
    with tempfile.TemporaryDirectory() as td:
        exe = D.compile_check(os.path.join(td, "tips_plan_check"), sanitize=False)
        for name, s in kept.items():
            b, keys, recs = T.golden_build(name)[:3]
            contigs, calls, _ = P.arrays_of(b.calls)
            plan = D.run_check(exe, os.path.join(td, "plan.bin"), keys, recs, contigs, calls, s["k"], s["read_length"])
            assert plan.status == 0, (name, plan.status)
            fasta, table = D.files_of_plan(plan, b.calls, s["k"])
            assert fasta == D.golden(name, "fasta") and table == D.golden(name, "graph").decode(), name
            made = [t for t in plan.contigs if len(t[6]) > 1 and not (t[5] and len(t[6]) == 2 and t[6][0][1])]     # (not a linear region's own join)
            s.update({key: plan.info[key] for key in D.INFO_KEYS if key not in s},
                     joined_bubble_records=sum(len(p) > 2 for _, p in plan.records[:plan.info["bubble_records"]]),
                     isolated_by_collapse=sum(1 for t in made if t[5]), joined_contigs=len(made), most_pieces=max([len(t[6]) for t in plan.contigs], default=0))
            print(name, {key: s[key] for key in ("tips", "back_tips", "nodes_before", "nodes", "changed", "records", "joined_contigs", "longest")})
    reached = dict(
        every_node_goes_records_remain=[n for n, s in kept.items() if s["nodes_before"] and not s["nodes"] and s["records"]],
        empty_files=[n for n, s in kept.items() if not s["bytes"]],
        change_with_return_0=[n for n, s in kept.items() if not s["changed"] and (s["nodes"] != s["nodes_before"] or not s["same_as_raw"])],
        no_change=[n for n, s in kept.items() if not s["changed"] and s["nodes"] == s["nodes_before"] and s["same_as_raw"] and s["records"]],
        joined_bubble_records=[n for n, s in kept.items() if s["joined_bubble_records"]],
        isolated_by_collapse=[n for n, s in kept.items() if s["isolated_by_collapse"]],
        back_tips=[n for n, s in kept.items() if s["back_tips"]])
    print("reached", {key: len(v) for key, v in reached.items()})
    assert all(reached.values()), f"the goldens do not reach: {[key for key, v in reached.items() if not v]}"
    assert "twohash_k31_L150" in reached["every_node_goes_records_remain"] and {"twohash_k31_L150__drop70", "s3_k8__drop70"} <= set(reached["empty_files"])
    assert "s3_k24_long__drop30" in reached["change_with_return_0"] and "c1_k21__mrl10" in reached["no_change"]
    with open(os.path.join(HERE, "detip_summary.json"), "w") as f:
        json.dump({"reached": reached, "fixtures": kept, "not_returned": not_returned}, f, indent=1, sort_keys=True)
        f.write("\n")
    check_sizes()


if __name__ == "__main__":
    main()
