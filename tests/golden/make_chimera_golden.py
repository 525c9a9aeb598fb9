#!/usr/bin/env python3
"""The reference's graph and contig file after the first two steps of ContigGraph::cleanGraph, deleteTipsAndClean and removeChimerasAndClean
(src/ContigGraph.cpp:168-184), for the Stage-3 fixtures:
    make -C oracle ref && python tests/golden/make_chimera_golden.py
tests/golden/chimera_driver.cpp (our own text: it includes the reference's headers; nodeMap and isolated_contigs are private, so its compile line
carries -fno-access-control) is built by oracle/Makefile's recipe (`make ref` builds it too), as the two other Stage-3 drivers are; the binary
goes to oracle/_ref/ and is never committed.  For every fixture of tests/stage3_variants.py the driver reloads the map as
tests/golden/raw_contigs_driver.cpp does, builds the graph, runs the two steps, writes the graph as a table and prints the contigs.  Stored:
dechimera_<name>.fasta.gz and dechimera_<name>.graph.gz (the table, and as its last line the counts the reference printed;
tests/dechimera_golden.py says how it reads) and dechimera_summary.json.  A variant is kept only where the reference exits 0 within the time
limit, and the kept set must be the detip goldens'.
The script fails unless the set holds each of the three outcomes of a chimeric extension (cut at the node, at the far node, at both), a collapse
right behind a cut, a collapse of a node the loop came to with one path out, a node left alone because P sits in its far node's slot 4, one
because P is not the far node's lowest extension, one because the ratio is below 3, and a fixture where the step removes nothing and the file is
the detip golden -- all judged from fgpu_chimera_plan's own account of the fixture, once its files equal the reference's.  A fixture whose
validation behind the step erases a node is listed if there is one, and under not_reached if there is none."""
import glob
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from tests import stage3_variants as V  # noqa: E402
from tests.dechimera_golden import counts_said  # noqa: E402
from tests.golden_util import Case  # noqa: E402
from make_raw_contigs_golden import OUT, TIME_LIMIT  # noqa: E402
from make_raw_contigs_golden import build_driver as raw_build_driver  # noqa: E402

DRIVER = os.path.join(OUT, "chimera_driver")
REQUIRED = ("cut_near", "cut_far", "cut_both", "collapse_right_behind_a_cut", "collapse_of_a_node_met_with_one_path", "skipped_p_in_slot_4",
            "skipped_p_not_the_far_nodes_lowest", "skipped_ratio_below_3", "nothing_removed_file_is_the_detip_golden")


def written_here(path):
    return os.path.relpath(path, HERE).startswith("dechimera_") and not path.endswith(".cpp")


def check_sizes():
    """no file this script writes is larger than the largest file under tests/golden that it does not write"""
    sizes = {os.path.join(d, f): os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(HERE) for f in fs}
    limit = max(n for p, n in sizes.items() if not written_here(p))
    too_large = {os.path.relpath(p, HERE): n for p, n in sizes.items() if written_here(p) and n > limit}
    assert not too_large, (limit, too_large)


def build_driver():
    """oracle/Makefile holds the one recipe of the three drivers"""
    raw_build_driver(DRIVER)


def reference_files(c, bloom, lines, max_read_length, driver=DRIVER):
    """(fasta bytes, graph table with its counts line) of the driver on this filter and map, or (None, why) where the reference does not return"""
    with tempfile.TemporaryDirectory() as td:
        b, j, fa, gr = (os.path.join(td, n) for n in ("b.bloom", "j.junctions", "out.fasta", "out.graph"))
        open(b, "wb").write(bloom.tobytes())
        open(j, "w").write("\n".join(lines) + "\n")
        try:
            r = subprocess.run([driver, b, str(len(bloom) * 8 - 1), str(c.counters["n_hash"]), str(c.k), str(c.j), j, str(max_read_length), fa, gr],
                               capture_output=True, timeout=TIME_LIMIT)
        except subprocess.TimeoutExpired:
            return None, "no return within %d s" % TIME_LIMIT
        if r.returncode != 0:
            return None, "exit %d" % r.returncode
        return open(fa, "rb").read(), open(gr).read() + counts_said(r.stdout.decode(errors="replace"))


def reached_by(kept):
    return dict(
        cut_near=[n for n, s in kept.items() if s["cut_near"]], cut_far=[n for n, s in kept.items() if s["cut_far"]],
        cut_both=[n for n, s in kept.items() if s["cut_both"]],
        collapse_right_behind_a_cut=[n for n, s in kept.items() if s["collapsed_after_cut"]],
        # "a node that an earlier cut of this loop made collapsible": one the loop met with a single path out, in a run that cut something -- the
        # detip in front collapses or erases every node it leaves with one path out, so only a cut of this loop can have made it so
        collapse_of_a_node_met_with_one_path=[n for n, s in kept.items() if s["removed"] and s["collapsed_0"] > s["collapsed_after_cut"]],
        skipped_p_in_slot_4=[n for n, s in kept.items() if s["skipped_1"]],
        skipped_p_not_the_far_nodes_lowest=[n for n, s in kept.items() if s["skipped_5"]],
        skipped_ratio_below_3=[n for n, s in kept.items() if s["skipped_4"]],
        nothing_removed_file_is_the_detip_golden=[n for n, s in kept.items() if not s["removed"] and s["same_as_detip"] and s["records"]],
        validation_erases_a_node=[n for n, s in kept.items() if s["collapsed_1"] + s["degenerate_1"]])


def main():
    from tests import dechimera_golden as C
    from tests import detip_golden as D
    from tests import raw_contigs_ref as P
    from tests import test_raw_contigs_ref_cpu as T
    build_driver()
    for p in glob.glob(os.path.join(HERE, "dechimera_*.gz")):
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
            with gzip.GzipFile(os.path.join(HERE, f"dechimera_{name}.{kind}.gz"), "wb", mtime=0) as f:
                f.write(data)
        removed, nodes, validated = (int(v) for v in table.splitlines()[-1].split()[1:])
        seqs = fasta.decode().split("\n")[1::2]
        kept[name] = dict(k=c.k, read_length=mrl, bytes=len(fasta), longest=max(map(len, seqs), default=0), reference_removed=removed, reference_nodes=nodes,
                          reference_validation=validated, same_as_detip=int(fasta == D.golden(name, "fasta")))
    assert sorted(kept) == sorted(D.summary()["fixtures"]) and len(kept) == 28, sorted(set(kept) ^ set(D.summary()["fixtures"]))
    # ---- what the kept set has to reach, by fgpu_chimera_plan's own account
    with tempfile.TemporaryDirectory() as td:
        exe = C.compile_check(os.path.join(td, "chimera_plan_check"), sanitize=False)
        for name, s in kept.items():
            b, keys, recs = T.golden_build(name)[:3]
            contigs, calls, _ = P.arrays_of(b.calls)
            plan = C.run_check(exe, os.path.join(td, "plan.bin"), keys, recs, contigs, calls, C.summaries_of(b.calls), s["k"], s["read_length"])
            assert plan.status == 0, (name, plan.status)
            fasta, table = C.files_of_plan(plan, b.calls, s["k"])
            assert fasta == C.golden(name, "fasta") and table == C.golden(name, "graph").decode(), name
            assert (plan.info["removed"], plan.info["nodes"]) == (s["reference_removed"], s["reference_nodes"]), name
            s.update(plan.info)
            print(name, {key: s[key] for key in ("removed", "cut_near", "cut_far", "cut_both", "collapsed_0", "collapsed_after_cut", "collapsed_1", "degenerate_1",
                                                 "skipped_1", "skipped_4", "skipped_5", "nodes", "records")})
    reached = reached_by(kept)
    print("reached", {key: len(v) for key, v in reached.items()})
    missing = [key for key in REQUIRED if not reached[key]]
    assert not missing, f"the goldens do not reach: {missing} (add seeded cases: tests/chimera_cases.py)"
    not_reached = [key for key, v in reached.items() if not v]
    with open(os.path.join(HERE, "dechimera_summary.json"), "w") as f:
        json.dump({"reached": reached, "not_reached": not_reached, "fixtures": kept, "not_returned": not_returned}, f, indent=1, sort_keys=True)
        f.write("\n")
    check_sizes()


if __name__ == "__main__":
    main()
