"""fgpu_tips_plan (faucet_amd/csrc/tips_plan.cpp: ContigGraph::deleteTipsAndClean and printContigs behind it, over piece lists) against the compiled
reference's own files after the step (tests/golden/detip_<name>.fasta.gz and .graph.gz, made by tests/golden/make_detip_golden.py), byte for byte:
the plan is compiled with a main of its own (tests/host/tips_plan_check.cpp) under -fsanitize=address,undefined as a stand-alone program and run
over the build tests/graph_build_ref.py gives with the map in the order the reference's reloaded map iterated in; the text and the coverages of its
lists come from tests/detip_ref.join.  tests/detip_plan_ref.py, the same step restated in plain Python, writes the same files; on the three seeded map
orders of the unvaried fixtures, where there is no reference file, the program and the library's build of the same source must say what the restatement
says.  And `faucet --detipped_contigs` on a library without the entry points.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import detip_golden as D
from tests import detip_plan_ref as R
from tests import raw_contigs_ref as P
from tests.golden_util import Case
from tests.test_contig_ref_cpu import UNVARIED
from tests.test_graph_build_ref_cpu import ORDERS
from tests.test_raw_contigs_ref_cpu import NAMES as RAW_NAMES
from tests.test_raw_contigs_ref_cpu import build_in, golden_fasta
from tests.test_stage3_walker import _fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(D.summary()["fixtures"])


def test_the_goldens_are_the_set_the_script_asks_for():
    s = D.summary()
    assert NAMES == RAW_NAMES and len(NAMES) == 28 and set(UNVARIED) <= set(NAMES) and not set(s["not_returned"]) & set(NAMES) and len(s["not_returned"]) == 18
    r = s["reached"]
    assert "twohash_k31_L150" in r["every_node_goes_records_remain"] and {"twohash_k31_L150__drop70", "s3_k8__drop70"} <= set(r["empty_files"])
    assert "s3_k24_long__drop30" in r["change_with_return_0"] and "c1_k21__mrl10" in r["no_change"]
    assert r["joined_bubble_records"] and r["isolated_by_collapse"] and r["back_tips"]
    assert D.golden("c1_k21__mrl10", "fasta") == golden_fasta("c1_k21__mrl10")
    assert all(D.golden(n, "fasta") == b"" for n in r["empty_files"])
    assert sum(1 for n in UNVARIED if s["fixtures"][n]["tips"]) == 12 and max(f["longest"] for f in s["fixtures"].values()) == 3334
    assert 3 <= min(s["fixtures"][n]["tips"] for n in UNVARIED if s["fixtures"][n]["tips"]) and max(s["fixtures"][n]["tips"] for n in UNVARIED) == 53


def restated(calls, keys, recs, k, read_length):
    """tests/detip_plan_ref.plan's results, in the terms a tests/detip_golden.Plan holds them in"""
    return R.plan(calls, keys, recs["cov"], k, read_length)


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_writes_the_references_file_and_graph(name):
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    plan = D.Plan("sizing 0\nstatus 0\nsizes\ninfo\n")
    plan.nodes, plan.contigs, plan.records, plan.info = restated(b.calls, keys, recs, fx.case.k, fx.max_read_length)
    fasta, table = D.files_of_plan(plan, b.calls, fx.case.k)
    assert fasta == D.golden(name, "fasta")
    assert table == D.golden(name, "graph").decode()


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return D.compile_check(str(tmp_path_factory.mktemp("tips_plan") / "tips_plan_check"), sanitize=True)


@pytest.mark.parametrize("name", NAMES)
def test_the_plan_program_writes_the_references_file_and_graph(plan_exe, tmp_path, name):
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    assert b.status == 0
    contigs, calls, _ = P.arrays_of(b.calls)
    plan = D.run_check(plan_exe, str(tmp_path / "plan.bin"), keys, recs, contigs, calls, fx.case.k, fx.max_read_length)
    assert plan.status == 0 and plan.sizing == (3 if any(plan.sizes) else 0)
    assert plan.sizes == [len(plan.nodes), len(plan.contigs), sum(len(t[6]) for t in plan.contigs), len(plan.records), sum(len(p) for _, p in plan.records)]
    fasta, table = D.files_of_plan(plan, b.calls, fx.case.k)
    assert fasta == D.golden(name, "fasta")
    assert table == D.golden(name, "graph").decode()
    want = D.summary()["fixtures"][name]
    assert {key: want[key] for key in D.INFO_KEYS} == plan.info
    assert (plan.nodes, plan.contigs, plan.records, plan.info) == restated(b.calls, keys, recs, fx.case.k, fx.max_read_length)
    used = [c for t in plan.contigs for c, _ in t[6]]
    assert len(used) == len(set(used))                                        # a call lies in one contig of the graph left


@pytest.mark.parametrize("name, order", [(name, o) for name in UNVARIED for o in ORDERS[1:]])
def test_the_plan_program_and_the_library_against_the_restatement_on_seeded_orders(plan_exe, tmp_path, name, order):
    """other orders of the same maps, where the loops meet the nodes in another order (no reference file: the reloaded map has the one order)"""
    from faucet_amd import api
    b, keys, recs = build_in(name, order)
    fx = _fixture(name)
    contigs, calls, _ = P.arrays_of(b.calls)
    plan = D.run_check(plan_exe, str(tmp_path / "plan.bin"), keys, recs, contigs, calls, fx.case.k, fx.max_read_length)
    status, graph, records, info = api.tips_plan(keys, recs, contigs, calls, fx.case.k, fx.max_read_length)
    assert status == plan.status
    try:                                              # (a build that stopped is a prefix of one: the plan is made of it all the same)
        want = restated(b.calls, keys, recs, fx.case.k, fx.max_read_length)
    except (R.Unset, P.UnsetContig, P.NotABuild) as e:
        assert status == (2 if isinstance(e, P.NotABuild) else 1) and graph is None
        return
    assert status == 0 and (plan.nodes, plan.contigs, plan.records, plan.info) == want
    assert records == plan.records and graph["lists"] == [t[6] for t in plan.contigs]
    assert [(int(n["key"]), [int(v) for v in n["cov"]], [int(v) for v in n["slot"]]) for n in graph["nodes"]] == plan.nodes
    assert [int(v) for v in graph["contigs"]["len"]] == [t[2] for t in plan.contigs]
    assert (info["tips"], info["back_tips"], info["print"]["records"], info["print"]["nodes"]) == tuple(plan.info[key] for key in ("tips", "back_tips", "records", "nodes"))
    D.files_of_plan(plan, b.calls, fx.case.k)                                  # the lists join, to the lengths the plan says
    live = {c for t in plan.contigs for c, _ in t[6]}
    assert all(c in live for _, p in plan.records for c, _ in p)              # what is printed is of the graph left


def test_the_plan_program_on_short_room_and_on_arrays_that_are_no_build(plan_exe, tmp_path):
    name = "twohash_k31_L150"
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    contigs, calls, _ = P.arrays_of(b.calls)
    path = str(tmp_path / "plan.bin")

    def run(keys, recs, contigs, calls, read_length=fx.max_read_length, cap=D.NO_LIMIT):
        return D.run_check(plan_exe, path, keys, recs, contigs, calls, fx.case.k, read_length, cap)
    full = run(keys, recs, contigs, calls)
    assert full.status == 0 and min(full.sizes[1:]) > 1
    for cap in (0, 1, min(full.sizes[1:]) - 1, max(full.sizes) - 1):           # room for too little: the sizes and the info all the same
        short = run(keys, recs, contigs, calls, cap=cap)
        assert short.status == 3 and short.sizes == full.sizes and short.info == full.info
    empty = run(keys[:0], recs[:0], contigs[:0], calls[:0])
    assert (empty.sizing, empty.status, empty.sizes) == (0, 0, [0] * 5) and not any(empty.info.values())
    assert run(keys, recs, contigs[:-1], calls[:-1]).status == 2               # a forward call without its backward one
    without = np.arange(len(keys)) != int(np.nonzero((np.asarray(recs["cov"]) > 0).sum(axis=1) > 1)[0][0])
    assert run(keys[without], recs[without], contigs, calls).status == 2       # calls of a start that is not in the map
    bad = contigs.copy()
    bad["ind2"][0] = 5
    assert run(keys, recs, bad, calls).status == 2
    long_reads = run(keys, recs, contigs, calls, read_length=1 << 20)          # every contig that hangs on one node is a tip, no isolated contig is printed
    assert long_reads.status == 0 and long_reads.info["isolated_kept"] == 0 and long_reads.info["tips"] >= full.info["tips"]
    no_tips = run(keys, recs, contigs, calls, read_length=0)                   # nothing is a tip: the graph is the build's, the file the raw contigs'
    assert no_tips.status == 0 and not no_tips.info["changed"] and no_tips.info["nodes"] == no_tips.info["nodes_before"]
    assert all(len(p) <= 2 for _, p in no_tips.records)


# ---- the command line on a library without the entry points ----
def test_cli_detipped_contigs_without_the_entry_points_exits_2_before_any_input(tmp_path):
    """tests/stub/faucet_gpu_stub.cpp answers the C ABI without fgpu_stage3_build and fgpu_stage3_detip: --detipped_contigs is refused with exit
    code 2 and a message before any input is opened (the inputs named here do not exist) and before anything is written"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "faucet_stub")
    src = [os.path.join(ROOT, "faucet_amd", "host", "faucet_main.cpp"), os.path.join(ROOT, "tests", "stub", "faucet_gpu_stub.cpp"),
           os.path.join(ROOT, "oracle", "faucet_oracle.cpp"), os.path.join(ROOT, "faucet_amd", "csrc", "sizing.cpp")]
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), *src, "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    c = Case("c1_k21")
    missing = str(tmp_path / "no_such_reads.fa")
    prefix = str(tmp_path / "out")
    for flags in (["--detipped_contigs"], ["--raw_contigs", "--detipped_contigs"]):
        r = subprocess.run([exe, "-read_load_file", missing, "-read_scan_file", missing, "-file_prefix", prefix] + flags + c.meta["args"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
        assert "lacks" in r.stderr and ("fgpu_stage3_detip" in r.stderr or "fgpu_stage3_raw_contigs" in r.stderr)
        assert r.stdout == "" and os.listdir(str(tmp_path)) == ["faucet_stub"]
    assert "--detipped_contigs" in r.stderr or "--raw_contigs" in r.stderr
