"""tests/raw_contigs_ref.py (ContigGraph::printContigs on buildContigGraph's graph, restated) against the compiled reference's own files
(tests/golden/raw_contigs_<name>.fasta.gz, made by tests/golden/make_raw_contigs_golden.py), byte for byte: the restatement runs over the
build tests/graph_build_ref.py gives with the oracle answering the probes, the map in the order the reference's reloaded map iterated in
(raw_contigs_<name>.order.gz).  And fgpu_raw_plan (faucet_amd/csrc/raw_plan.cpp), compiled with a main of its own under
-fsanitize=address,undefined as a stand-alone program, against the restatement's print list on every golden fixture and on the three seeded
map orders of the unvaried ones.  And `faucet --raw_contigs` on a library without the entry points.  No GPU."""
import functools
import gzip
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import graph_build_ref as G
from tests import raw_contigs_ref as P
from tests.golden_util import GOLDEN, Case
from tests.test_contig_ref_cpu import UNVARIED
from tests.test_graph_build_ref_cpu import ORDERS, build_of, finder_of
from tests.test_stage3_walker import _fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY = os.path.join(GOLDEN, "raw_contigs_summary.json")
_golden_builds = {}


def summary():
    if not os.path.exists(SUMMARY):                  # (only while tests/golden/make_raw_contigs_golden.py is making it)
        return {"fixtures": {}, "not_returned": {}, "total": {}}
    with open(SUMMARY) as f:
        return json.load(f)


NAMES = sorted(summary()["fixtures"])
PLAN_CASES = [(name, "golden") for name in NAMES] + [(name, o) for name in UNVARIED for o in ORDERS[1:]]


def golden_fasta(name):
    with gzip.open(os.path.join(GOLDEN, f"raw_contigs_{name}.fasta.gz"), "rb") as f:
        return f.read()


def golden_order(name):
    """the keys of the fixture's map in the order the reference's reloaded map iterated in"""
    with gzip.open(os.path.join(GOLDEN, f"raw_contigs_{name}.order.gz"), "rt") as f:
        return np.array([int(x, 16) for x in f.read().split()], dtype=np.uint64)


def build_over(f, order, k):
    """the Build of a Finder's map with its junctions in the order of the keys `order`, with the permuted keys and records"""
    row = {int(x): r for r, x in enumerate(f.keys)}
    perm = np.array([row[int(x)] for x in order], dtype=np.int64)
    assert sorted(perm.tolist()) == list(range(len(f.keys)))
    keys, recs = f.keys[perm], f.recs[perm]

    def find_neighbor(alive, kmer, index):
        a = np.empty(len(perm), dtype=bool)
        a[perm] = alive
        return f.find(a, kmer, index)
    return G.build_contig_graph(find_neighbor, keys, recs["cov"], k), keys, recs


def golden_build(name):
    """(Build, keys, records, Finder) of one fixture with its map in the golden order; made once, shared, left unchanged"""
    if name not in _golden_builds:
        fx, f = _fixture(name), finder_of(name)
        _golden_builds[name] = (*build_over(f, golden_order(name), fx.case.k), f)
    return _golden_builds[name]


def build_in(name, order):
    return golden_build(name)[:3] if order == "golden" else build_of(name, order)[:3]


def test_the_goldens_are_the_set_the_script_asks_for():
    s = summary()
    assert set(UNVARIED) <= set(NAMES) and len(UNVARIED) == 13 and not set(s["not_returned"]) & set(NAMES)
    assert all(s["total"][key] > 0 for key in ("bubble_records", "isolated_kept", "isolated_dropped", "far_is_start", "exactly_k", "below_32", "above_32",
                                               "below_64", "above_64"))


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_writes_the_references_file(name):
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    assert b.status == 0
    got, info, _ = P.raw_contigs(b.calls, keys, recs["cov"], fx.case.k, fx.max_read_length)
    assert got == golden_fasta(name)
    want = summary()["fixtures"][name]
    assert {key: want[key] for key in info} == info


def test_canon_contig_compares_letters_not_codes():
    assert P.canon_contig("AG") == "AG" and P.canon_contig("CT") == "AG"      # G < T as letters, T < G as codes
    assert P.canon_contig("ACGT") == "ACGT" and P.canon_contig("TTTA") == "TAAA"
    assert P.join(["ACGTA", "TACCC"], [False, False], 2) == "ACGTACCC" and P.join(["ACGTA", "GGGTA"], [False, True], 2) == "ACGTACCC"
    assert P.join(["TACGT", "TACCC"], [True, False], 2) == "ACGTACCC"


# ---- fgpu_raw_plan as a stand-alone program under the sanitizers ----
@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("raw_plan") / "raw_plan_check")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-Wall",
                        os.path.join(ROOT, "tests", "host", "raw_plan_check.cpp"), os.path.join(ROOT, "faucet_amd", "csrc", "raw_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run_plan(exe, path, keys, recs, contigs, calls, k, read_length, cap):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQiiQ", len(keys), len(contigs), k, read_length, cap))
        for a in (np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(recs), contigs, calls):
            f.write(a.tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1"))
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    status, n = (int(v) for v in lines[0].split()[1::2])
    return status, n, [int(v) for v in lines[1].split()[1:]], lines[2:]


@pytest.mark.parametrize("name, order", PLAN_CASES)
def test_the_plan_program_against_the_restatement(plan_exe, tmp_path, name, order):
    b, keys, recs = build_in(name, order)
    fx = _fixture(name)
    contigs, calls, _ = P.arrays_of(b.calls)
    path = str(tmp_path / "plan.bin")
    try:                                              # (a build that stopped is a prefix of one: the plan is made of it all the same)
        records, info = P.plan(b.calls, keys, recs["cov"], fx.case.k, fx.max_read_length)
    except (P.UnsetContig, P.NotABuild) as e:
        assert _run_plan(plan_exe, path, keys, recs, contigs, calls, fx.case.k, fx.max_read_length, len(contigs))[0] == (1 if isinstance(e, P.UnsetContig) else 2)
        return
    status, n, counts, lines = _run_plan(plan_exe, path, keys, recs, contigs, calls, fx.case.k, fx.max_read_length, len(contigs))
    assert (status, n) == (0, len(records))
    assert counts == [info[key] for key in ("records", "bubble_records", "node_contigs", "isolated_kept", "isolated_dropped", "nodes")]
    assert lines == P.plan_lines(records, contigs)


def test_the_plan_program_on_short_room_and_on_arrays_that_are_no_build(plan_exe, tmp_path):
    name = "twohash_k31_L150"                         # (linear regions on both sides of the read length, so the last call is a backward one)
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    contigs, calls, _ = P.arrays_of(b.calls)
    records, info = P.plan(b.calls, keys, recs["cov"], fx.case.k, fx.max_read_length)
    path = str(tmp_path / "plan.bin")
    run = functools.partial(_run_plan, plan_exe, path)
    status, n, counts, lines = run(keys, recs, contigs, calls, fx.case.k, fx.max_read_length, len(records) - 1)
    assert (status, n, counts[0]) == (3, len(records), len(records)) and lines == P.plan_lines(records, contigs)[:-1]
    assert run(keys[:0], recs[:0], contigs[:0], calls[:0], fx.case.k, fx.max_read_length, 0)[:3] == (0, 0, [0] * 6)
    assert run(keys, recs, contigs[:-1], calls[:-1], fx.case.k, fx.max_read_length, len(contigs))[0] == 2        # a forward call without its backward one
    assert b.calls[-1].phase == G.LINEAR_BACKWARD and info["isolated_kept"] and info["isolated_dropped"]
    without = np.arange(len(keys)) != int(np.nonzero((np.asarray(recs["cov"]) > 0).sum(axis=1) > 1)[0][0])
    assert run(keys[without], recs[without], contigs, calls, fx.case.k, fx.max_read_length, len(contigs))[0] == 2       # calls of a start that is not in the map
    bad = contigs.copy()
    bad["ind2"][0] = 5
    assert run(keys, recs, bad, calls, fx.case.k, fx.max_read_length, len(contigs))[0] == 2
    read_length_above_all = 1 << 20
    status, n, counts, _ = run(keys, recs, contigs, calls, fx.case.k, read_length_above_all, len(contigs))
    assert status == 0 and counts[3] == 0 and counts[4] == info["isolated_kept"] + info["isolated_dropped"]


# ---- the command line on a library without the entry points ----
def test_cli_raw_contigs_without_the_entry_points_exits_2_before_any_input(tmp_path):
    """tests/stub/faucet_gpu_stub.cpp answers the C ABI without fgpu_stage3_build and fgpu_stage3_raw_contigs: --raw_contigs is refused with exit
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
    r = subprocess.run([exe, "-read_load_file", missing, "-read_scan_file", missing, "-file_prefix", prefix, "--raw_contigs"] + c.meta["args"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--raw_contigs" in r.stderr and "fgpu_stage3_raw_contigs" in r.stderr and "lacks" in r.stderr
    assert r.stdout == "" and os.listdir(str(tmp_path)) == ["faucet_stub"]
