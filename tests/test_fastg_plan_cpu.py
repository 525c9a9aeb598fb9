"""ContigGraph::printGraph on the host: CleanGraph::fastg_records (faucet_amd/csrc/clean_graph.h) and the name function the kernel shares
(faucet_amd/csrc/fastg_name.h), as a stand-alone program (tests/host/fastg_plan_check.cpp) built under -fsanitize=address,undefined and run directly,
against tests/fastg_ref.py over THE REFERENCE'S graph tables.  No GPU.

The file the program renders on the host has to be, byte for byte, what the restatement prints from the reference's table of the same graph: the
detip_*.graph.gz and dechimera_*.graph.gz goldens of all 28 fixtures, the graph tests/detip_plan_ref.py holds before its step for the raw graph,
and, where oracle/_ref is built, the tables oracle/_ref/detip_driver and chimera_driver write on the spot for the seeded maps of
tests/chimera_cases.py.  The table gives the walk's order, every length, index, end and average; the program gives only what no table holds: the
letters (its piece lists, joined by tests/detip_ref.join and held to the table's lengths and averages) and the contig numbers that stand for <this>.

printf's %g: the program's fmt mode holds fgpu_fastg_g to snprintf("%g") of the double on every (sum, n) with n <= 300, 10^6 seeded pairs with n
up to 2^32 - 1 and the traps (200001/200000, the decimal tie the double is not; 1601/16; 1/100000; 0/n; 255/1; 23/2).

FGPU_PLAN_UNSET is pinned on graphs changed by hand, the same change made to the table where a table can say it: an index that is neither end's
(Contig::getSide finds nothing), a node that is gone under a contig's end, a deleted contig left hanging in a slot."""
import collections
import ctypes as C
import os
import shutil
import subprocess

import pytest

from tests import chimera_cases
from tests import dechimera_golden as G
from tests import detip_golden as D
from tests import fastg_cases as FC
from tests import fastg_ref as F
from tests import stage3_fuzz_cases as S
from tests.golden_util import Case
from tests.test_raw_contigs_ref_cpu import build_in
from tests.test_stage3_walker import _fixture

ROOT = FC.ROOT
NAMES = sorted(G.summary()["fixtures"])
SHAPES = ("no_neighbours_on_either_side", "four_neighbours", "both_ends_on_one_node", "degenerate_loop", "primed_neighbour_under_a_primed_header",
          "isolated_below_read_length", "isolated_at_exactly_read_length")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return FC.compile_check(str(tmp_path_factory.mktemp("fastg_plan") / "fastg_plan_check"))


def test_the_shared_name_function_prints_what_percent_g_prints(check_exe):
    checked, mismatches, lines = FC.run_fmt(check_exe)
    assert mismatches == 0, lines[:20]
    assert checked == sum(255 * n + 1 for n in range(1, 301)) + 1000000 + 14


def shapes_of(graph, recs, read_length):
    out = collections.Counter()
    for r in recs:
        t = graph.contigs[r.contig]
        out[SHAPES[0]] += not r.primed_neighbours and not r.neighbours
        out[SHAPES[1]] += len(r.primed_neighbours) == 4 or len(r.neighbours) == 4
        out[SHAPES[2]] += t.node1 is not None and t.node1 == t.node2
        out[SHAPES[3]] += t.node1 is not None and t.node1 == t.node2 and t.ind1 == t.ind2
        out[SHAPES[4]] += any(p for _, p in r.primed_neighbours)
        out[SHAPES[6]] += t.isolated and t.bases == read_length
    out[SHAPES[5]] += sum(1 for c in graph.isolated if graph.contigs[c].bases < read_length)
    return out


def table_of(name, step, b, keys, recs, k):
    if step == "raw":
        return FC.raw_table(b.calls, keys, recs["cov"], k)
    return (D if step == "detip" else G).golden(name, "graph").decode()


def compare(check_exe, tmp_path, table, calls, keys, recs, k, read_length, step):
    """the program's file against the restatement's over `table`; (graph, records) of the restatement"""
    plan = FC.run_plan(check_exe, str(tmp_path / "plan.bin"), keys, recs, calls, k, read_length, step)
    assert plan.status == 0
    text, info, graph, rs = FC.expected(table, plan.contigs, calls, k, read_length)
    assert plan.text == text
    assert plan.info == info
    assert [t for t, _, _ in plan.records] == [plan.contigs[r.contig][0] for r in rs]
    tigs = [t[0] for t in plan.contigs]
    assert len(set(tigs)) == len(tigs)                                        # <this> is unique per contig
    return graph, rs


@pytest.fixture(scope="module")
def golden_shapes(check_exe, tmp_path_factory):
    """name -> the shapes its three graphs hold, after the comparison with the restatement; each fixture is compared once per module, whoever asks first"""
    done = {}

    def of(name):
        if name not in done:
            b, keys, recs = build_in(name, "golden")
            fx = _fixture(name)
            k, rl = fx.case.k, fx.max_read_length
            total = collections.Counter()
            for step in FC.STEPS:
                graph, rs = compare(check_exe, tmp_path_factory.mktemp("golden"), table_of(name, step, b, keys, recs, k), b.calls, keys, recs, k, rl, step)
                total += shapes_of(graph, rs, rl)
            done[name] = total
        return done[name]
    return of


@pytest.mark.parametrize("name", NAMES)
def test_the_plan_program_prints_the_restatements_file_of_the_references_tables(golden_shapes, name):
    golden_shapes(name)


def exactly_read_length(check_exe, tmp_path):
    """no golden holds an isolated contig of exactly its read length, so the read length is set to an isolated contig's length, for the program and
    the restatement alike (the raw graph: no step reads it there, only the walk does): (name, table, build, k, that length, the shapes)"""
    name = next(n for n in NAMES if F.Graph(table_of(n, "raw", *build_in(n, "golden"), _fixture(n).case.k)).isolated)
    b, keys, recs = build_in(name, "golden")
    k = _fixture(name).case.k
    table = table_of(name, "raw", b, keys, recs, k)
    g = F.Graph(table)
    exact = g.contigs[g.isolated[0]].bases
    graph, rs = compare(check_exe, tmp_path, table, b.calls, keys, recs, k, exact, "raw")
    return table, (b, keys, recs), k, exact, shapes_of(graph, rs, exact)


def test_an_isolated_contig_of_exactly_read_length_is_printed_and_one_base_less_is_not(check_exe, tmp_path):
    table, (b, keys, recs), k, exact, shapes = exactly_read_length(check_exe, tmp_path)
    assert shapes[SHAPES[6]] >= 1
    graph, rs = compare(check_exe, tmp_path, table, b.calls, keys, recs, k, exact + 1, "raw")
    assert shapes_of(graph, rs, exact + 1)[SHAPES[5]] >= 1 and not any(graph.contigs[r.contig].isolated and graph.contigs[r.contig].bases == exact for r in rs)
    graph, rs = compare(check_exe, tmp_path, table, b.calls, keys, recs, k, -1, "raw")      # (size_t >= int: -1 is the largest size_t, nothing is printed)
    assert not any(graph.contigs[r.contig].isolated for r in rs)


def test_the_fixtures_hold_every_shape(golden_shapes, check_exe, tmp_path):
    total = sum((golden_shapes(name) for name in NAMES), collections.Counter()) + exactly_read_length(check_exe, tmp_path)[4]
    print({s: total[s] for s in SHAPES})
    assert all(total[s] > 0 for s in SHAPES), {s: total[s] for s in SHAPES}


# ---- FGPU_PLAN_UNSET, on a graph changed by hand ----
def s_lines_of(table, graph, c):
    """the numbers of the table's lines that are S lines of contig c, with the key of the node each stands under"""
    out, key = [], None
    for i, ln in enumerate(table.splitlines()):
        f = ln.split()
        if f[0] == "N":
            key = int(f[1], 16)
        elif f[0] == "S" and graph.slots[(key, int(f[1]))] == c:
            out.append((i, key))
    return out


UNSET_ON = (("s3_k8", "dechimera"), ("c1_k21", "detip"), ("j6_k21", "dechimera"), ("twohash_k31_L150__mrl10", "detip"), ("s3_k30", "detip"))


@pytest.mark.parametrize("name, step", UNSET_ON)
def test_where_the_reference_goes_through_a_pointer_that_is_gone_the_plan_says_unset(check_exe, tmp_path, name, step):
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    k, rl = fx.case.k, fx.max_read_length
    table = (D if step == "detip" else G).golden(name, "graph").decode()
    graph = F.Graph(table)
    recs_ref, _ = F.records(graph, rl)
    printed = {r.contig for r in recs_ref}
    # contigs between two distinct nodes, printed, that are somebody's neighbour: the first and the last of them
    fit = [c for c, t in enumerate(graph.contigs) if t.node1 is not None and t.node2 is not None and t.node1 != t.node2 and c in printed and
           any(c in [n for n, _ in r.primed_neighbours + r.neighbours] for r in recs_ref)]
    assert fit, "the fixture holds no such contig"
    run = lambda *change: FC.run_plan(check_exe, str(tmp_path / "p.bin"), keys, recs, b.calls, k, rl, step, change)      # noqa: E731
    assert run().status == 0
    for c in dict.fromkeys((fit[0], fit[-1])):
        t = graph.contigs[c]
        # the contig is deleted where it hangs: a slot holds a pointer to freed memory
        assert run("dead", c).status == 1
        # its ind1 becomes another index: Contig::getSide(node1, the slot it hangs in) finds neither end
        assert run("noend", c).status == 1
        new = (t.ind1 + 1) % 5 if (t.ind1 + 1) % 5 != t.ind2 else (t.ind1 + 2) % 5
        lines = table.splitlines()
        for i, _ in s_lines_of(table, graph, c):
            f = lines[i].split()
            f[3] = str(new)
            lines[i] = " ".join(f)
        with pytest.raises(F.Unset):
            F.records(F.Graph("\n".join(lines) + "\n"), rl)
        # the node at its second end is erased: getNeighbors goes through node2_p
        assert run("gone", c).status == 1
        lines, keep, key = table.splitlines(), [], None
        for ln in lines:
            f = ln.split()
            if f[0] == "N":
                key = int(f[1], 16)
            if f[0] in ("N", "S") and key == t.node2:
                continue
            keep.append(ln)
        with pytest.raises(F.Unset):
            F.records(F.Graph("\n".join(keep) + "\n"), rl)
        # the slot at its first end lets go of it: the walk prints it nowhere, yet it is a neighbour at its second end.  The reference would print
        # its name there; the plan has no record to name and says FGPU_PLAN_INPUT (2) -- no step leaves such a graph, and nothing is guessed
        assert run("nowhere", c).status == 2


def test_records_as_the_library_lays_them_out():
    from faucet_amd import _lib as L
    from faucet_amd import api
    assert api.FASTG_REC_DTYPE.itemsize == 32 and [api.FASTG_REC_DTYPE.fields[n][1] for n in ("tig", "text_word", "cov_sum", "len", "cov_n")] == [0, 8, 16, 24, 28]
    assert C.sizeof(L.FastgInfo) == 32 and api.FASTG_TILE == 4096 and api.FASTG_PRIMED == 1 << 31
    assert all(hasattr(api.Context, n) for n in ("stage3_fastg", "stage3_raw_graph", "stage3_graph_fastg"))
    L.load()                                                                  # (raises if the library lacks a declared symbol)


# ---- the command line on a library without the entry points ----
def test_cli_graph_flags_without_the_entry_points_exit_2_before_any_input(tmp_path):
    """tests/stub/faucet_gpu_stub.cpp answers the C ABI without Stage 3's entry points: each graph flag, alone or mixed with the contig flags, is
    refused with exit code 2 and a message before any input is opened (the inputs named here do not exist) and before anything is written"""
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
    for flags, entry in ((["--raw_graph"], "fgpu_stage3_raw_graph"), (["--detipped_graph"], "fgpu_stage3_graph_fastg"), (["--dechimered_graph"], "fgpu_stage3_graph_fastg"),
                         (["--raw_contigs", "--dechimered_graph"], "fgpu_stage3_"), (["--raw_graph", "--detipped_graph", "--dechimered_graph"], "fgpu_stage3_")):
        r = subprocess.run([exe, "-read_load_file", missing, "-read_scan_file", missing, "-file_prefix", prefix] + flags + c.meta["args"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (flags, r.returncode, r.stderr[-2000:])
        assert "lacks" in r.stderr and entry in r.stderr and r.stderr.startswith(tuple(flags)), (flags, r.stderr[-2000:])      # (the first flag refused says so)
        assert r.stdout == "" and os.listdir(str(tmp_path)) == ["faucet_stub"]


# ---- the compiled reference, asked on the spot ----
@pytest.mark.skipif(not S.chimera_driver_built(), reason="oracle/_ref/faucet_ref and the three Stage-3 drivers were not built (make -C oracle ref)")
@pytest.mark.parametrize("case_id", chimera_cases.SPOT_IDS)
def test_the_plan_program_on_seeded_maps_with_the_drivers_asked_on_the_spot(check_exe, tmp_path, case_id):
    from tests.test_stage3_fuzz_cpu import account_of
    a = account_of(case_id)
    m = a.map
    tables = dict(raw=FC.raw_table(a.build.calls, a.keys, a.recs["cov"], m.k), detip=a.answers.table, dechimera=S.chimera_answers(case_id)[1])
    for step in FC.STEPS:
        compare(check_exe, tmp_path, tables[step], a.build.calls, a.keys, a.recs, m.k, m.max_read_length, step)
