"""fgpu_chimera_plan (faucet_amd/csrc/tips_plan.cpp over clean_graph.h: ContigGraph::deleteTipsAndClean, removeChimerasAndClean and printContigs
behind them, over piece lists and coverage summaries) against the compiled reference's own files after the two steps
(tests/golden/dechimera_<name>.fasta.gz and .graph.gz, made by tests/golden/make_chimera_golden.py), byte for byte: the plan is compiled with a
main of its own (tests/host/chimera_plan_check.cpp) under -fsanitize=address,undefined as a stand-alone program and run over the build
tests/graph_build_ref.py gives with the map in the order the reference's reloaded map iterated in.  tests/dechimera_plan_ref.py, the same step
restated in plain Python over whole coverage lists, writes the same files and gives the same account.  The summary operations of
faucet_amd/csrc/cov_summary.h, through the same program, against what the compiled reference's ContigJuncList made of the hand-made lists
(tests/golden/join_concat.json.gz).  fgpu_tips_plan, now a few lines over the same header, against the detip goldens through the library.  Where
oracle/_ref is built, the compiled reference (oracle/_ref/chimera_driver) is asked on the spot about 24 seeded maps (tests/chimera_cases.py).  No GPU.

The LIVE graph: fgpu_stage3_dechimera does not run fgpu_chimera_plan -- it works on the CleanGraph fgpu_stage3_detip left, which was built without
summaries, detipped, serialised, and only then given the summaries by CleanGraph::set_cov, a fold over every surviving piece list.  The same program's
`live` mode does just that, in that order, under the same sanitizers: its output has to be `plan`'s byte for byte on the goldens, the seeded orders and
the 24 seeded maps (where it also has to write the driver's two files), and every summary of a live contig (S lines: right behind set_cov, and behind
the step) has to be that of the coverage list tests/detip_ref.join makes of the contig's piece list from the calls' whole lists.  The inputs are
counted to be able to tell: contigs with a flipped piece that reads differently backwards, long lists; what set_cov refuses is asked through mode
arguments of the program.

FGPU_PLAN_UNSET: among the 28 goldens, the 18 variants the reference does not return on (it stops in buildContigGraph on all of them, before
either step) and the 67 seeded maps there is none on which the compiled reference aborts INSIDE this step, so the status is checked on a map
changed by hand into what the step cannot go through -- a covered slot without a contig, where the reference calls a method on a null pointer
-- and on the seeded map orders, against the restatement."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import chimera_cases
from tests import dechimera_golden as G
from tests import dechimera_plan_ref as R
from tests import detip_golden as D
from tests import detip_ref as J
from tests import raw_contigs_ref as P
from tests import stage3_fuzz_cases as S
from tests.golden_util import Case
from tests.join_cases import cases
from tests.test_contig_ref_cpu import UNVARIED
from tests.test_graph_build_ref_cpu import ORDERS
from tests.test_join_ref_cpu import KS
from tests.test_join_ref_cpu import golden as join_golden
from tests.test_raw_contigs_ref_cpu import build_in
from tests.test_stage3_walker import _fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(G.summary()["fixtures"])
REQUIRED = ("cut_near", "cut_far", "cut_both", "collapse_right_behind_a_cut", "collapse_of_a_node_met_with_one_path", "skipped_p_in_slot_4",
            "skipped_p_not_the_far_nodes_lowest", "skipped_ratio_below_3", "nothing_removed_file_is_the_detip_golden")


def test_the_goldens_are_the_set_the_script_asks_for():
    s = G.summary()
    assert NAMES == sorted(D.summary()["fixtures"]) and len(NAMES) == 28 and sorted(s["not_returned"]) == sorted(D.summary()["not_returned"])
    assert all(s["reached"][key] for key in REQUIRED)
    assert s["not_reached"] == ["validation_erases_a_node"] and not s["reached"]["validation_erases_a_node"] and chimera_cases.VALIDATION_IDS
    # what the compiled reference printed on the 13 unvaried fixtures
    assert [s["fixtures"][n]["reference_removed"] for n in UNVARIED] == [11, 3, 0, 17, 17, 8, 1, 1, 3, 5, 1, 14, 0], UNVARIED
    for n in s["reached"]["nothing_removed_file_is_the_detip_golden"]:
        assert G.golden(n, "fasta") == D.golden(n, "fasta") and G.golden(n, "graph").decode().splitlines()[0].endswith(" 0")


def restated(calls, keys, recs, k, read_length):
    return R.plan(calls, keys, recs["cov"], k, read_length)


def tips_part(info):
    return {key: info[key] for key in G.TIPS_KEYS}


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_writes_the_references_file_and_graph(name):
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    nodes, contigs, records, info, tips_info, averages = restated(b.calls, keys, recs, fx.case.k, fx.max_read_length)
    fasta, table = G.files_of(nodes, contigs, records, info, tips_info["changed"], b.calls, fx.case.k)
    assert fasta == G.golden(name, "fasta")
    assert table == G.golden(name, "graph").decode()                          # (its last line: the counts the reference printed)
    want = G.summary()["fixtures"][name]
    assert (info["removed"], info["nodes"], info["collapsed_1"] + info["degenerate_1"] if info["validated"] else -1) == \
        (want["reference_removed"], want["reference_nodes"], want["reference_validation"])
    # the averages the restatement decided on, from whole lists, are the table's, from the lists joined again
    joined = J.join(D.triples_of(b.calls), [t[6] for t in contigs], fx.case.k) if contigs else []
    assert ["%.17g" % a for a in averages] == ["%.17g" % j[3] for j in joined]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return G.compile_check(str(tmp_path_factory.mktemp("chimera_plan") / "chimera_plan_check"), sanitize=True)


def run(plan_exe, tmp_path, b, keys, recs, k, read_length, covs=None, contigs=None, calls=None, cap=G.NO_LIMIT, mode=("plan",)):
    c, cl, _ = P.arrays_of(b.calls)
    return G.run_check(plan_exe, str(tmp_path / "plan.bin"), keys, recs, c if contigs is None else contigs, cl if calls is None else calls,
                       G.summaries_of(b.calls) if covs is None else covs, k, read_length, cap, mode)


@pytest.mark.parametrize("name", NAMES)
def test_the_plan_program_writes_the_references_file_and_graph(plan_exe, tmp_path, name):
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    assert b.status == 0
    plan = run(plan_exe, tmp_path, b, keys, recs, fx.case.k, fx.max_read_length)
    assert plan.status == 0 and plan.sizing == (3 if any(plan.sizes) else 0)
    assert plan.sizes == [len(plan.nodes), len(plan.contigs), sum(len(t[6]) for t in plan.contigs), len(plan.records), sum(len(p) for _, p in plan.records)]
    fasta, table = G.files_of_plan(plan, b.calls, fx.case.k)
    assert fasta == G.golden(name, "fasta")
    assert table == G.golden(name, "graph").decode()
    want = G.summary()["fixtures"][name]
    assert {key: want[key] for key in G.INFO_KEYS} == plan.info
    nodes, contigs, records, info, tips_info, _ = restated(b.calls, keys, recs, fx.case.k, fx.max_read_length)
    assert (plan.nodes, plan.contigs, plan.records, plan.info, plan.tips_info) == (nodes, contigs, records, info, tips_part(tips_info))
    assert plan.tips_info == tips_part(D.summary()["fixtures"][name])         # the first step's account is the detip goldens'
    assert plan.info["removed"] == plan.info["cut_near"] + plan.info["cut_far"] + plan.info["cut_both"]
    used = [c for t in plan.contigs for c, _ in t[6]]
    assert len(used) == len(set(used))                                        # a call lies in one contig of the graph left


@pytest.mark.parametrize("name, order", [(name, o) for name in UNVARIED for o in ORDERS[1:]])
def test_the_plan_program_and_the_library_against_the_restatement_on_seeded_orders(plan_exe, tmp_path, name, order):
    """other orders of the same maps, where the loops meet the nodes in another order (no reference file: the reloaded map has the one order)"""
    from faucet_amd import api
    b, keys, recs = build_in(name, order)
    fx = _fixture(name)
    contigs, calls, _ = P.arrays_of(b.calls)
    covs = G.summaries_of(b.calls)
    plan = run(plan_exe, tmp_path, b, keys, recs, fx.case.k, fx.max_read_length)
    status, graph, records, info, tips_info = api.chimera_plan(keys, recs, contigs, calls, covs, fx.case.k, fx.max_read_length)
    assert status == plan.status
    try:
        want = restated(b.calls, keys, recs, fx.case.k, fx.max_read_length)
    except (R.Unset, P.UnsetContig, P.NotABuild) as e:
        assert status == (2 if isinstance(e, P.NotABuild) else 1) and graph is None
        return
    assert status == 0 and (plan.nodes, plan.contigs, plan.records, plan.info, plan.tips_info) == (*want[:4], tips_part(want[4]))
    assert records == plan.records and graph["lists"] == [t[6] for t in plan.contigs]
    assert [(int(n["key"]), [int(v) for v in n["cov"]], [int(v) for v in n["slot"]]) for n in graph["nodes"]] == plan.nodes
    flat = dict(info, collapsed_0=info["collapsed"][0], collapsed_1=info["collapsed"][1], degenerate_0=info["degenerate"][0], degenerate_1=info["degenerate"][1],
                **{"skipped_%d" % i: v for i, v in enumerate(info["skipped"])}, **info["print"])
    assert {key: flat[key] for key in G.INFO_KEYS} == plan.info
    G.files_of_plan(plan, b.calls, fx.case.k)                                  # the lists join, to the lengths the plan says


def test_the_plan_program_on_short_room_on_arrays_that_are_no_build_and_where_the_reference_cannot_go_on(plan_exe, tmp_path):
    name = "s3_k8"
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    k, mrl = fx.case.k, fx.max_read_length
    contigs, calls, _ = P.arrays_of(b.calls)
    covs = G.summaries_of(b.calls)
    full = run(plan_exe, tmp_path, b, keys, recs, k, mrl)
    assert full.status == 0 and min(full.sizes[1:]) > 1 and full.info["removed"] and full.info["skipped_5"]
    for cap in (0, 1, min(full.sizes[1:]) - 1, max(full.sizes) - 1):           # room for too little: the sizes and both accounts all the same
        short = run(plan_exe, tmp_path, b, keys, recs, k, mrl, cap=cap)
        assert short.status == 3 and short.sizes == full.sizes and short.info == full.info and short.tips_info == full.tips_info
    empty = G.run_check(plan_exe, str(tmp_path / "e.bin"), keys[:0], recs[:0], contigs[:0], calls[:0], covs[:0], k, mrl)
    assert (empty.sizing, empty.status, empty.sizes) == (0, 0, [0] * 5) and not any(empty.info.values())
    bad = contigs.copy()
    bad["ind2"][0] = 5
    assert run(plan_exe, tmp_path, b, keys, recs, k, mrl, contigs=bad).status == 2     # no build: an index outside 0..4
    none = covs.copy()
    none[len(none) // 2] = (0, 0, 0, 0, (0, 0))
    assert run(plan_exe, tmp_path, b, keys, recs, k, mrl, covs=none).status == 2       # a contig without a coverage entry: nothing is guessed
    # ---- FGPU_PLAN_UNSET (the module's docstring says why these are made by hand)
    # a node with two paths out gets a third coverage, on a slot no call filled: getMinMaxForwardExtensions calls otherEndNode on a null contig
    order, _, _ = P.graph_of(b.calls, keys, recs["cov"], k)
    nodes = dict(order)
    row = next(i for i, key in enumerate(keys) if int(key) in nodes and sum(v > 0 for v in nodes[int(key)].cov) == 2 and
               any(v == 0 and c is None for v, c in zip(nodes[int(key)].cov, nodes[int(key)].contigs[:4])))
    covered = recs.copy()
    slot = next(i for i in range(4) if nodes[int(keys[row])].cov[i] == 0 and nodes[int(keys[row])].contigs[i] is None)
    covered["cov"][row][slot] = 9
    assert run(plan_exe, tmp_path, b, keys, covered, k, mrl).status == 1
    # with no read length nothing is a tip, and with all coverages equal no ratio reaches 3: the step goes through every node and removes nothing
    flat = covs.copy()
    flat["sum"], flat["first"], flat["last"] = flat["n"] * 7, 7, 7
    calm = run(plan_exe, tmp_path, b, keys, recs, k, 0, covs=flat)
    assert calm.status == 0 and calm.info["removed"] == 0 and calm.tips_info["tips"] == 0 and calm.info["nodes"] == calm.info["nodes_before"]
    assert calm.info["skipped_4"] > 0 and calm.info["skipped_5"] == 0


# ---- the live graph: the device's path (of_build without summaries, detip, the first step's records, set_cov, the step) as a program ----
def summary_of(cov):
    return (sum(cov), len(cov), cov[0], cov[-1])


def live_and_plan(plan_exe, tmp_path, b, keys, recs, k, read_length):
    """(`live`'s output, `plan`'s) over one build, after the two checks every input gets: live's output without its S lines IS plan's, byte for
    byte (status, sizes, both accounts, the N, C and P lines), and every S line -- right behind set_cov over the list it stands beside, behind
    the step over the contig record of its number -- is the summary of the coverage list tests/detip_ref.join makes of that piece list from
    the calls' WHOLE lists"""
    plan = run(plan_exe, tmp_path, b, keys, recs, k, read_length)
    lv = run(plan_exe, tmp_path, b, keys, recs, k, read_length, mode=("live",))
    assert lv.text == plan.text and lv.refused is None
    if plan.status != 0:
        assert not lv.s
        return lv, plan
    triples = D.triples_of(b.calls)
    before = J.join(triples, [pl for _, pl in lv.s0], k) if lv.s0 else []
    assert [s for s, _ in lv.s0] == [summary_of(j[2]) for j in before]
    after = J.join(triples, [t[6] for t in lv.contigs], k) if lv.contigs else []
    assert lv.s == [summary_of(j[2]) for j in after]
    # a contig the step left alone is the same list with the same summary before and behind it
    was = {tuple(pl): s for s, pl in lv.s0}
    assert all(was[tuple(t[6])] == s for t, s in zip(lv.contigs, lv.s) if tuple(t[6]) in was)
    return lv, plan


def telling(lv, calls):
    """(contigs of the graph the step left that have more than one piece and hold a flipped piece whose own summary has n >= 2 and first != last --
    the ones a fold that forgets to reverse gets wrong --, the longest piece list, lists with a single-entry piece, ... with one not at an end, and
    the first count again over the lists set_cov folded: the detipped graph, ahead of the step)"""
    covs = G.summaries_of(calls)
    asym = lambda c: int(covs[c]["n"]) >= 2 and int(covs[c]["first"]) != int(covs[c]["last"])      # noqa: E731
    lists = [t[6] for t in lv.contigs]
    single = [pl for pl in lists if len(pl) > 1 and any(int(covs[c]["n"]) == 1 for c, _ in pl)]
    return (sum(1 for pl in lists if len(pl) > 1 and any(fl and asym(c) for c, fl in pl)), max(map(len, lists), default=0), len(single),
            sum(1 for pl in single if any(int(covs[c]["n"]) == 1 for c, _ in pl[1:-1])),
            sum(1 for _, pl in lv.s0 if len(pl) > 1 and any(fl and asym(c) for c, fl in pl)))


_told = {}


@pytest.mark.parametrize("name", NAMES)
def test_the_live_graph_gives_the_plans_output_and_folds_every_summary_right(plan_exe, tmp_path, name):
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    lv, plan = live_and_plan(plan_exe, tmp_path, b, keys, recs, fx.case.k, fx.max_read_length)
    assert lv.status == 0 and G.files_of_plan(lv, b.calls, fx.case.k) == (G.golden(name, "fasta"), G.golden(name, "graph").decode())
    _told[name] = telling(lv, b.calls)


def test_the_goldens_can_tell_a_wrong_fold(plan_exe, tmp_path):
    """a fold that is wrong in first, last or sum shows in an S line only on a list with a flipped piece that reads differently backwards: the
    goldens hold at least 100 such contigs behind the step (160 when this was written) and a list of at least 20 pieces (29)"""
    for name in NAMES:
        if name not in _told:
            b, keys, recs = build_in(name, "golden")
            fx = _fixture(name)
            _told[name] = telling(run(plan_exe, tmp_path, b, keys, recs, fx.case.k, fx.max_read_length, mode=("live",)), b.calls)
    flipped, longest, single, interior, folded = (f([_told[n][i] for n in NAMES]) for i, f in enumerate((sum, max, sum, sum, sum)))
    print("contigs with a flipped asymmetric piece", flipped, "longest list", longest, "lists with a single-entry piece", single, "interior", interior,
          "flipped asymmetric when set_cov folded", folded, "fixtures without one", [n for n in NAMES if not _told[n][4]])
    assert flipped >= 100 and longest >= 20, (flipped, longest)


@pytest.mark.parametrize("name, order", [(name, o) for name in UNVARIED for o in ORDERS[1:]])
def test_the_live_graph_on_seeded_orders(plan_exe, tmp_path, name, order):
    b, keys, recs = build_in(name, order)
    fx = _fixture(name)
    live_and_plan(plan_exe, tmp_path, b, keys, recs, fx.case.k, fx.max_read_length)


def test_the_live_graph_refuses_what_it_cannot_fold(plan_exe, tmp_path):
    name = "s3_k8"
    b, keys, recs = build_in(name, "golden")
    fx = _fixture(name)
    k, mrl = fx.case.k, fx.max_read_length
    full = run(plan_exe, tmp_path, b, keys, recs, k, mrl, mode=("live",))
    assert full.status == 0 and full.info["removed"] and full.s and any(len(t[6]) > 1 for t in full.contigs)
    # removeChimerasAndClean on a graph that was never given summaries: FGPU_PLAN_INPUT (2)
    never = run(plan_exe, tmp_path, b, keys, recs, k, mrl, mode=("live", "no_summaries"))
    assert never.refused == ["2"] and never.status == 2 and not any(never.info.values()) and not never.s0 and not never.s
    # set_cov with one summary of no entries: FGPU_PLAN_INPUT, the graph still without summaries -- and nothing was written: the right summaries
    # behind it give what they give alone, S lines included
    zero = run(plan_exe, tmp_path, b, keys, recs, k, mrl, mode=("live", "zero_entries"))
    assert zero.refused == ["2", "have_cov", "0"]
    assert (zero.text, zero.s0, zero.s) == (full.text, full.s0, full.s)
    # set_cov with n_calls one short of a call some list names: FGPU_PLAN_INPUT, the graph still without summaries
    short = run(plan_exe, tmp_path, b, keys, recs, k, mrl, mode=("live", "short_calls"))
    assert short.refused == ["2", "have_cov", "0", "named", "1"] and short.status == 2 and not short.s0 and not short.s


def test_tips_plan_through_the_library_still_writes_the_detip_goldens():
    """the refactor: fgpu_tips_plan over clean_graph.h gives what it gave (tests/test_detip_plan_cpu.py holds the stand-alone program to the same)"""
    from faucet_amd import api
    for name in NAMES:
        b, keys, recs = build_in(name, "golden")
        fx = _fixture(name)
        contigs, calls, _ = P.arrays_of(b.calls)
        status, graph, records, info = api.tips_plan(keys, recs, contigs, calls, fx.case.k, fx.max_read_length)
        assert status == 0
        plan = D.Plan("sizing 0\nstatus 0\nsizes\ninfo\n")
        plan.nodes = [(int(n["key"]), [int(v) for v in n["cov"]], [int(v) for v in n["slot"]]) for n in graph["nodes"]]
        plan.contigs = [(int(t["node1"]) if t["has1"] else None, int(t["node2"]) if t["has2"] else None, int(t["len"]), int(t["ind1"]), int(t["ind2"]),
                         int(t["isolated"]), pl) for t, pl in zip(graph["contigs"], graph["lists"])]
        plan.records = records
        plan.info = dict(tips=info["tips"], nodes=info["print"]["nodes"], validated=info["validated"], changed=info["changed"],
                         collapsed_1=info["collapsed"][1], degenerate_1=info["degenerate"][1])
        fasta, table = D.files_of_plan(plan, b.calls, fx.case.k)
        assert fasta == D.golden(name, "fasta") and table == D.golden(name, "graph").decode(), name
        want = D.summary()["fixtures"][name]
        assert (info["back_tips"], info["collapsed"][0], info["degenerate"][0], info["print"]["records"]) == \
            (want["back_tips"], want["collapsed_0"], want["degenerate_0"], want["records"])


# ---- the summary operation against the compiled reference's ContigJuncList ----
@pytest.mark.parametrize("k", KS)
def test_folded_summaries_equal_the_references_joined_coverage_lists(plan_exe, tmp_path, k):
    t = cases(k)
    stored = {g["name"]: g for g in join_golden(k)}
    pieces_of = [[(fl, t.contigs[c][2]) for c, fl in pl] for pl in t.lists]
    got = G.run_fold(plan_exe, str(tmp_path / "fold.txt"), [("L", p) for p in pieces_of])
    assert len(got) == len(t.names) == len(stored)
    for name, g in zip(t.names, got):
        cov = stored[name]["cov"]
        assert g == (sum(cov), len(cov), cov[0], cov[-1], stored[name]["avg"]), name
    # three pieces with a single-entry middle piece: the minimum runs over three entries, and the other bracketing gives the same
    three = [i for i, p in enumerate(pieces_of) if len(p) == 3 and len(p[1][1]) == 1]
    assert three
    back = G.run_fold(plan_exe, str(tmp_path / "fold.txt"), [("R", pieces_of[i]) for i in three])
    assert back == [got[i] for i in three]
    every = G.run_fold(plan_exe, str(tmp_path / "fold.txt"), [("R", p) for p in pieces_of])
    assert every == got                                                        # ... and so does every other list: the operation is associative


def test_records_as_the_library_lays_them_out():
    from faucet_amd import _lib as L
    from faucet_amd import api
    assert api.COV_SUMMARY_DTYPE.itemsize == 16 and [api.COV_SUMMARY_DTYPE.fields[n][1] for n in ("sum", "n", "first", "last")] == [0, 8, 12, 13]
    assert C.sizeof(L.ChimeraInfo) == 184 and L.ChimeraInfo.print.offset == 136
    assert hasattr(api.Context, "stage3_cov_calls") and hasattr(api.Context, "stage3_dechimera") and hasattr(api, "chimera_plan")


# ---- the command line on a library without the entry points ----
def test_cli_dechimered_contigs_without_the_entry_points_exits_2_before_any_input(tmp_path):
    """tests/stub/faucet_gpu_stub.cpp answers the C ABI without Stage 3's entry points: --dechimered_contigs, alone or with the two other flags in any
    order, is refused with exit code 2 and a message before any input is opened (the inputs named here do not exist) and before anything is written"""
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
    for flags in (["--dechimered_contigs"], ["--dechimered_contigs", "--detipped_contigs"], ["--raw_contigs", "--dechimered_contigs"]):
        r = subprocess.run([exe, "-read_load_file", missing, "-read_scan_file", missing, "-file_prefix", prefix] + flags + c.meta["args"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
        assert "lacks" in r.stderr and "fgpu_stage3_" in r.stderr
        assert r.stdout == "" and os.listdir(str(tmp_path)) == ["faucet_stub"]
    r = subprocess.run([exe, "-read_load_file", missing, "-read_scan_file", missing, "-file_prefix", prefix, "--dechimered_contigs"] + c.meta["args"],
                       capture_output=True, text=True, timeout=120)
    assert "--dechimered_contigs" in r.stderr and "fgpu_stage3_dechimera" in r.stderr


# ---- the compiled reference, asked on the spot ----
driver_built = pytest.mark.skipif(not os.path.exists(S.CHIMERA_DRIVER), reason="oracle/_ref/chimera_driver was not built (make -C oracle ref)")


@driver_built
def test_the_compiled_reference_asked_on_the_spot_about_seeded_maps(plan_exe, tmp_path):
    """24 maps none of this was written against (tests/chimera_cases.py): oracle/_ref/chimera_driver is asked here and now, and the restatement and the
    plan program have to write its files; the ids on which the validation behind the step erases a node say so in the reference's own count line"""
    from tests.test_stage3_fuzz_cpu import account_of
    erased = []
    for case_id in chimera_cases.SPOT_IDS:
        a = account_of(case_id)
        m = a.map
        fasta, table = S.chimera_answers(case_id)
        nodes, contigs, records, info, tips_info, _ = restated(a.build.calls, a.keys, a.recs, m.k, m.max_read_length)
        assert G.files_of(nodes, contigs, records, info, tips_info["changed"], a.build.calls, m.k) == (fasta, table), case_id
        plan = run(plan_exe, tmp_path, a.build, a.keys, a.recs, m.k, m.max_read_length)
        assert plan.status == 0 and G.files_of_plan(plan, a.build.calls, m.k) == (fasta, table), case_id
        assert (plan.nodes, plan.contigs, plan.records, plan.info) == (nodes, contigs, records, info), case_id
        if int(table.splitlines()[-1].split()[3]) > 0:
            erased.append(case_id)
    assert erased == chimera_cases.VALIDATION_IDS


@pytest.mark.skipif(not S.chimera_driver_built(), reason="oracle/_ref/faucet_ref and the three Stage-3 drivers were not built (make -C oracle ref)")
@pytest.mark.parametrize("case_id", chimera_cases.SPOT_IDS)
def test_the_live_graph_writes_the_references_files_on_seeded_maps(plan_exe, tmp_path, case_id):
    """the device's path on the maps where it is hardest: on the VALIDATION_IDS the validation behind the step erases a node ON THE LIVE GRAPH,
    as many as the reference's own count line says, and each of them holds at least 20 contigs that can tell a wrong fold (22 to 188 when this was
    written)"""
    from tests.test_stage3_fuzz_cpu import account_of
    a = account_of(case_id)
    m = a.map
    lv, plan = live_and_plan(plan_exe, tmp_path, a.build, a.keys, a.recs, m.k, m.max_read_length)
    fasta, table = S.chimera_answers(case_id)
    assert lv.status == 0 and G.files_of_plan(lv, a.build.calls, m.k) == (fasta, table)
    told = telling(lv, a.build.calls)
    print(case_id, "contigs with a flipped asymmetric piece", told[0], "longest list", told[1], "lists with a single-entry piece", told[2], "interior", told[3],
          "flipped asymmetric when set_cov folded", told[4])
    if case_id in chimera_cases.VALIDATION_IDS:
        erased = lv.info["collapsed_1"] + lv.info["degenerate_1"]
        assert lv.info["validated"] and erased > 0 and erased == int(table.splitlines()[-1].split()[3])
        assert told[0] >= 20, told
    if case_id == chimera_cases.LONGEST_LIST_ID:
        assert told[1] >= 20, told                                             # (37 pieces when this was written)
