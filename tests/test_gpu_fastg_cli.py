"""`faucet --raw_graph --detipped_graph --dechimered_graph` on the reads of a handful of the seeded ids of tests/stage3_fuzz_cases.py: with all six
Stage-3 flags together and with each graph flag alone.  The FASTG files have to be what tests/fastg_ref.py prints from the graph tables of the
restatements run in FILE order over the run's own .junctions and .bloom (the command line builds in file order; tests/test_stage3_fuzz_cpu.py and
test_dechimera_plan_cpu.py pin those restatements to the compiled reference), <this> renumbered by first appearance on both sides; the contig
files have to be those of a run without the graph flags; printGraph's four lines stand together, ahead of the line of the same stage's contig
file, as src/Faucet.cpp:313-314 and :325-326 order the two calls.  Needs an MI355X and oracle/_ref (faucet_ref makes the reads' arguments)."""
import os

import pytest

from tests import dechimera_golden as G
from tests import dechimera_plan_ref as R2
from tests import fastg_cases as FC
from tests import fastg_ref as F
from tests import stage3_fuzz_cases as S
from tests.test_gpu_fastg import expected_of, raw_lists
from tests.test_gpu_stage3_fuzz import _account, _started
from tests.test_gpu_vs_reference_fuzz import EXE
from tests.test_stage3_fuzz_cpu import restated
from tests.test_stage3_walker import REF_KAT, fixture_from

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (S.binaries_built() and os.path.exists(REF_KAT)),
                                                  reason="oracle/_ref/faucet_ref, ref_kat and the two drivers were not built (make -C oracle ref)")]
IDS = ("rand-101", "tandem-0", "runs-1", "hairpin-0", "runs-3")           # isolated contigs on both sides of the read length; loops; an empty map
CONTIG_FLAGS = ["--raw_contigs", "--detipped_contigs", "--dechimered_contigs"]
GRAPH_FLAGS = ["--raw_graph", "--detipped_graph", "--dechimered_graph"]
STAGES = ("raw", "detipped", "dechimered")
CONTIG_LINES = ("Raw contigs:", "Detipped contigs:", "Dechimered contigs:")


def _run(case_id, tmp_path, tag, flags):
    path, args = S.case_of(case_id)[:2]
    d = tmp_path / tag
    d.mkdir()
    r = _started(f"faucet on {case_id} {flags}", ["stdbuf", "-o0", EXE, "-read_load_file", path, "-read_scan_file", path, "-file_prefix", str(d / "out")] + args + flags)
    assert r.returncode == (0 if "--no_cleaning" in args else 3), r.stdout[-2000:] + r.stderr[-3000:]
    return r, d


def _expected(d, stdout, args):
    """per stage (renumbered bytes, info) from the restatements in file order over the run's own outputs"""
    m = S.map_from(str(d), stdout, args)
    fx = fixture_from(m.bloom, m.lines, m.k, m.n_hash, m.j, m.max_read_length)
    want = restated(m, None, order=fx.keys)
    calls, cov, k, rl = want.build.calls, want.recs["cov"], m.k, m.max_read_length
    nodes, contigs, records, info, tips_info, _ = R2.plan(calls, want.keys, cov, k, rl)
    tables = dict(raw=FC.raw_table(calls, want.keys, cov, k), detipped=want.table, dechimered=G.files_of(nodes, contigs, records, info, tips_info["changed"], calls, k)[1])
    lists = dict(raw=raw_lists(calls, want.keys, cov, k), detipped=[t[6] for t in want.plan.contigs], dechimered=[t[6] for t in contigs])
    return {stage: expected_of(tables[stage], lists[stage], calls, k, rl) for stage in STAGES}


def _graph_blocks(stdout):
    """printGraph's four lines, block by block, and the line numbers they begin at"""
    lines = stdout.split("\n")
    at = [i for i, ln in enumerate(lines) if ln == "Printing unitig FASTG."]
    return [lines[i:i + 4] for i in at], at, lines


@pytest.mark.parametrize("case_id", IDS)
def test_cli_graph_flags_together_and_alone(case_id, tmp_path):
    from tests.test_gpu_fastg import renumbered
    _account(case_id)
    args = S.case_of(case_id)[1]
    plain, dp = _run(case_id, tmp_path, "contigs", CONTIG_FLAGS)
    six, d6 = _run(case_id, tmp_path, "six", CONTIG_FLAGS + GRAPH_FLAGS)
    want = _expected(d6, six.stdout, args)
    assert sorted(os.listdir(d6)) == sorted(os.listdir(dp) + ["out.%s_graph.fastg" % s for s in STAGES])
    for f in os.listdir(dp):                                                  # every other file, the three contig files among them, is the plain run's
        assert (d6 / f).read_bytes() == (dp / f).read_bytes(), f
    files = {s: (d6 / ("out.%s_graph.fastg" % s)).read_bytes() for s in STAGES}
    for s in STAGES:
        assert renumbered(files[s]) == want[s][0], s
    blocks, at, lines = _graph_blocks(six.stdout)
    assert blocks == [F.stdout_lines(want[s][1]) for s in STAGES]
    for i, head in zip(at, CONTIG_LINES):                                     # the graph is printed ahead of the same stage's contigs
        assert lines[i + 4].startswith(head), lines[i:i + 5]
    assert "Printing unitig FASTG." not in plain.stdout
    for s, flag in zip(STAGES, GRAPH_FLAGS):
        r, d = _run(case_id, tmp_path, s, [flag])
        assert sorted(f for f in os.listdir(d) if f.endswith((".fasta", ".fastg"))) == ["out.%s_graph.fastg" % s]
        assert (d / ("out.%s_graph.fastg" % s)).read_bytes() == files[s]
        assert _graph_blocks(r.stdout)[0] == [F.stdout_lines(want[s][1])] and not any(head in r.stdout for head in CONTIG_LINES)


def test_cli_dechimered_graph_against_the_references_own_final_fastg(tmp_path):
    """`faucet_ref` run from the goldens' reads WITH cleaning writes <prefix>.cleaned_graph_unitigs.fastg; where its final graph is its dechimered
    graph (tests/fastg_cases.reference_final_graph: decided from reference data only), `faucet --dechimered_graph` on the same reads with the same
    arguments has to write that graph.  Both files come from maps in orders of their own and name contigs by numbers of their own, so they are
    compared as tests/fastg_ref.halves makes them comparable: every header/sequence half as (own (length, coverage text), the neighbours'
    (length, coverage text), sequence), as multisets.  The command line's whole path -- junction order, build, both steps, the device's emitter --
    against a file the reference itself wrote."""
    qualified, left = [], {}
    for name in FC.golden_reads():
        why, reads, args, text, _, _ = FC.reference_final_graph(name, tmp_path / name)
        if why:
            left.setdefault(why, []).append(name)
            continue
        d = tmp_path / name / "cli"
        d.mkdir()
        r = _started(f"faucet --dechimered_graph on {name}", ["stdbuf", "-o0", EXE, "-read_load_file", reads, "-read_scan_file", reads, "-file_prefix", str(d / "out")] +
                     args + ["--dechimered_graph"])
        assert r.returncode == 3, (name, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])      # (cleaning asked for, which this program does not do)
        got = (d / "out.dechimered_graph.fastg").read_bytes()
        assert F.halves(got) == F.halves(text), name
        qualified.append((name, got.count(b"\n") // 4))
    print("qualified", qualified, "left out", left)
    assert len(qualified) >= 4, (qualified, left)


def test_cli_help_lists_the_graph_flags():
    r = _started("faucet --help", [EXE, "--help"])
    assert all(flag in r.stdout + r.stderr for flag in GRAPH_FLAGS)
