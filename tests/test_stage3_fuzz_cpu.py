"""The restatements of the reference's Stage 3 (tests/graph_build_ref.py, raw_contigs_ref.py, detip_plan_ref.py) and the host-only plans
(fgpu_raw_plan, fgpu_tips_plan as stand-alone programs under -fsanitize=address,undefined) against the COMPILED REFERENCE on maps none of them
was written against: the ids of tests/golden/stage3_fuzz_ids.json (tests/stage3_fuzz_cases.py: random runs, tandem repeats, homopolymer and
dinucleotide runs, hairpins, circles, and thinned variants of them).  Per id `faucet_ref` writes .bloom and .junctions, oracle/_ref/raw_contigs_driver
and detip_driver say what the reference's buildContigGraph, printContigs and deleteTipsAndClean make of them, and the restatements, run over the
host walker with the oracle's probes in the order the driver's order file gives, have to write the same bytes: the raw FASTA, the FASTA after the
step, the graph table with its counts line.  Every listed id must return -- one that does not fails, it is never skipped.  No GPU; skipped
where oracle/_ref was not built (make -C oracle ref)."""
import collections

import pytest

from tests import detip_golden as D
from tests import detip_plan_ref as R
from tests import raw_contigs_ref as P
from tests import stage3_fuzz_cases as S
from tests.contig_ref import paths_out, print_kmer
from tests.test_detip_plan_cpu import plan_exe as tips_plan_exe  # noqa: F401  (fixtures: the two check programs, built once per module)
from tests.test_graph_build_ref_cpu import Finder
from tests.test_raw_contigs_ref_cpu import _run_plan, build_over
from tests.test_raw_contigs_ref_cpu import plan_exe as raw_plan_exe  # noqa: F401
from tests.test_stage3_walker import fixture_from

pytestmark = pytest.mark.skipif(not S.binaries_built(), reason="oracle/_ref/faucet_ref, raw_contigs_driver, detip_driver are built where the reference "
                                "tree is mounted (make -C oracle ref)")
IDS, GPU_IDS = S.listed()["ids"], S.listed()["gpu_ids"]
CLASSES = ("even_k", "k_8", "empty_map", "far_is_start", "own_reverse_complement", "homopolymer_start", "joined_bubble_record", "isolated_kept",
           "isolated_dropped", "back_tip", "every_node_goes", "three_pieces", "below_32", "above_32", "below_64", "above_64")
OPTIONAL = ("over_255",)       # a distance list of more than 255 entries or a distance over 255: asserted only to be what the list file says
Account = collections.namedtuple("Account", "map answers build keys recs raw raw_info plan detip table")
_accounts = {}


def account_of(case_id):
    """the reference's answers on an id and the restatements' over the same map in the same order; made once, shared, left unchanged"""
    if case_id not in _accounts:
        m, ans = S.case_of(case_id)[3:]
        _accounts[case_id] = restated(m, ans)
    return _accounts[case_id]


def restated(m, ans, order=None):
    """the restatements over a Map with its junctions in the order of the keys `order` (default: the order the reference's reloaded map
    iterated in, ans.order; `ans` may be None where another order is given)"""
    fx = fixture_from(m.bloom, m.lines, m.k, m.n_hash, m.j, m.max_read_length)
    b, keys, recs = build_over(Finder(fx, fx.keys, fx.recs), ans.order if order is None else order, m.k)
    assert b.status == 0, b.status                          # the reference's own buildContigGraph returned on this map
    raw, raw_info, _ = P.raw_contigs(b.calls, keys, recs["cov"], m.k, m.max_read_length)
    plan = D.Plan("sizing 0\nstatus 0\nsizes\ninfo\n")
    plan.nodes, plan.contigs, plan.records, plan.info = R.plan(b.calls, keys, recs["cov"], m.k, m.max_read_length)
    detip, table = D.files_of_plan(plan, b.calls, m.k)
    return Account(m, ans, b, keys, recs, raw, raw_info, plan, detip, table)


def dechimered(a):
    """the restatement of the next step, removeChimerasAndClean (tests/dechimera_plan_ref.py), over an Account's build in the Account's order: (the
    file after the two steps, the step's account over tests/dechimera_golden.INFO_KEYS and more); not part of the Account, so that only who asks
    pays for it"""
    from tests import dechimera_plan_ref
    from tests import detip_ref
    records, info = dechimera_plan_ref.plan(a.build.calls, a.keys, a.recs["cov"], a.map.k, a.map.max_read_length)[2:4]
    return D.fasta_of(records, detip_ref.join(D.triples_of(a.build.calls), [p for _, p in records], a.map.k) if records else []), info


def classes_of(a):
    """the classes of the module's docstring an id reaches, from the reference's own files and the restatement's account of the map"""
    seqs = a.answers.raw_fasta.decode().split("\n")[1::2]
    rc = lambda s: s.translate(str.maketrans("ACGT", "TGCA"))[::-1]      # noqa: E731
    out = dict(
        even_k=a.map.k % 2 == 0, k_8=a.map.k == 8, empty_map=not a.map.lines,
        far_is_start=any(w.far_is_start for w in a.build.calls),
        own_reverse_complement=any(s == rc(s) for s in seqs),
        # faucet_amd/csrc/build_graph.h:97 (utils/JunctionMap.cpp:43-47): a complex junction whose k-mer is one base k times
        homopolymer_start=any(paths_out([int(v) for v in c]) > 1 and len(set(print_kmer(int(x), a.map.k))) == 1 for x, c in zip(a.keys, a.recs["cov"])),
        joined_bubble_record=any(len(p) > 2 for _, p in a.plan.records[:a.plan.info["bubble_records"]]),
        isolated_kept=a.raw_info["isolated_kept"] > 0, isolated_dropped=a.raw_info["isolated_dropped"] > 0,
        back_tip=a.plan.info["back_tips"] > 0,
        every_node_goes=a.plan.info["nodes_before"] > 0 and a.plan.info["nodes"] == 0,
        three_pieces=any(len(t[6]) >= 3 for t in a.plan.contigs),
        below_32=any(len(s) < 32 for s in seqs), above_32=any(len(s) > 32 for s in seqs),
        below_64=any(len(s) < 64 for s in seqs), above_64=any(len(s) > 64 for s in seqs),
        over_255=any(len(w.contig.distances) > 255 or max(w.contig.distances, default=0) > 255 for w in a.build.calls))
    return sorted(key for key, v in out.items() if v)


@pytest.mark.parametrize("case_id", IDS)
def test_the_restatements_write_the_references_files(case_id):
    a = account_of(case_id)
    assert a.raw == a.answers.raw_fasta
    assert a.detip == a.answers.detip_fasta
    assert a.table == a.answers.table


@pytest.mark.parametrize("case_id", IDS)
def test_the_plan_programs_write_the_references_files(raw_plan_exe, tips_plan_exe, tmp_path, case_id):  # noqa: F811
    a = account_of(case_id)
    m = a.map
    contigs, calls, _ = P.arrays_of(a.build.calls)
    records, info = P.plan(a.build.calls, a.keys, a.recs["cov"], m.k, m.max_read_length)
    status, n, counts, lines = _run_plan(raw_plan_exe, str(tmp_path / "raw.bin"), a.keys, a.recs, contigs, calls, m.k, m.max_read_length, len(contigs))
    assert (status, n) == (0, len(records))
    assert counts == [info[key] for key in ("records", "bubble_records", "node_contigs", "isolated_kept", "isolated_dropped", "nodes")]
    assert lines == P.plan_lines(records, contigs)
    assert P.fasta_of([r.number for r in records], P.strings_of(records, a.build.calls, m.k)) == a.answers.raw_fasta
    plan = D.run_check(tips_plan_exe, str(tmp_path / "tips.bin"), a.keys, a.recs, contigs, calls, m.k, m.max_read_length)
    assert plan.status == 0 and plan.sizing == (3 if any(plan.sizes) else 0)
    fasta, table = D.files_of_plan(plan, a.build.calls, m.k)
    assert fasta == a.answers.detip_fasta
    assert table == a.answers.table
    assert (plan.nodes, plan.contigs, plan.records, plan.info) == (a.plan.nodes, a.plan.contigs, a.plan.records, a.plan.info)


def test_the_list_is_the_one_the_script_asks_for():
    """about 60 ids of every family, the candidates the reference did not return on beside them with the reason, at most a tenth of the maps
    empty; and the GPU tests' subset: every family, every k, both cleaning settings, at least four variants"""
    s = S.listed()
    assert 50 <= len(IDS) <= 70 and len(set(IDS)) == len(IDS) and not set(s["rejected"]) & set(IDS) and all(s["rejected"].values())
    assert {S.split(i)[0] for i in IDS} == set(S.FAMILIES) and {S.split(i)[2] for i in IDS} == {None, *S.KINDS}
    empty = [i for i in IDS if not account_of(i).map.lines]
    assert 1 <= len(empty) <= len(IDS) // 10, empty
    assert 20 <= len(GPU_IDS) <= 28 and set(GPU_IDS) <= set(IDS)
    assert {S.split(i)[0] for i in GPU_IDS} == set(S.FAMILIES) and sum(1 for i in GPU_IDS if S.split(i)[2]) >= 4
    assert {account_of(i).map.k for i in GPU_IDS} == {account_of(i).map.k for i in IDS} >= set(S.LOW_K)
    assert {"--no_cleaning" in S.case_of(i)[1] for i in GPU_IDS} == {True, False}


def test_the_list_reaches_every_class():
    """each class at least once, in the whole list and in the GPU tests' subset, counted again from the reference's files of today and equal to
    what the list file says"""
    reached = {cl: [i for i in IDS if cl in classes_of(account_of(i))] for cl in CLASSES + OPTIONAL}
    assert reached == S.listed()["reached"]
    assert all(reached[cl] for cl in CLASSES), [cl for cl in CLASSES if not reached[cl]]
    assert all(set(reached[cl]) & set(GPU_IDS) for cl in CLASSES), [cl for cl in CLASSES if not set(reached[cl]) & set(GPU_IDS)]
