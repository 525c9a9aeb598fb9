"""The device's Stage 3 (faucet_amd/csrc/stage3.hip, stage3_emit.hip, stage3_join.hip, raw_plan.cpp, tips_plan.cpp, build_graph.h) against the
COMPILED REFERENCE on maps made on the spot: the GPU subset of tests/golden/stage3_fuzz_ids.json (tests/stage3_fuzz_cases.py: random runs, tandem
repeats, homopolymer and dinucleotide runs, hairpins, circles, thinned variants; every family, every k, both cleaning settings).  The reference
binaries under oracle/_ref/ (faucet_ref, ref_kat, raw_contigs_driver, detip_driver, chimera_driver) run on this machine's CPUs; nothing is stored.

The ABI, no restatement in between: the reference's .bloom uploaded, its map set in the order its reloaded map iterates in, then
fgpu_stage3_find_neighbors against `ref_kat neighbors`, fgpu_stage3_raw_contigs against the driver's file, fgpu_stage3_detip against the driver's
file and graph table; only `info` is held to the restatement, which tests/test_stage3_fuzz_cpu.py pins to the reference on this very map.
On the 36 ids of tests/chimera_cases.GPU_IDS (that subset and the 24 maps the dechimera step is asked about on the spot, six of them maps on which
validateNoneCollapsible erases a node behind the step): fgpu_stage3_cov_calls over the build where it lies against numpy over the restated build,
then fgpu_stage3_dechimera on the live graph fgpu_stage3_detip left against the chimera driver's file and graph table, its `info` against the
restatement (tests/dechimera_plan_ref.py, pinned to the driver on this very map by tests/test_dechimera_plan_cpu.py); and the two steps twice on one
context.

The command line: `faucet --raw_contigs --detipped_contigs --dechimered_contigs` on the reads of each id and of each unvaried id of those 24 --
.bloom, .junctions and the pair filters byte-equal to faucet_ref's, the three contig files equal to the restatement run in file order over the run's
own outputs, the three summary lines in the order of the steps, the exit code; and on four ids `-gpus 2` under both protocols.  On some of them
validateNoneCollapsible erases a node in file order too.  Children run one after the other, each under a time limit; after one that ended on a
signal or ran into its limit nothing more is started.  Needs an MI355X."""
import json
import os
import subprocess

import pytest

from tests import chimera_cases
from tests import dechimera_golden as G
from tests import stage3_fuzz_cases as S
from tests.test_gpu_dechimera import _flat
from tests.test_gpu_dechimera import device_table as dechimera_table
from tests.test_gpu_detip import device_table
from tests.test_gpu_vs_reference_fuzz import EXE, same_as_the_reference
from tests.test_stage3_fuzz_cpu import GPU_IDS, account_of, dechimered, restated
from tests.test_stage3_walker import REF_KAT, _same_as_reference, _starts, device_of, fixture_from

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (S.binaries_built() and os.path.exists(REF_KAT)),
                                                  reason="oracle/_ref/faucet_ref, ref_kat and the two drivers were not built (make -C oracle ref)")]
chimera_driver = pytest.mark.skipif(not S.chimera_driver_built(), reason="oracle/_ref/chimera_driver was not built (make -C oracle ref)")
CHILD_TIMEOUT = 60
# the command line runs on reads: once per unvaried id of the subset, and of the maps the dechimera step is asked about on the spot
CLI_IDS = list(dict.fromkeys([i.partition("__")[0] for i in GPU_IDS] + [i for i in chimera_cases.SPOT_IDS if "__" not in i]))
CLI_FLAGS = ["--raw_contigs", "--detipped_contigs", "--dechimered_contigs"]
OWN_FILES = (".raw_contigs.fasta", ".detipped_contigs.fasta", ".dechimered_contigs.fasta")
OWN_LINES = ("Raw contigs:", "Detipped contigs:", "Dechimered contigs:")
TWO_RANKS = ("tandem", "hairpin", "paired", "empty")
_builds, _cli, _file_order = {}, {}, {}

# ---- the latch: after a child that crashed or hung nothing more is started ------------------------------------------------------------------
_casualty = []


def _started(what, cmd, **kw):
    """the finished child, under the latch: one that ended on a signal, aborted (134), segfaulted (139) or ran into its time limit fails this
    test and every later one of the module, which start nothing"""
    if _casualty:
        pytest.fail(f"not started: an earlier child of this module crashed or hung -- {_casualty[0]}")
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, errors="replace", timeout=CHILD_TIMEOUT, **kw)
    except subprocess.TimeoutExpired as e:
        _casualty.append(f"{what}: no end after {e.timeout} s")
        pytest.fail(_casualty[0])
    if r.returncode < 0 or r.returncode in (134, 139):
        _casualty.append(f"{what}: ended with {r.returncode}; stderr ends: {r.stderr[-1500:]}")
        pytest.fail(_casualty[0])
    return r


def _chimera(case_id):
    """the chimera driver's two files on an id (CPU), under the latch as _account is"""
    if _casualty:
        pytest.fail(f"not started: an earlier child of this module crashed or hung -- {_casualty[0]}")
    try:
        return S.chimera_answers(case_id)
    except S.NotReturned as e:
        pytest.fail(f"{case_id}: {e}")


def _account(case_id):
    """the reference's answers and the restatement's account (CPU); a listed id on which a reference binary does not return fails"""
    if _casualty:
        pytest.fail(f"not started: an earlier child of this module crashed or hung -- {_casualty[0]}")
    try:
        return account_of(case_id)
    except S.NotReturned as e:
        pytest.fail(f"{case_id}: {e}")


# ---- the ABI against the reference --------------------------------------------------------------------------------------------------------------
def _neighbors(m, tmp_path):
    """`ref_kat neighbors` on a Map: the reference's own findNeighbor for every covered (junction, index)"""
    b, j = str(tmp_path / "v.bloom"), str(tmp_path / "v.junctions")
    m.bloom.tofile(b)
    with open(j, "w") as f:
        f.write("".join(ln + "\n" for ln in m.lines))
    r = _started("ref_kat neighbors", [REF_KAT, "neighbors", b, str(len(m.bloom) * 8 - 1), str(m.n_hash), str(m.k), str(m.j), j, str(m.max_read_length)])
    assert r.returncode == 0, (r.returncode, r.stderr[-500:])
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"kat":"neighbor"')]


def _built(case_id):
    """(context with the id's map set and built, not taken; what fgpu_stage3_build said, kept per id)"""
    a = _account(case_id)
    m = a.map
    ctx = device_of(fixture_from(m.bloom, m.lines, m.k, m.n_hash, m.j, m.max_read_length))
    ctx.stage3_set_junctions(a.keys, a.recs)
    _builds[case_id] = ctx.stage3_build(m.max_read_length, take=False)
    return ctx, _builds[case_id]


@pytest.mark.parametrize("case_id", GPU_IDS)
def test_whole_walks_equal_the_references_findNeighbor(case_id, tmp_path):
    a = _account(case_id)
    m = a.map
    kat = _neighbors(m, tmp_path)
    assert bool(kat) == bool(m.lines)
    if not kat:
        return
    ctx = device_of(fixture_from(m.bloom, m.lines, m.k, m.n_hash, m.j, m.max_read_length))
    ctx.stage3_set_junctions(a.keys, a.recs)
    starts, idx = _starts(kat)
    got, _, contigs = ctx.stage3_find_neighbors(starts, idx, m.max_read_length, contigs=True)
    _same_as_reference(kat, got, contigs)


@pytest.mark.parametrize("case_id", GPU_IDS)
def test_raw_contigs_and_detip_equal_the_references_files(case_id):
    a = _account(case_id)
    m, ans = a.map, a.answers
    ctx, built = _built(case_id)
    assert built["status"] == 0 and built["totals"][0] == len(a.build.calls)
    raw, raw_info = ctx.stage3_raw_contigs(m.max_read_length)
    assert raw == ans.raw_fasta
    assert raw_info == a.raw_info
    detip, info = ctx.stage3_detip(m.max_read_length)
    assert detip == ans.detip_fasta
    assert device_table(ctx, info) == ans.table
    want = a.plan.info
    assert {key: info[key] for key in ("nodes_before", "tips", "back_tips", "validated", "changed")} == \
           {key: want[key] for key in ("nodes_before", "tips", "back_tips", "validated", "changed")}
    assert info["collapsed"] == [want["collapsed_0"], want["collapsed_1"]] and info["degenerate"] == [want["degenerate_0"], want["degenerate_1"]]
    assert {key: info["print"][key] for key in ("records", "bubble_records", "node_contigs", "isolated_kept", "isolated_dropped", "nodes")} == \
           {key: want[key] for key in ("records", "bubble_records", "node_contigs", "isolated_kept", "isolated_dropped", "nodes")}


@chimera_driver
@pytest.mark.parametrize("case_id", chimera_cases.GPU_IDS)
def test_cov_calls_and_dechimera_equal_the_references_files(case_id):
    """the summaries of the build where it lies (k_cov_calls) against numpy over the restated build's whole lists; then the two steps, the second on
    the live graph the first left (CleanGraph::set_cov over every surviving piece list), against the two drivers' files"""
    a = _account(case_id)
    m, ans = a.map, a.answers
    fasta, table = _chimera(case_id)
    ctx, built = _built(case_id)
    assert built["status"] == 0 and built["totals"][0] == len(a.build.calls)
    assert ctx.stage3_cov_calls().tobytes() == G.summaries_of(a.build.calls).tobytes()
    detip, tips = ctx.stage3_detip(m.max_read_length)
    assert detip == ans.detip_fasta
    got, info = ctx.stage3_dechimera()
    assert got == fasta
    assert dechimera_table(ctx, tips["changed"], info) == table
    want = dechimered(a)[1]
    assert {key: _flat(info)[key] for key in G.INFO_KEYS} == {key: want[key] for key in G.INFO_KEYS}
    if case_id in chimera_cases.VALIDATION_IDS:                               # validateNoneCollapsible erased a node on the live graph
        assert info["validated"] and info["collapsed"][1] + info["degenerate"][1] > 0


@chimera_driver
def test_the_two_steps_twice_give_the_same_bytes_twice():
    """detip, dechimera, detip, dechimera on a map whose second step erases nodes: the step mutates the live graph, so the second detip has to make
    a new one from the build, which -- its summaries included -- is what it was"""
    case_id = chimera_cases.VALIDATION_IDS[0]
    a = _account(case_id)
    fasta = _chimera(case_id)[0]
    ctx, _ = _built(case_id)
    summaries = ctx.stage3_cov_calls().tobytes()
    first = ctx.stage3_detip(a.map.max_read_length), ctx.stage3_dechimera()
    again = ctx.stage3_detip(a.map.max_read_length), ctx.stage3_dechimera()
    assert first == again and first[0][0] == a.answers.detip_fasta and first[1][0] == fasta
    assert first[1][1]["collapsed"][1] + first[1][1]["degenerate"][1] > 0
    assert ctx.stage3_cov_calls().tobytes() == summaries


def test_some_build_takes_more_than_one_round():
    """the device builds by rounds of walks made at once and made again where an earlier call changed the map under them: a subset whose builds
    all end in their first round would not have run that path at all; nor one on which no round outgrew its array and was run again (ten of
    the subset's builds did when the list was made)"""
    infos = {i: _builds[i] if i in _builds else _built(i)[1] for i in GPU_IDS}
    assert max(b["rounds"] for b in infos.values()) > 1, {i: b["rounds"] for i, b in infos.items()}
    assert max(b["regrown"] for b in infos.values()) >= 1, {i: b["regrown"] for i, b in infos.items()}
    print("rounds", {i: b["rounds"] for i, b in infos.items()}, "regrown", {i: b["regrown"] for i, b in infos.items() if b["regrown"]})


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------
def _cli_run(case_id, tmp_path, tag, extra=(), env=None):
    path, args = S.case_of(case_id)[:2]
    d = tmp_path / tag
    d.mkdir()
    r = _started(f"faucet on {case_id} {list(extra)} {env or ''}",
                 ["stdbuf", "-o0", EXE, "-read_load_file", path, "-read_scan_file", path, "-file_prefix", str(d / "out")] + args + CLI_FLAGS + list(extra),
                 env=dict(os.environ, **(env or {})))
    return r, d


def _line(stdout, head):
    lines = [ln for ln in stdout.split("\n") if ln.startswith(head)]
    assert len(lines) == 1, (head, lines)
    return lines[0]


@pytest.mark.parametrize("case_id", CLI_IDS)
def test_cli_against_faucet_ref_and_the_restatement_in_file_order(case_id, tmp_path):
    _account(case_id)
    path, args, ref_dir = S.case_of(case_id)[:3]
    r, d = _cli_run(case_id, tmp_path, "one")
    same_as_the_reference(S.reference_stdout(case_id), ref_dir, r, d, args, own_files=OWN_FILES, own_lines=OWN_LINES)
    assert r.returncode == (0 if "--no_cleaning" in args else 3)
    m = S.map_from(str(d), r.stdout, args)
    fx = fixture_from(m.bloom, m.lines, m.k, m.n_hash, m.j, m.max_read_length)
    want = restated(m, None, order=fx.keys)                                  # the restatement in FILE order over the run's own outputs
    assert (d / "out.raw_contigs.fasta").read_bytes() == want.raw
    assert (d / "out.detipped_contigs.fasta").read_bytes() == want.detip
    chimera, ci = dechimered(want)
    _file_order[case_id] = ci["collapsed_1"] + ci["degenerate_1"]
    assert (d / "out.dechimered_contigs.fasta").read_bytes() == chimera
    ri, ti = want.raw_info, want.plan.info
    assert _line(r.stdout, "Raw contigs:").startswith("Raw contigs: %d records (%d bubble, %d off nodes, %d isolated; %d isolated below" % (
        ri["records"], ri["bubble_records"], ri["node_contigs"], ri["isolated_kept"], ri["isolated_dropped"]))
    assert _line(r.stdout, "Detipped contigs:").startswith("Detipped contigs: %d tips deleted (and %d back tips), %d of %d nodes left, %d records" % (
        ti["tips"], ti["back_tips"], ti["nodes"], ti["nodes_before"], ti["records"]))
    assert _line(r.stdout, "Dechimered contigs:") == "Dechimered contigs: %d chimeric extensions removed, %d of %d nodes left, %d records" % (
        ci["removed"], ci["nodes"], ci["nodes_before"], ci["records"])
    assert r.stdout.index("Raw contigs:") < r.stdout.index("Detipped contigs:") < r.stdout.index("Dechimered contigs:")     # in the order of the steps


def test_some_cli_id_has_a_validation_that_erases_a_node_in_file_order():
    """the command line builds in FILE order, where other cuts fall than in the reloaded map's: on some of its ids validateNoneCollapsible has
    to erase a node behind the step all the same, and the two-rank runs' tandem pick is one of them.  Counted by the restatement over the
    reference's files, which the run's own equal byte for byte (the test above); ids that test has come through are not restated again"""
    for case_id in CLI_IDS:
        if case_id not in _file_order:
            _account(case_id)
            args, ref_dir = S.case_of(case_id)[1:3]
            m = S.map_from(ref_dir, S.reference_stdout(case_id), args)
            ci = dechimered(restated(m, None, order=fixture_from(m.bloom, m.lines, m.k, m.n_hash, m.j, m.max_read_length).keys))[1]
            _file_order[case_id] = ci["collapsed_1"] + ci["degenerate_1"]
    erasing = {i: _file_order[i] for i in CLI_IDS if _file_order[i]}
    print("validation erases nodes in file order on", erasing)
    assert erasing
    assert _two_ranks_id("tandem") in erasing


def _two_ranks_id(which):
    for i in CLI_IDS:
        if which in ("tandem", "hairpin"):
            if S.split(i)[0] == which:
                return i
        elif which == "paired":
            if S.split(i)[0] == "rand" and "--paired_ends" in S.case_of(i)[1]:
                return i
        elif not S.case_of(i)[3].lines:
            return i
    pytest.fail(f"the GPU tests' subset holds no id for {which!r}")


@pytest.mark.parametrize("protocol", ["shards", "slices"])
@pytest.mark.parametrize("which", TWO_RANKS)
def test_cli_with_two_ranks_writes_the_one_device_runs_files(which, protocol, tmp_path):
    """-gpus 2 (both ranks on the one device) under either FAUCET_SHARD_PROTOCOL: every file, the three contig files included, and the three
    summary lines are the one-device run's"""
    case_id = _two_ranks_id(which)
    _account(case_id)
    args = S.case_of(case_id)[1]
    if case_id not in _cli:
        _cli[case_id] = _cli_run(case_id, tmp_path, "one")
        r, d = _cli[case_id]
        _cli[case_id] = (r, {f: (d / f).read_bytes() for f in os.listdir(d)})
    one, files = _cli[case_id]
    two, d2 = _cli_run(case_id, tmp_path, "two", ["-gpus", "2"], env={"FAUCET_SHARD_PROTOCOL": "slices"} if protocol == "slices" else None)
    assert two.returncode == one.returncode == (0 if "--no_cleaning" in args else 3), two.stdout[-2000:] + two.stderr[-3000:]
    assert sorted(os.listdir(d2)) == sorted(files) and all(f"out{e}" in files for e in OWN_FILES)
    for f, data in files.items():
        assert (d2 / f).read_bytes() == data, f
    for head in OWN_LINES:
        assert _line(two.stdout, head) == _line(one.stdout, head)
