"""ContigGraph::removeChimerasAndClean on the device's build (faucet_amd/csrc/clean_graph.h, stage3_emit.hip, stage3_join.hip):
fgpu_stage3_cov_calls -- the coverage summaries the step reads, k_cov_calls -- on hand-made contigs against numpy and on a build left on the
device; fgpu_stage3_dechimera on every golden fixture against the compiled reference's own file and graph after the two steps
(tests/golden/dechimera_<name>.fasta.gz, .graph.gz), with the map in the order the reference's map iterated in, and the states it refuses;
`faucet --dechimered_contigs`.  Needs an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import dechimera_golden as G
from tests import detip_golden as D
from tests import raw_contigs_ref as P
from tests.golden_util import Case
from tests.test_gpu_raw_contigs import _take_build
from tests.test_raw_contigs_ref_cpu import golden_build
from tests.test_stage3_walker import _device, _fixture

pytestmark = pytest.mark.gpu
NAMES = sorted(G.summary()["fixtures"])
LENGTHS = (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4097)


def test_the_goldens_are_there():
    assert len(NAMES) == 28 and NAMES == sorted(D.summary()["fixtures"])


# ---- fgpu_stage3_cov_calls ----
def _by_numpy(contigs, cov):
    from faucet_amd import api
    out = np.zeros(len(contigs), dtype=api.COV_SUMMARY_DTYPE)
    for i, c in enumerate(contigs):
        v = cov[int(c["cov_first"]):int(c["cov_first"]) + int(c["n_cov"])]
        out[i] = (int(v.sum(dtype=np.uint64)), len(v), int(v[0]) if len(v) else 0, int(v[-1]) if len(v) else 0, (0, 0))
    return out


def _hand_made(n, seed, lengths=None):
    """n contig records over one coverage array, the lists one behind the other with a few unused bytes between them; lengths: the first lists'"""
    from faucet_amd import api
    rng = np.random.default_rng(seed)
    sizes = list(lengths or []) + [int(v) for v in rng.integers(1, 6, size=n)]
    sizes = sizes[:n]
    contigs = np.zeros(n, dtype=api.CONTIG_DTYPE)
    at, parts = 0, []
    for i, m in enumerate(sizes):
        gap = int(rng.integers(0, 3))
        parts.append(np.full(gap, 0x5A, dtype=np.uint8))
        v = rng.integers(0, 256, size=m).astype(np.uint8)
        if i % 3 == 0:
            v[rng.integers(0, m)] = 255
        if i % 3 == 1:
            v[rng.integers(0, m)] = 0
        parts.append(v)
        contigs["cov_first"][i], contigs["n_cov"][i] = at + gap, m
        at += gap + m
    return contigs, np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def test_cov_calls_of_hand_made_lists_against_numpy():
    ctx = _device("c1_k21")
    contigs, cov = _hand_made(len(LENGTHS) + 40, 31, LENGTHS)
    assert [int(v) for v in contigs["n_cov"][:len(LENGTHS)]] == list(LENGTHS)
    for fill in (0, 255):                                                      # whole lists of the two extreme values: 4097 x 255 is no byte sum
        flat = cov.copy()
        flat[:] = fill
        got = ctx.stage3_cov_calls(contigs, flat)
        assert got.tobytes() == _by_numpy(contigs, flat).tobytes()
        assert int(got["sum"][len(LENGTHS) - 1]) == 4097 * fill
    got = ctx.stage3_cov_calls(contigs, cov)
    want = _by_numpy(contigs, cov)
    assert got.tobytes() == want.tobytes() and 0 in cov and 255 in cov
    order = np.random.default_rng(32).permutation(len(contigs))                # records in another order than their lists lie in
    assert ctx.stage3_cov_calls(contigs[order], cov).tobytes() == want[order].tobytes()
    same = contigs[[3, 3, 11, 3]]                                              # records may share entries
    assert ctx.stage3_cov_calls(same, cov).tobytes() == want[[3, 3, 11, 3]].tobytes()
    none = contigs[:5].copy()
    none["n_cov"][2] = 0                                                       # a record of no entries: (0, 0, 0, 0)
    got = ctx.stage3_cov_calls(none, cov)
    assert got.tobytes() == _by_numpy(none, cov).tobytes() and got[2].tobytes() == bytes(16)
    none["cov_first"][2] = len(cov)                                            # ... even at the array's end
    assert ctx.stage3_cov_calls(none, cov)[2].tobytes() == bytes(16)


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257))
def test_cov_calls_at_the_block_and_lane_group_edges(n):
    """four lanes per record, 64 records per block: the last group of a block, the first of the next, a block of one group"""
    ctx = _device("c1_k21")
    contigs, cov = _hand_made(n, 40 + n, (9, 1, 4097)[:n])
    got = ctx.stage3_cov_calls(contigs, cov)
    assert len(got) == n and got.tobytes() == _by_numpy(contigs, cov).tobytes()


def test_cov_calls_argument_errors():
    from faucet_amd import _lib as L
    from faucet_amd import api
    ctx = _device("j8_k23")                                                    # (a context of its own: no build may lie on it)
    ctx.stage3_set_junctions(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=api.JUNC_DTYPE))
    ctx.stage3_build(100)                                                      # ... taken
    contigs, cov = _hand_made(70, 51)
    out = np.full(len(contigs), 0x5A, dtype=np.uint8).repeat(16).view(api.COV_SUMMARY_DTYPE)
    untouched = out.tobytes()

    def call(c=contigs, n=None, v=cov, nv=None, o=out):
        return ctx.lib.fgpu_stage3_cov_calls(ctx.h, None if c is None else c.ctypes.data, (0 if c is None else len(c)) if n is None else n,
                                             None if v is None else v.ctypes.data, (0 if v is None else len(v)) if nv is None else nv, None if o is None else o.ctypes.data)
    for field, value in (("cov_first", len(cov) + 1), ("n_cov", len(cov) + 1), ("cov_first", 1 << 40), ("n_cov", 0xFFFFFFFF)):
        bad = contigs.copy()
        bad[field][69] = value
        assert call(c=bad) == L.ERR_ARG and b"fgpu_stage3_cov_calls" in ctx.lib.fgpu_last_error(ctx.h) and b"69" in ctx.lib.fgpu_last_error(ctx.h), (field, value)
    last = contigs.copy()
    last["n_cov"][69] += 1                                                     # one entry past the array's end
    assert int(last["cov_first"][69]) + int(last["n_cov"][69]) == len(cov) + 1 and call(c=last) == L.ERR_ARG
    assert call(v=cov[:-1]) == L.ERR_ARG                                       # the array ends before the last list does
    assert call(v=None, nv=len(cov)) == L.ERR_ARG and call(o=None) == L.ERR_ARG and call(v=None) == L.ERR_ARG
    assert out.tobytes() == untouched                                          # nothing was launched, nothing written
    assert call(c=None, v=None) == L.ERR_STATE                                 # no build whose calls could be meant
    assert call(c=None, n=3, v=None) == L.ERR_ARG and call(c=None, v=cov) == L.ERR_ARG and call(c=None, v=None, nv=4) == L.ERR_ARG
    assert out.tobytes() == untouched
    assert call() == L.OK and out.tobytes() == _by_numpy(contigs, cov).tobytes()
    assert call(c=contigs[:0], v=None) == L.OK and call(c=contigs[:0], o=None) == L.OK      # no records: nothing to do


def test_cov_calls_over_the_build_left_on_the_device():
    name = "s3_k8"
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    out, calls, text, kmers, dist, cov, info = ctx.stage3_build(fx.max_read_length, raw=True)
    assert info["status"] == 0 and len(out) == len(b.calls) > 64
    from faucet_amd import _lib as L
    totals = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert ctx.lib.fgpu_stage3_build_totals(ctx.h, totals) == L.ERR_STATE and list(totals) == [0, 0, 0, 0]      # taken: no build to speak of
    built = dict(totals=[0, 0, 0, 0])
    bt = (C.c_uint64 * 4)()
    assert ctx.lib.fgpu_stage3_build(ctx.h, fx.max_read_length, bt, None) == L.OK       # a build made past the Python class: the room is the library's own count
    built["totals"] = [int(v) for v in bt]
    assert ctx.lib.fgpu_stage3_build_totals(ctx.h, totals) == L.OK and list(totals) == built["totals"] and totals[0] == len(out)
    on_device = ctx.stage3_cov_calls()
    assert on_device.tobytes() == ctx.stage3_cov_calls(out, cov).tobytes() == _by_numpy(out, cov).tobytes() == G.summaries_of(b.calls).tobytes()
    kept = _take_build(ctx, built["totals"])                                   # the build is still there, and unchanged
    assert all(a.tobytes() == f.tobytes() for a, f in zip(kept, (out, calls, text, kmers, dist, cov)))


# ---- fgpu_stage3_dechimera ----
def device_table(ctx, tips_changed, info):
    """the graph table with its counts line (tests/dechimera_golden.py) of the graph fgpu_stage3_dechimera left, taken with fgpu_stage3_graph_take:
    its contigs' bases and coverages by a join over the build where it lies"""
    graph = ctx.stage3_graph_take()
    joined = ctx.stage3_join(graph["lists"]) if graph["lists"] else (np.zeros(0), [], [], [], [])
    assert [len(s) for s in joined[1]] == [int(v) for v in graph["contigs"]["len"]]
    nodes = [(int(n["key"]), [int(v) for v in n["cov"]], [int(v) for v in n["slot"]]) for n in graph["nodes"]]
    contigs = [(int(t["node1"]) if t["has1"] else None, int(t["node2"]) if t["has2"] else None, int(t["len"]), int(t["ind1"]), int(t["ind2"]), int(t["isolated"]))
               for t in graph["contigs"]]
    flat = dict(changed=info["changed"], removed=info["removed"], nodes=info["print"]["nodes"], validated=info["validated"], collapsed_1=info["collapsed"][1],
                degenerate_1=info["degenerate"][1])
    return G.table_of(nodes, contigs, [(len(s), float(a)) for s, a in zip(joined[1], joined[4])], tips_changed, flat)


def _flat(info):
    return dict(info, collapsed_0=info["collapsed"][0], collapsed_1=info["collapsed"][1], degenerate_0=info["degenerate"][0], degenerate_1=info["degenerate"][1],
                **{"skipped_%d" % i: v for i, v in enumerate(info["skipped"])}, **info["print"])


@pytest.mark.parametrize("name", NAMES)
def test_dechimera_equals_the_references_file_and_graph(name):
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    want = G.summary()["fixtures"][name]
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    built = ctx.stage3_build(fx.max_read_length, take=False)
    assert built["status"] == 0 and built["totals"][0] == len(b.calls)
    detipped, tips = ctx.stage3_detip(fx.max_read_length)
    assert detipped == D.golden(name, "fasta")
    got, info = ctx.stage3_dechimera()
    assert got == G.golden(name, "fasta")
    assert {key: _flat(info)[key] for key in G.INFO_KEYS} == {key: want[key] for key in G.INFO_KEYS}
    assert device_table(ctx, tips["changed"], info) == G.golden(name, "graph").decode()
    with pytest.raises(RuntimeError):                                          # taken: nothing left
        ctx.stage3_graph_take()
    # the build and the first step's results are what they were: detip again gives the detip file and graph again, and the build is unchanged
    again, tips2 = ctx.stage3_detip(fx.max_read_length)
    assert again == detipped and tips2 == tips
    from tests.test_gpu_detip import device_table as detip_table
    assert detip_table(ctx, tips2) == D.golden(name, "graph").decode()
    kept = _take_build(ctx, built["totals"])
    fresh = ctx.stage3_build(fx.max_read_length, raw=True)
    assert all(a.tobytes() == f.tobytes() for a, f in zip(kept, fresh[:6]))


def test_dechimera_leaves_the_joined_records_to_be_taken():
    """fgpu_stage3_join_take behind the call: the strings, distances and coverages of the print records, as a join of the plan's lists gives them"""
    from faucet_amd import _lib as L
    from faucet_amd import api
    name = "j6_k21"
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    ctx.stage3_build(fx.max_read_length, take=False)
    ctx.stage3_detip(fx.max_read_length)
    nbytes, ci = C.c_uint64(0), L.ChimeraInfo()
    assert ctx.lib.fgpu_stage3_dechimera(ctx.h, C.byref(nbytes), C.byref(ci)) == 0 and nbytes.value == len(G.golden(name, "fasta"))
    status, _, records, _, _ = api.chimera_plan(keys, recs, *P.arrays_of(b.calls)[:2], G.summaries_of(b.calls), fx.case.k, fx.max_read_length)
    assert status == 0 and records
    from tests import detip_ref as J
    want = J.join(D.triples_of(b.calls), [p for _, p in records], fx.case.k)
    words = sum((len(w[0]) + 31) // 32 for w in want)
    jt, jd, jc = np.zeros(words, dtype=np.uint64), np.zeros(sum(len(w[1]) for w in want), dtype=np.uint8), np.zeros(sum(len(w[2]) for w in want), dtype=np.uint8)
    assert ctx.lib.fgpu_stage3_join_take(ctx.h, jt.ctypes.data, len(jt), jd.ctypes.data, len(jd), jc.ctypes.data, len(jc)) == 0
    assert jd.tolist() == [v for w in want for v in w[1]] and jc.tolist() == [v for w in want for v in w[2]]
    assert ctx.stage3_fasta_take(nbytes.value) == G.golden(name, "fasta")


def test_dechimera_needs_the_live_graph_of_a_detip_and_runs_once():
    from faucet_amd import _lib as L
    name = "c1_k21"
    keys, recs = golden_build(name)[1:3]
    fx = _fixture(name)
    ctx = _device(name)
    nbytes, ci = C.c_uint64(7), L.ChimeraInfo()

    def call():
        nbytes.value = 7
        return ctx.lib.fgpu_stage3_dechimera(ctx.h, C.byref(nbytes), C.byref(ci))
    from tests.test_stage3_walker import device_of
    fresh = device_of(fx)                                                       # a context that has never been detipped: a build on the device, no graph
    fresh.stage3_set_junctions(keys, recs)
    fresh.stage3_build(fx.max_read_length, take=False)
    nbytes.value = 7
    assert fresh.lib.fgpu_stage3_dechimera(fresh.h, C.byref(nbytes), C.byref(ci)) == L.ERR_STATE and nbytes.value == 0
    assert b"fgpu_stage3_dechimera" in fresh.lib.fgpu_last_error(fresh.h) and b"fgpu_stage3_detip" in fresh.lib.fgpu_last_error(fresh.h)
    assert not any(_flat(ci.as_dict())[key] for key in G.INFO_KEYS)
    assert fresh.stage3_detip(fx.max_read_length)[0] == D.golden(name, "fasta")  # ... and nothing of the context was touched: the two steps run
    assert fresh.stage3_dechimera()[0] == G.golden(name, "fasta")
    fresh.close()
    ctx.stage3_set_junctions(keys, recs)
    ctx.stage3_build(fx.max_read_length, take=False)
    ctx.stage3_detip(fx.max_read_length)
    ctx.stage3_graph_take()
    assert call() == L.ERR_STATE and nbytes.value == 0 and b"fgpu_stage3_dechimera" in ctx.lib.fgpu_last_error(ctx.h)      # the graph was taken
    ctx.stage3_detip(fx.max_read_length)
    got, info = ctx.stage3_dechimera()
    assert got == G.golden(name, "fasta") and info["removed"] == 11
    assert call() == L.ERR_STATE and b"has run" in ctx.lib.fgpu_last_error(ctx.h)              # the step has run on that graph
    assert ctx.stage3_graph_take()["lists"]                                     # ... which is still there to be taken
    ctx.stage3_detip(fx.max_read_length)
    ctx.stage3_build(fx.max_read_length, take=False)                            # another build: the graph is of one that is gone
    assert call() == L.ERR_STATE and b"build" in ctx.lib.fgpu_last_error(ctx.h)
    ctx.stage3_detip(fx.max_read_length)
    assert ctx.stage3_dechimera()[0] == got
    assert ctx.lib.fgpu_stage3_dechimera(ctx.h, None, C.byref(ci)) == L.ERR_ARG
    ctx.stage3_set_junctions(keys[:0], recs[:0])                                # an empty map
    ctx.stage3_build(fx.max_read_length, take=False)
    assert ctx.stage3_detip(fx.max_read_length)[0] == b""
    got, info = ctx.stage3_dechimera()
    assert got == b"" and info["removed"] == info["nodes_before"] == info["print"]["records"] == 0 and ctx.stage3_graph_take()["lists"] == []


# ---- the command line ----
def _plan_over(cwd, c):
    """the restatements in FILE order over the run's own .junctions and .bloom: tests/graph_build_ref.py's build with the oracle answering the probes,
    tests/dechimera_plan_ref.py's plan over it (which tests/test_dechimera_plan_cpu.py pins to the compiled reference's own files), tests/detip_ref.join's
    text: (the file after the two steps, the step's info, the file after the first, the raw file)"""
    from tests import dechimera_plan_ref as R
    from tests import detip_plan_ref as R1
    from tests import detip_ref as J
    from tests import graph_build_ref as GB
    from tests.test_graph_build_ref_cpu import Finder
    from tests.test_stage3_walker import Fixture, _map_of
    with open(os.path.join(cwd, "out.junctions")) as f:
        lines = f.read().split("\n")[:-1]
    bloom = np.fromfile(os.path.join(cwd, "out.bloom"), dtype=np.uint8)
    keys, recs = _map_of(lines)
    fx = Fixture(c, bloom, keys, recs, c.max_read_length, None, lines)
    f = Finder(fx, keys, recs)
    b = GB.build_contig_graph(lambda alive, km, ix: f.find(np.asarray(alive, dtype=bool), km, ix), keys, recs["cov"], c.k)
    assert b.status == 0
    triples = D.triples_of(b.calls)

    def file_of(records):
        return D.fasta_of(records, J.join(triples, [p for _, p in records], c.k) if records else [])
    records, info = R.plan(b.calls, keys, recs["cov"], c.k, c.max_read_length)[2:4]
    detipped = R1.plan(b.calls, keys, recs["cov"], c.k, c.max_read_length)[2]
    return file_of(records), info, file_of(detipped), P.raw_contigs(b.calls, keys, recs["cov"], c.k, c.max_read_length)[0]


@pytest.mark.parametrize("name", ["c1_k21", "twohash_k31_L150"])
def test_cli_dechimered_contigs(name, tmp_path):
    """`faucet --dechimered_contigs` writes <prefix>.dechimered_contigs.fasta behind the scan outputs, alone and behind the two other Stage-3 files;
    every other output file, and the exit code, are those of a run without the flag"""
    from tests.test_gpu_estimate_stream import output_files, written_input
    from tests.test_gpu_scan_kept_cli import run
    c = Case(name)
    inp = written_input(c, tmp_path)
    args = ["-read_load_file", inp, "-read_scan_file", inp] + c.meta["args"]
    plain, alone, three = str(tmp_path / "plain"), str(tmp_path / "alone"), str(tmp_path / "three")
    g = run(plain, args)
    r = run(alone, args + ["--dechimered_contigs"])
    r3 = run(three, args + ["--dechimered_contigs", "--raw_contigs", "--detipped_contigs"])
    assert r.returncode == r3.returncode == g.returncode == (0 if c.no_cleaning else 3), r.stdout[-2000:] + r.stderr[-3000:]
    for ext in output_files(c):
        for cwd in (alone, three):
            with open(os.path.join(plain, "out." + ext), "rb") as a, open(os.path.join(cwd, "out." + ext), "rb") as b:
                assert a.read() == b.read(), ext
    assert sorted(os.listdir(alone)) == sorted(os.listdir(plain) + ["out.dechimered_contigs.fasta"])
    assert sorted(os.listdir(three)) == sorted(os.listdir(plain) + ["out.dechimered_contigs.fasta", "out.detipped_contigs.fasta", "out.raw_contigs.fasta"])
    want, info, detipped, raw = _plan_over(alone, c)
    for cwd in (alone, three):
        with open(os.path.join(cwd, "out.dechimered_contigs.fasta"), "rb") as f:
            assert f.read() == want
    with open(os.path.join(three, "out.detipped_contigs.fasta"), "rb") as f:
        assert f.read() == detipped
    with open(os.path.join(three, "out.raw_contigs.fasta"), "rb") as f:
        assert f.read() == raw
    line = [ln for ln in r.stdout.split("\n") if ln.startswith("Dechimered contigs:")]
    assert line == ["Dechimered contigs: %d chimeric extensions removed, %d of %d nodes left, %d records" % (info["removed"], info["nodes"], info["nodes_before"], info["records"])]
    assert "Dechimered contigs:" not in g.stdout and "Raw contigs:" not in r.stdout and "Detipped contigs:" not in r.stdout
    assert r3.stdout.index("Raw contigs:") < r3.stdout.index("Detipped contigs:") < r3.stdout.index("Dechimered contigs:")     # the files in the order of the steps
    assert [ln for ln in r3.stdout.split("\n") if ln.startswith("Dechimered contigs:")] == line


@pytest.mark.parametrize("protocol", ["shards", "slices"])
def test_cli_dechimered_contigs_with_two_ranks(protocol, tmp_path):
    """-gpus 2 (both ranks on the one device): the last rank's context holds the merged map and the whole bloo2 after either protocol -- the
    file, and the junctions it was built on, are the one-device run's"""
    from tests.test_gpu_estimate_stream import written_input
    from tests.test_gpu_scan_kept_cli import run
    c = Case("c1_k21")
    inp = written_input(c, tmp_path)
    args = ["-read_load_file", inp, "-read_scan_file", inp] + c.meta["args"] + ["--dechimered_contigs"]
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    g = run(one, args)
    r = run(two, args + ["-gpus", "2"], env={"FAUCET_SHARD_PROTOCOL": "slices"} if protocol == "slices" else None)
    assert r.returncode == g.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name in ("out.junctions", "out.bloom", "out.dechimered_contigs.fasta"):
        with open(os.path.join(one, name), "rb") as a, open(os.path.join(two, name), "rb") as b:
            assert a.read() == b.read(), name
    assert [ln for ln in r.stdout.split("\n") if ln.startswith("Dechimered contigs:")] == [ln for ln in g.stdout.split("\n") if ln.startswith("Dechimered contigs:")]
    assert _plan_over(one, c)[0] == open(os.path.join(one, "out.dechimered_contigs.fasta"), "rb").read()
