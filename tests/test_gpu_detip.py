"""ContigGraph::deleteTipsAndClean on the device's build (faucet_amd/csrc/tips_plan.cpp, stage3_emit.hip, stage3_join.hip): fgpu_stage3_detip on
every golden fixture against the compiled reference's own file and graph after the step (tests/golden/detip_<name>.fasta.gz, .graph.gz), with the
map in the order the reference's map iterated in; fgpu_stage3_fasta_joined on hand-made joined text against a printer of a few lines, on the text a
join left on the device, and its argument errors; `faucet --detipped_contigs`.  Needs an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import detip_golden as D
from tests import raw_contigs_ref as P
from tests.golden_util import Case
from tests.test_gpu_raw_contigs import _random, _rc, _take_build
from tests.test_raw_contigs_ref_cpu import golden_build
from tests.test_stage3_walker import _device, _fixture

pytestmark = pytest.mark.gpu
NAMES = sorted(D.summary()["fixtures"])
K = 21                                              # of the context the hand-made strings are printed on (c1_k21's)


def test_the_goldens_are_there():
    assert len(NAMES) == 28


def device_table(ctx, info):
    """the graph table with its counts line (tests/detip_golden.py) of the graph fgpu_stage3_detip left, taken with fgpu_stage3_graph_take: its
    contigs' bases and coverages by a join over the build where it lies"""
    graph = ctx.stage3_graph_take()
    joined = ctx.stage3_join(graph["lists"]) if graph["lists"] else (np.zeros(0), [], [], [], [])
    assert [len(s) for s in joined[1]] == [int(v) for v in graph["contigs"]["len"]]
    nodes = [(int(n["key"]), [int(v) for v in n["cov"]], [int(v) for v in n["slot"]]) for n in graph["nodes"]]
    contigs = [(int(t["node1"]) if t["has1"] else None, int(t["node2"]) if t["has2"] else None, int(t["len"]), int(t["ind1"]), int(t["ind2"]), int(t["isolated"]))
               for t in graph["contigs"]]
    table = D.table_of(nodes, contigs, [(len(s), float(a)) for s, a in zip(joined[1], joined[4])], info["changed"])
    counts = "counts %d %d %d\n" % (info["tips"], info["print"]["nodes"], sum(info["collapsed"][1:] + info["degenerate"][1:]) if info["validated"] else -1)
    return table + counts


@pytest.mark.parametrize("name", NAMES)
def test_detip_equals_the_references_file_and_graph(name):
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    want = D.summary()["fixtures"][name]
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    built = ctx.stage3_build(fx.max_read_length, take=False)
    assert built["status"] == 0 and built["totals"][0] == len(b.calls) and want["records"] <= 193
    got, info = ctx.stage3_detip(fx.max_read_length)
    assert got == D.golden(name, "fasta")
    assert (info["tips"], info["print"]["nodes"], info["changed"], info["print"]["records"]) == (want["tips"], want["nodes"], want["changed"], want["records"])
    assert {key: info[key] for key in ("nodes_before", "back_tips", "validated")} == {key: want[key] for key in ("nodes_before", "back_tips", "validated")}
    assert info["collapsed"] == [want["collapsed_0"], want["collapsed_1"]] and info["degenerate"] == [want["degenerate_0"], want["degenerate_1"]]
    assert {key: info["print"][key] for key in ("bubble_records", "node_contigs", "isolated_kept", "isolated_dropped")} == \
           {key: want[key] for key in ("bubble_records", "node_contigs", "isolated_kept", "isolated_dropped")}
    assert device_table(ctx, info) == D.golden(name, "graph").decode()
    with pytest.raises(RuntimeError):                                          # taken: nothing left
        ctx.stage3_graph_take()
    again, info2 = ctx.stage3_detip(fx.max_read_length)                        # the build is still there, and unchanged
    assert again == got and info2 == info
    kept = _take_build(ctx, built["totals"])
    fresh = ctx.stage3_build(fx.max_read_length, raw=True)
    assert all(a.tobytes() == f.tobytes() for a, f in zip(kept, fresh[:6]))


def test_detip_needs_a_finished_untaken_build_that_returned():
    from faucet_amd import _lib as L
    name = "c1_k21"
    keys, recs = golden_build(name)[1:3]
    fx = _fixture(name)
    ctx = _device(name)
    nbytes, ti = C.c_uint64(7), L.TipsInfo()

    def call():
        return ctx.lib.fgpu_stage3_detip(ctx.h, fx.max_read_length, C.byref(nbytes), C.byref(ti))
    ctx.stage3_set_junctions(keys, recs)
    assert call() == L.ERR_ARG and nbytes.value == 0                          # no build yet
    ctx.stage3_build(fx.max_read_length)
    assert call() == L.ERR_ARG                                                # taken
    ctx.stage3_set_junctions(keys[:0], recs[:0])
    ctx.stage3_build(fx.max_read_length, take=False)
    got, info = ctx.stage3_detip(fx.max_read_length)
    assert got == b"" and info["tips"] == info["nodes_before"] == info["print"]["records"] == 0
    assert ctx.stage3_graph_take()["lists"] == []
    stopped = "s3_k8__zero2"                                                  # the reference trips an assert in buildContigGraph on this map
    fx = _fixture(stopped)
    ctx = _device(stopped)
    ctx.stage3_set_junctions(fx.keys, fx.recs)
    built = ctx.stage3_build(fx.max_read_length, take=False)
    assert built["status"] in (1, 3)
    assert ctx.lib.fgpu_stage3_detip(ctx.h, fx.max_read_length, C.byref(nbytes), C.byref(ti)) == L.ERR_ARG
    assert b"status" in ctx.lib.fgpu_last_error(ctx.h)
    assert len(_take_build(ctx, built["totals"])[0]) == built["stop_call"]    # ... and is still takeable


# ---- fgpu_stage3_fasta_joined on hand-made joined text ----
def _printer(numbers, strings):
    return "".join(">Contig%d\n%s\n" % (n, min(s, _rc(s))) for n, s in zip(numbers, strings)).encode()


def _joined_of(strings):
    from faucet_amd import api
    text, first = P.pack_text(strings)
    joined = np.zeros(len(strings), dtype=api.JOINED_DTYPE)
    joined["text_word"], joined["len"] = first, [len(s) for s in strings]
    return joined, text


def _hand_made():
    """(numbers, strings): record bytes are 8 + digits + bases + 1"""
    rng = np.random.default_rng(21)
    strings = [_random(rng, n) for n in (K, 31, 32, 33, 63, 64, 65)]          # numbers 1 .. 7: 10 + bases bytes each
    numbers = list(range(1, 8))
    used = sum(10 + len(s) for s in strings)
    strings.append(_random(rng, 4096 - used - 10))                            # number 8 ends on the first tile's last byte,
    strings.append(_random(rng, 50))                                          # number 9 starts on the second tile's first
    strings.append(_random(rng, 2 * 4096 + 1))                                # number 10: one record of 2 x 4 KiB + 1 bases
    numbers += [8, 9, 10]
    strings += [_random(rng, 1) for _ in range(400)]                          # 400 records of one base, eleven bytes each while the number has one digit
    numbers += [1 + i % 9 for i in range(400)]
    strings += [_random(rng, 5) for _ in range(4)]
    numbers += [99, 100, 999999999, 4294967295]
    strings.append("ACGT" * 5)                                                # its own reverse complement: stays
    x, y = _random(rng, 2048), _random(rng, 5)                                # the reverse complement first differs at base 2 049 (index 2 048): word 64,
    strings.append(x + "G" + y + "A" + _rc(x))                                # the wave's second step; G against T there: stays (codes alone would turn it)
    strings.append(x + "T" + y + "C" + _rc(x))                                # ... is turned
    x = _random(rng, 64)                                                      # ... and in word 2 (base 65) of the first step
    strings.append(x + "T" + y + "C" + _rc(x))
    strings += ["GA", "TC"]
    numbers += [11, 12, 13, 14, 15, 16]
    return numbers, strings


def test_fasta_joined_of_hand_made_text_against_the_printer():
    ctx = _device("c1_k21")
    numbers, strings = _hand_made()
    want = _printer(numbers, strings)
    assert want[4095:4097] == b"\n>" and want.find(b">Contig9\n") == 4096 and b">Contig100\n" in want and b">Contig99\n" in want
    assert _printer([1], ["TC"]) == b">Contig1\nGA\n"                          # (the printer itself: letters, not codes)
    joined, text = _joined_of(strings)
    assert ctx.stage3_fasta_joined(joined, numbers, text) == want
    for lo, hi in ((0, 1), (7, 8), (9, 10), (10, 410), (300, len(strings)), (len(strings) - 6, len(strings) - 4)):      # slices: other offsets, other tiles
        j, t = _joined_of(strings[lo:hi])
        assert ctx.stage3_fasta_joined(j, numbers[lo:hi], t) == _printer(numbers[lo:hi], strings[lo:hi]), (lo, hi)
    order = np.random.default_rng(22).permutation(len(strings))                # records in another order than their strings lie in the text
    assert ctx.stage3_fasta_joined(joined[order], [numbers[i] for i in order], text) == _printer([numbers[i] for i in order], [strings[i] for i in order])
    assert ctx.stage3_fasta_joined(joined[:0], [], text) == b"" and ctx.stage3_fasta_joined(joined[:0], [], None) == b""   # n = 0


def test_fasta_joined_on_the_text_a_join_left_on_the_device():
    from faucet_amd import _lib as L
    from faucet_amd import api
    name = "onehash_k25"
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    ctx.stage3_build(fx.max_read_length, take=False)
    status, graph, records, _ = api.tips_plan(keys, recs, *P.arrays_of(b.calls)[:2], fx.case.k, fx.max_read_length)
    assert status == 0 and max(len(p) for _, p in records) > 2
    lists, numbers = [p for _, p in records], np.array([n for n, _ in records], dtype=np.uint32)
    joined, text, _, _ = ctx.stage3_join(lists, raw=True)                      # taken: the uploaded form
    uploaded = ctx.stage3_fasta_joined(joined, numbers, text)
    assert uploaded == D.golden(name, "fasta")
    nbytes = C.c_uint64(3)
    assert ctx.lib.fgpu_stage3_fasta_joined(ctx.h, joined.ctypes.data, numbers.ctypes.data, len(joined), None, 0, C.byref(nbytes)) == L.ERR_STATE and nbytes.value == 0
    first = np.zeros(len(lists) + 1, dtype=np.uint64)
    first[1:] = np.cumsum([len(p) for p in lists])
    pieces = np.zeros(int(first[-1]), dtype=api.JOIN_PIECE_DTYPE)
    pieces["call"], pieces["flip"] = [c for p in lists for c, _ in p], [int(f) for p in lists for _, f in p]
    out, totals = np.zeros(len(lists), dtype=api.JOINED_DTYPE), (C.c_uint64 * 3)()
    assert ctx.lib.fgpu_stage3_join(ctx.h, first.ctypes.data, len(lists), pieces.ctypes.data, len(pieces), None, 0, None, 0, None, 0, None, 0, out.ctypes.data, totals) == L.OK
    assert ctx.stage3_fasta_joined(out, numbers, None) == uploaded             # the join's text where it lies
    jt, jd, jc = np.zeros(totals[0], dtype=np.uint64), np.zeros(totals[1], dtype=np.uint8), np.zeros(totals[2], dtype=np.uint8)
    assert ctx.lib.fgpu_stage3_join_take(ctx.h, jt.ctypes.data, len(jt), jd.ctypes.data, len(jd), jc.ctypes.data, len(jc)) == L.OK and jt.tobytes() == text.tobytes()


def test_fasta_joined_argument_errors():
    from faucet_amd import _lib as L
    ctx = _device("c1_k21")
    numbers, strings = _hand_made()
    numbers, strings = np.array(numbers[:12], dtype=np.uint32), strings[:12]
    joined, text = _joined_of(strings)
    want = _printer(numbers, strings)
    nbytes = C.c_uint64(5)

    def call(j, n, t=text, words=None):
        return ctx.lib.fgpu_stage3_fasta_joined(ctx.h, j.ctypes.data, numbers.ctypes.data, n, None if t is None else t.ctypes.data,
                                                (0 if t is None else len(t)) if words is None else words, C.byref(nbytes))
    assert call(joined, len(joined)) == L.OK and nbytes.value == len(want)
    for field, value in (("text_word", len(text) + 1), ("len", 0), ("len", 32 * (len(text) - int(joined["text_word"][3])) + 1), ("text_word", len(text))):
        bad = joined.copy()
        bad[field][3] = value
        assert call(bad, len(bad)) == L.ERR_ARG and nbytes.value == 0, (field, value)
    assert call(joined, 1 << 32) == L.ERR_ARG
    assert call(joined, len(joined), None, 5) == L.ERR_ARG                     # words of no text
    assert call(joined, len(joined), None) == L.ERR_STATE                      # no join whose text the records could index
    assert ctx.stage3_fasta_take(len(want)) == want                            # ... and the file of the good call is still there
    ok = joined.copy()
    ok["len"][9] = 32 * (len(text) - int(joined["text_word"][9]))              # up to the text's last base: fine
    assert call(ok, len(ok)) == L.OK


# ---- the command line ----
def _plan_over(cwd, c):
    """the restatement in FILE order over the run's own .junctions and .bloom: tests/graph_build_ref.py's build with the oracle answering the probes,
    tests/detip_plan_ref.py's plan over it (which tests/test_detip_plan_cpu.py pins to the compiled reference's own files), tests/detip_ref.join's text"""
    from tests import detip_plan_ref as R
    from tests import graph_build_ref as G
    from tests.test_graph_build_ref_cpu import Finder
    from tests.test_stage3_walker import Fixture, _map_of
    with open(os.path.join(cwd, "out.junctions")) as f:
        lines = f.read().split("\n")[:-1]
    bloom = np.fromfile(os.path.join(cwd, "out.bloom"), dtype=np.uint8)
    keys, recs = _map_of(lines)
    fx = Fixture(c, bloom, keys, recs, c.max_read_length, None, lines)
    f = Finder(fx, keys, recs)
    b = G.build_contig_graph(lambda alive, km, ix: f.find(np.asarray(alive, dtype=bool), km, ix), keys, recs["cov"], c.k)
    assert b.status == 0
    records, info = R.plan(b.calls, keys, recs["cov"], c.k, c.max_read_length)[2:]
    from tests import detip_ref as J
    joined = J.join(D.triples_of(b.calls), [p for _, p in records], c.k) if records else []
    return D.fasta_of(records, joined), info, P.raw_contigs(b.calls, keys, recs["cov"], c.k, c.max_read_length)[0]


@pytest.mark.parametrize("name", ["c1_k21", "twohash_k31_L150"])
def test_cli_detipped_contigs(name, tmp_path):
    """`faucet --detipped_contigs` writes <prefix>.detipped_contigs.fasta behind the scan outputs, alone and behind <prefix>.raw_contigs.fasta;
    every other output file, and the exit code, are those of a run without the flag (as for --raw_contigs there is no reference file for this
    path: a map reloaded from .junctions iterates in another order than the one that was dumped)"""
    from tests.test_gpu_estimate_stream import output_files, written_input
    from tests.test_gpu_scan_kept_cli import run
    c = Case(name)
    inp = written_input(c, tmp_path)
    args = ["-read_load_file", inp, "-read_scan_file", inp] + c.meta["args"]
    plain, alone, both = str(tmp_path / "plain"), str(tmp_path / "alone"), str(tmp_path / "both")
    g = run(plain, args)
    r = run(alone, args + ["--detipped_contigs"])
    r2 = run(both, args + ["--detipped_contigs", "--raw_contigs"])
    assert r.returncode == r2.returncode == g.returncode == (0 if c.no_cleaning else 3), r.stdout[-2000:] + r.stderr[-3000:]
    for ext in output_files(c):
        for cwd in (alone, both):
            with open(os.path.join(plain, "out." + ext), "rb") as a, open(os.path.join(cwd, "out." + ext), "rb") as b:
                assert a.read() == b.read(), ext
    assert sorted(os.listdir(alone)) == sorted(os.listdir(plain) + ["out.detipped_contigs.fasta"])
    assert sorted(os.listdir(both)) == sorted(os.listdir(plain) + ["out.detipped_contigs.fasta", "out.raw_contigs.fasta"])
    want, info, raw = _plan_over(alone, c)
    for cwd in (alone, both):
        with open(os.path.join(cwd, "out.detipped_contigs.fasta"), "rb") as f:
            assert f.read() == want
    with open(os.path.join(both, "out.raw_contigs.fasta"), "rb") as f:
        assert f.read() == raw
    assert info["tips"] > 0 and want != raw
    line = [ln for ln in r.stdout.split("\n") if ln.startswith("Detipped contigs:")]
    assert len(line) == 1 and line[0].startswith("Detipped contigs: %d tips deleted (and %d back tips), %d of %d nodes left, %d records" % (
        info["tips"], info["back_tips"], info["nodes"], info["nodes_before"], info["records"]))
    assert "Detipped contigs:" not in g.stdout and "Raw contigs:" not in r.stdout
    assert r2.stdout.index("Raw contigs:") < r2.stdout.index("Detipped contigs:")      # raw file first, then this one


@pytest.mark.parametrize("protocol", ["shards", "slices"])
def test_cli_detipped_contigs_with_two_ranks(protocol, tmp_path):
    """-gpus 2 (both ranks on the one device): the last rank's context holds the merged map and the whole bloo2 after either protocol -- the
    file, and the junctions it was built on, are the one-device run's"""
    from tests.test_gpu_estimate_stream import written_input
    from tests.test_gpu_scan_kept_cli import run
    c = Case("c1_k21")
    inp = written_input(c, tmp_path)
    args = ["-read_load_file", inp, "-read_scan_file", inp] + c.meta["args"] + ["--detipped_contigs"]
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    g = run(one, args)
    r = run(two, args + ["-gpus", "2"], env={"FAUCET_SHARD_PROTOCOL": "slices"} if protocol == "slices" else None)
    assert r.returncode == g.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name in ("out.junctions", "out.bloom", "out.detipped_contigs.fasta"):
        with open(os.path.join(one, name), "rb") as a, open(os.path.join(two, name), "rb") as b:
            assert a.read() == b.read(), name
    assert [ln for ln in r.stdout.split("\n") if ln.startswith("Detipped contigs:")] == [ln for ln in g.stdout.split("\n") if ln.startswith("Detipped contigs:")]
    assert _plan_over(one, c)[0] == open(os.path.join(one, "out.detipped_contigs.fasta"), "rb").read()
