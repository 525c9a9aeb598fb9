"""The raw contigs on the device (faucet_amd/csrc/stage3_emit.hip, raw_plan.cpp): fgpu_stage3_raw_contigs on every golden fixture against the
compiled reference's own <prefix>.raw_contigs.fasta (tests/golden/raw_contigs_<name>.fasta.gz), byte for byte, with the map in the order the
reference's map iterated in; fgpu_stage3_fasta on hand-made text against a ten-line printer; `faucet --raw_contigs`.  Needs an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import graph_build_ref as G
from tests import raw_contigs_ref as P
from tests.golden_util import Case
from tests.test_graph_build_ref_cpu import Finder
from tests.test_raw_contigs_ref_cpu import NAMES, golden_build, golden_fasta
from tests.test_stage3_walker import Fixture, _device, _fixture, _map_of

pytestmark = pytest.mark.gpu
K = 21                                              # of the context the hand-made strings are printed on (c1_k21's)


def _take_build(ctx, totals):
    from faucet_amd import api
    n, nt, ns, nc = totals
    out, calls = np.zeros(n, dtype=api.CONTIG_DTYPE), np.zeros(n, dtype=api.BUILD_DTYPE)
    text, kmers, dist, cov = np.zeros(nt, dtype=np.uint64), np.zeros(ns, dtype=np.uint64), np.zeros(ns, dtype=np.uint8), np.zeros(nc, dtype=np.uint8)
    assert ctx.lib.fgpu_stage3_build_take(ctx.h, out.ctypes.data, calls.ctypes.data, n, text.ctypes.data, nt, kmers.ctypes.data, dist.ctypes.data, ns,
                                          cov.ctypes.data, nc) == 0
    return out, calls, text, kmers, dist, cov


@pytest.mark.parametrize("name", NAMES)
def test_raw_contigs_equal_the_references_file(name):
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    built = ctx.stage3_build(fx.max_read_length, take=False)
    assert built["status"] == 0 and built["totals"][0] == len(b.calls)
    got, info = ctx.stage3_raw_contigs(fx.max_read_length)
    assert got == golden_fasta(name)
    assert info == P.plan(b.calls, keys, recs["cov"], fx.case.k, fx.max_read_length)[1]
    again, info2 = ctx.stage3_raw_contigs(fx.max_read_length)                 # the build is still there, and unchanged
    assert again == got and info2 == info
    kept = _take_build(ctx, built["totals"])
    fresh = ctx.stage3_build(fx.max_read_length, raw=True)
    assert all(a.tobytes() == f.tobytes() for a, f in zip(kept, fresh[:6]))


def test_raw_contigs_need_a_finished_untaken_build_that_returned():
    from faucet_amd import _lib as L
    name = "c1_k21"
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    ctx = _device(name)
    nbytes, ri = C.c_uint64(7), L.RawInfo()

    def call():
        return ctx.lib.fgpu_stage3_raw_contigs(ctx.h, fx.max_read_length, C.byref(nbytes), C.byref(ri))
    ctx.stage3_set_junctions(keys, recs)
    assert call() == L.ERR_ARG and nbytes.value == 0                          # no build yet
    ctx.stage3_build(fx.max_read_length)
    assert call() == L.ERR_ARG                                                # taken
    ctx.stage3_set_junctions(keys[:0], recs[:0])
    ctx.stage3_build(fx.max_read_length, take=False)
    assert ctx.stage3_raw_contigs(fx.max_read_length) == (b"", dict.fromkeys(("records", "bubble_records", "node_contigs", "isolated_kept", "isolated_dropped", "nodes"), 0))
    stopped = "s3_k8__zero2"                                                  # the reference trips an assert in buildContigGraph on this map
    fx = _fixture(stopped)
    ctx = _device(stopped)
    ctx.stage3_set_junctions(fx.keys, fx.recs)
    built = ctx.stage3_build(fx.max_read_length, take=False)
    assert built["status"] in (1, 3)
    assert ctx.lib.fgpu_stage3_raw_contigs(ctx.h, fx.max_read_length, C.byref(nbytes), C.byref(ri)) == L.ERR_ARG
    assert b"status" in ctx.lib.fgpu_last_error(ctx.h)
    assert len(_take_build(ctx, built["totals"])[0]) == built["stop_call"]    # ... and is still takeable


# ---- fgpu_stage3_fasta on hand-made text ----
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _rc(s):
    return "".join(COMPLEMENT[ch] for ch in reversed(s))


def _printer(records, k):
    """records: (number, [(string, flip), ...]) -> the file"""
    out = []
    for number, pieces in records:
        s = [_rc(x) if flip else x for x, flip in pieces]
        seq = s[0] if len(s) == 1 else s[0][:len(s[0]) - k] + s[1]
        out.append(">Contig%d\n%s\n" % (number, min(seq, _rc(seq))))
    return "".join(out).encode()


def _device_file(ctx, records):
    from faucet_amd import api
    strings = [x for _, pieces in records for x, _ in pieces]
    text, first = P.pack_text(strings)
    seqs = np.zeros(len(records), dtype=api.FASTA_SEQ_DTYPE)
    at = 0
    for i, (number, pieces) in enumerate(records):
        seqs[i]["number"], seqs[i]["pieces"] = number, len(pieces)
        for p, (x, flip) in enumerate(pieces):
            seqs[i]["text_word"][p], seqs[i]["len"][p], seqs[i]["flip"][p] = first[at], len(x), int(flip)
            at += 1
    return seqs, text, ctx.stage3_fasta(seqs, text)


def _random(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def _hand_made_records():
    rng = np.random.default_rng(20)
    records = []
    for n in (1, 31, 32, 33, 63, 64, 65, 200):                                # one piece, both flips
        for flip in (False, True):
            records.append([(_random(rng, n), flip)])
    for seam in range(32):                                                    # the seam at every offset of a word, in the first word and in the third
        for words, (f0, f1) in zip((0, 2, 0, 2), ((False, False), (True, False), (False, True), (True, True))):
            records.append([(_random(rng, K + seam + 32 * words), f0), (_random(rng, K + int(rng.integers(0, 70))), f1)])
    records.append([(_random(rng, K), True), (_random(rng, 40), False)])       # a first piece of exactly k bases gives nothing
    records.append([(_random(rng, K), False), (_random(rng, K), True)])
    records.append([("ACGT" * 5, False)])                                      # its own reverse complement: stays
    records.append([("ACGT" * 20 + "AATT" + "ACGT" * 20, True)])
    records.append([("GA", False)])                                            # G against T at the first base: G < T as letters, T < G as codes
    records.append([("TC", False)])
    for n in (40, 2100):                                                       # ... and G against T at base 40, and at base 2100 (the wave's second step)
        x, y = _random(rng, n), _random(rng, 5)
        records.append([(x + "G" + y + "A" + _rc(x), False)])                  # stays: codes alone would turn it
        records.append([(x + "T" + y + "C" + _rc(x), False)])                  # is turned: codes alone would keep it
    records.append([(_random(rng, 10000), True)])                              # one record over several tiles of output
    records += [[(_random(rng, 1), False)] for _ in range(800)]                # ... and tiles of as many records as a tile can hold
    records.append([(_random(rng, 4097), False), (_random(rng, 3000), True)])
    numbers = list(range(1, len(records) + 1))                                 # 9 -> 10 and 99 -> 100 on the way
    numbers[-3:] = [999999999, 1000000000, 4294967295]
    for i in range(len(records) - 801, len(records) - 1):                      # (eleven bytes each: the shortest record there is)
        numbers[i] = 1 + i % 9
    return list(zip(numbers, records))


def test_fasta_of_hand_made_text_against_the_printer():
    ctx = _device("c1_k21")
    assert ctx.k == K
    records = _hand_made_records()
    want = _printer(records, K)
    assert b">Contig9\n" in want and b">Contig10\n" in want and b">Contig99\n" in want and b">Contig100\n" in want and len(want) > 5 * 4096
    assert b">Contig%d\nGA\n" % next(n for n, p in records if p[0][0] == "TC") in want       # (the printer itself: letters, not codes)
    seqs, text, got = _device_file(ctx, records)
    assert got == want
    for lo, hi in ((0, 1), (5, 6), (16, 17), (16, 145), (144, 152)):           # slices of it: other offsets, other tiles
        assert _device_file(ctx, records[lo:hi])[2] == _printer(records[lo:hi], K)


def test_fasta_edges_of_the_call():
    from faucet_amd import _lib as L
    from faucet_amd import api
    ctx = _device("c1_k21")
    nbytes = C.c_uint64(5)
    assert ctx.stage3_fasta(np.zeros(0, dtype=api.FASTA_SEQ_DTYPE), np.zeros(0, dtype=np.uint64)) == b""      # n = 0
    records = _hand_made_records()[:40]
    want = _printer(records, K)
    seqs, text, _ = _device_file(ctx, records)
    assert ctx.lib.fgpu_stage3_fasta(ctx.h, seqs.ctypes.data, len(seqs), text.ctypes.data, len(text), C.byref(nbytes)) == L.OK and nbytes.value == len(want)
    out = np.full(len(want) + 8, 0x5A, dtype=np.uint8)
    assert ctx.lib.fgpu_stage3_fasta_take(ctx.h, out.ctypes.data, len(want) - 1) == L.ERR_ARG and (out == 0x5A).all()      # one byte short: nothing copied
    assert ctx.lib.fgpu_stage3_fasta_take(ctx.h, out.ctypes.data, len(want)) == L.OK                                       # ... and the file is still there
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0x5A).all()
    assert ctx.lib.fgpu_stage3_fasta_take(ctx.h, out.ctypes.data, 0) == L.OK                                               # taken: nothing left
    for field, p, value in (("text_word", 0, len(text)), ("len", 0, 0), ("pieces", None, 3), ("pieces", None, 0), ("len", 1, 32 * len(text) + 1)):
        bad = seqs.copy()
        row = next(i for i in range(len(bad)) if bad[i]["pieces"] == 2)
        if p is None:
            bad[field][row] = value
        else:
            bad[field][row][p] = value
        assert ctx.lib.fgpu_stage3_fasta(ctx.h, bad.ctypes.data, len(bad), text.ctypes.data, len(text), C.byref(nbytes)) == L.ERR_ARG, (field, p)
    short = seqs.copy()
    row = next(i for i in range(len(short)) if short[i]["pieces"] == 2)
    short["len"][row][0] = K - 1                                               # a first piece of two below k
    assert ctx.lib.fgpu_stage3_fasta(ctx.h, short.ctypes.data, len(short), text.ctypes.data, len(text), C.byref(nbytes)) == L.ERR_ARG
    assert ctx.lib.fgpu_stage3_fasta(ctx.h, seqs.ctypes.data, len(seqs), None, 0, C.byref(nbytes)) == L.ERR_STATE          # no build whose text the pieces could index


def test_fasta_on_the_text_of_a_build_left_on_the_device():
    """text_host == NULL: the pieces index the build's own text; the records are the restatement's plan laid over the device's contigs"""
    name = "twohash_k31_L150"
    b, keys, recs = golden_build(name)[:3]
    fx = _fixture(name)
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    built = ctx.stage3_build(fx.max_read_length, take=False)
    from faucet_amd import api
    contigs = _take_build(ctx, built["totals"])[0]                             # (only to know where the device lays each string)
    ctx.stage3_build(fx.max_read_length, take=False)
    records = P.plan(b.calls, keys, recs["cov"], fx.case.k, fx.max_read_length)[0]
    seqs = np.zeros(len(records), dtype=api.FASTA_SEQ_DTYPE)
    for i, r in enumerate(records):
        seqs[i]["number"], seqs[i]["pieces"] = r.number, len(r.pieces)
        for p, (c, flip) in enumerate(r.pieces):
            seqs[i]["text_word"][p], seqs[i]["len"][p], seqs[i]["flip"][p] = contigs[c]["text_word"], contigs[c]["len"], int(flip)
    assert ctx.stage3_fasta(seqs) == golden_fasta(name)


# ---- the command line ----
def _restatement_over(cwd, c):
    """the restatement in FILE order over the run's own .junctions and .bloom"""
    with open(os.path.join(cwd, "out.junctions")) as f:
        lines = f.read().split("\n")[:-1]
    bloom = np.fromfile(os.path.join(cwd, "out.bloom"), dtype=np.uint8)
    keys, recs = _map_of(lines)
    fx = Fixture(c, bloom, keys, recs, c.max_read_length, None, lines)
    f = Finder(fx, keys, recs)
    b = G.build_contig_graph(lambda alive, km, ix: f.find(np.asarray(alive, dtype=bool), km, ix), keys, recs["cov"], c.k)
    assert b.status == 0
    return P.raw_contigs(b.calls, keys, recs["cov"], c.k, c.max_read_length)


@pytest.mark.parametrize("name", ["c1_k21", "twohash_k31_L150"])
def test_cli_raw_contigs(name, tmp_path):
    """`faucet --raw_contigs` writes <prefix>.raw_contigs.fasta behind the scan outputs: the restatement run in file order over the run's own
    .junctions and .bloom.  There is no reference file for this path -- the reference's main cannot print the file (src/Faucet.cpp:314 is
    commented out), and a map reloaded from .junctions iterates in another order than the one that was dumped -- so the tie to the reference is the
    restatement, which tests/test_raw_contigs_ref_cpu.py pins to the compiled reference's own files on the stored fixtures and
    tests/test_stage3_fuzz_cpu.py on maps made on the spot; tests/test_gpu_stage3_fuzz.py runs this command line on the reads behind those maps,
    its scan files against faucet_ref's and its contig files against the restatement so pinned.  Every other output file, and the exit code, are
    those of a run without the flag."""
    from tests.test_gpu_estimate_stream import output_files, written_input
    from tests.test_gpu_scan_kept_cli import run
    c = Case(name)
    inp = written_input(c, tmp_path)
    args = ["-read_load_file", inp, "-read_scan_file", inp] + c.meta["args"]
    plain, raw = str(tmp_path / "plain"), str(tmp_path / "raw")
    g = run(plain, args)
    r = run(raw, args + ["--raw_contigs"])
    assert r.returncode == g.returncode == (0 if c.no_cleaning else 3), r.stdout[-2000:] + r.stderr[-3000:]
    for ext in output_files(c):
        with open(os.path.join(plain, "out." + ext), "rb") as a, open(os.path.join(raw, "out." + ext), "rb") as b:
            assert a.read() == b.read(), ext
    assert sorted(os.listdir(raw)) == sorted(os.listdir(plain) + ["out.raw_contigs.fasta"])
    want, info, _ = _restatement_over(raw, c)
    with open(os.path.join(raw, "out.raw_contigs.fasta"), "rb") as f:
        assert f.read() == want
    line = [ln for ln in r.stdout.split("\n") if ln.startswith("Raw contigs:")]
    assert len(line) == 1 and line[0].startswith("Raw contigs: %d records (%d bubble, %d off nodes, %d isolated; %d isolated below" % (
        info["records"], info["bubble_records"], info["node_contigs"], info["isolated_kept"], info["isolated_dropped"]))
    assert "Raw contigs:" not in g.stdout


@pytest.mark.parametrize("protocol", ["shards", "slices"])
def test_cli_raw_contigs_with_two_ranks(protocol, tmp_path):
    """-gpus 2 (both ranks on the one device): the last rank's context holds the merged map and the whole bloo2 after either protocol -- the
    file, and the junctions it was built on, are the one-device run's"""
    from tests.test_gpu_estimate_stream import written_input
    from tests.test_gpu_scan_kept_cli import run
    c = Case("c1_k21")
    inp = written_input(c, tmp_path)
    args = ["-read_load_file", inp, "-read_scan_file", inp] + c.meta["args"] + ["--raw_contigs"]
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    g = run(one, args)
    r = run(two, args + ["-gpus", "2"], env={"FAUCET_SHARD_PROTOCOL": "slices"} if protocol == "slices" else None)
    assert r.returncode == g.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name in ("out.junctions", "out.bloom", "out.raw_contigs.fasta"):
        with open(os.path.join(one, name), "rb") as a, open(os.path.join(two, name), "rb") as b:
            assert a.read() == b.read(), name
    assert [ln for ln in r.stdout.split("\n") if ln.startswith("Raw contigs:")] == [ln for ln in g.stdout.split("\n") if ln.startswith("Raw contigs:")]
