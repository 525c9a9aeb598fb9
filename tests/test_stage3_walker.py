"""faucet_amd/stage3.py (findNeighbor for many junctions in lock-step over the batched Stage-3 probes) against the reference's own
findNeighbor (tests/golden/stage3_neighbors_*.jsonl.gz, made by oracle/_ref/ref_kat neighbors): on the golden maps, on runs of the reference at
even and small k, and on seeded variants of both (tests/stage3_variants.py) that reach what a clean scan's static map does not -- the
reference's asserts, junctions before and past maxDist, walks that run out, contigs over 128 bases, distances over 255.

CPU: the walker's host logic with the ORACLE answering getValidJExtension (checker only); GPU: the product path, fgpu_probe_valid_extension."""
import collections
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from faucet_amd import stage3
from oracle import pyoracle as po
from tests import stage3_variants as V
from tests.golden_util import GOLDEN, Case

FIXTURES = V.fixture_names()
REF_KAT = os.path.join(os.path.dirname(GOLDEN), os.pardir, "oracle", "_ref", "ref_kat")
EXE = os.path.join(os.path.dirname(GOLDEN), os.pardir, "faucet_amd", "faucet")
_cache = {}
Fixture = collections.namedtuple("Fixture", "case bloom keys recs max_read_length calls lines")


def _map_of(lines):
    keys, cov, dist, linked = V.parse_map(lines)
    recs = np.zeros(len(keys), dtype=po.JUNC_DTYPE)
    recs["cov"], recs["dist"], recs["linked"] = cov, dist, linked
    return keys, recs


Params = collections.namedtuple("Params", "k j counters spacer max_read_length")        # what a Fixture's `case` is asked for, of a map that is no golden case


def fixture_from(bloom, lines, k, n_hash, j, max_read_length, calls=None, spacer=100):
    """a Fixture of (filter bytes, .junctions lines, k, hash count, j, max read length) made on the spot, no golden case behind it"""
    return Fixture(Params(k, j, {"n_hash": n_hash}, spacer, max_read_length), np.asarray(bloom, dtype=np.uint8), *_map_of(lines), max_read_length, calls, lines)


def _fixture(name):
    """a fixture's case, filter bytes, map (keys, recs, .junctions lines), max_read_length and the reference's calls; made once, shared, left unchanged"""
    if name not in _cache:
        c = Case(name.split("__")[0])
        bloom, lines, mrl = V.inputs_of(name, c)
        with gzip.open(os.path.join(GOLDEN, f"stage3_neighbors_{name}.jsonl.gz"), "rt") as f:
            kat = [json.loads(line) for line in f if line.strip()]
        _cache[name] = Fixture(c, bloom, *_map_of(lines), mrl, kat, lines)
    return _cache[name]


def _same_as_reference(kat, got, contigs=None):
    """`abort` exactly where the reference aborted, otherwise its result field for field (and BfSearchResult::contig, the sequence getContig
    strings together)"""
    assert len(got) == len(kat)
    for i, (e, g) in enumerate(zip(kat, got)):
        if e.get("abort"):
            assert g["abort"] == 1, (e, g)
            continue
        assert g["abort"] == 0, (e, g)
        assert (int(g["kmer"]), int(g["node"]), int(g["rindex"]), int(g["dist"]), int(g["len"])) == (int(e["kmer"], 16), e["node"], e["rindex"], e["dist"], e["len"]), e
        if contigs is not None:
            assert contigs[i] == e["contig"], e


def _starts(kat):
    return np.array([int(e["start"], 16) for e in kat], dtype=np.uint64), np.array([e["index"] for e in kat], dtype=np.int8)


def _check(name, ctx):
    c, bloom, keys, recs, mrl, kat, _ = _fixture(name)
    w = stage3.NeighborWalker(ctx, keys, recs, c.k, mrl)
    _same_as_reference(kat, w.find_neighbors(*_starts(kat)))
    return w


class _OracleProbe:
    """stand-in for api.Context.probe_valid_extension (TEST ONLY): the oracle's restatement of getValidJExtension"""

    def __init__(self, c, bloom):
        self.k, self.j = c.k, c.j
        self.b = po.Bloom(len(bloom) * 8, c.counters["n_hash"])
        self.b.set_bits(bloom)

    def probe_valid_extension(self, kmers):
        return np.array([po.lib().fo_stage3_valid_extension(self.b.h, int(x), self.k, self.j) for x in kmers], dtype=np.int8)


def _device(name):
    return device_of(_fixture(name))


def device_of(fx):
    """a context of the fixture's shape with its filter uploaded as bloo2"""
    from faucet_amd import _lib as L
    from faucet_amd import api
    c, bloom = fx[:2]
    ctx = api.Context(c.k, len(bloom) * 8, c.counters["n_hash"], j=c.j, max_spacer_dist=c.spacer)
    ctx.bloom_upload(L.BLOO2, bloom)
    return ctx


@pytest.mark.parametrize("name", FIXTURES)
def test_walker_host_logic_against_the_reference_findNeighbor(name):
    c, bloom = _fixture(name)[:2]
    _check(name, _OracleProbe(c, bloom))


def test_the_fixtures_reach_every_class_of_call():
    """what tests/golden/make_stage3_neighbors.py requires of its inputs, counted again from the stored answers and the maps the recipes give:
    every class of call (the reference's asserts, junctions before / at / past maxDist, sinks, long contigs, far results, contig lengths at
    a word's edge, even k, both kinds of start) at least as often as tests/stage3_variants.py::MINIMUM asks, and as the summary file says"""
    with open(os.path.join(GOLDEN, "stage3_neighbors_summary.json")) as f:
        summary = json.load(f)
    assert sorted(summary["fixtures"]) == sorted(FIXTURES) and summary["minimum"] == V.MINIMUM
    total = dict.fromkeys(V.CLASSES, 0)
    for name in FIXTURES:
        fx = _fixture(name)
        kat = fx.calls
        n = V.count_classes(kat, fx.lines, fx.case.k)
        assert dict(calls=len(kat), **n) == summary["fixtures"][name], name
        for cl in V.CLASSES:
            total[cl] += n[cl]
    assert all(total[cl] >= V.MINIMUM[cl] for cl in V.CLASSES), total
    assert {cl: summary["total"][cl] for cl in V.CLASSES} == total


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_walker_on_the_device_probes_against_the_reference_findNeighbor(name):
    w = _check(name, _device(name))
    assert w.steps > 0 and w.probes >= w.steps       # one device call per lock-step round, many walks per call


def _check_device_walks(name, ctx):
    c, bloom, keys, recs, mrl, kat, _ = _fixture(name)
    ctx.stage3_set_junctions(keys, recs)
    starts, idx = _starts(kat)
    got, probes, contigs = ctx.stage3_find_neighbors(starts, idx, mrl, contigs=True)
    _same_as_reference(kat, got, contigs)
    plain, probes2 = ctx.stage3_find_neighbors(starts, idx, mrl)
    assert probes2 == probes and plain.tobytes() == got.tobytes()
    return probes


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_whole_walks_on_the_device_against_the_reference_findNeighbor(name):
    """fgpu_stage3_find_neighbors: every probe, every k-mer step and every map look-up of a walk on the device, one lane per walk; equal to the
    reference's own findNeighbor on every fixture, contig strings included, and to the lock-step walker probe for probe."""
    ctx = _device(name)
    probes = _check_device_walks(name, ctx)
    w = _check(name, ctx)
    assert probes == w.probes


@pytest.mark.gpu
def test_contig_stride_exactly_the_words_asked_for_and_one_less():
    """contig_stride_words = fgpu_stage3_contig_words(k, max_read_length) holds every contig of the fixture with the longest ones; one word less
    is FGPU_ERR_ARG, and nothing is written"""
    import ctypes as C

    from faucet_amd import _lib as L
    from faucet_amd import api
    name = "s3_k24_long__drop70"
    c, bloom, keys, recs, mrl, kat, _ = _fixture(name)
    assert max(e.get("len", 0) for e in kat) > 128
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    starts, idx = _starts(kat)
    n = len(starts)
    words = int(ctx.lib.fgpu_stage3_contig_words(c.k, mrl))
    assert 32 * words >= max(e.get("len", 0) for e in kat)
    want, want_probes, _ = ctx.stage3_find_neighbors(starts, idx, mrl, contigs=True)
    for stride in (words, words - 1):
        out = np.full(n, 0x5A, dtype=np.uint8).repeat(api.NEIGHBOR_DTYPE.itemsize).view(api.NEIGHBOR_DTYPE)
        text = np.full(n * words + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)           # (one word of margin behind the last walk's)
        probes = C.c_uint64(12345)
        rc = ctx.lib.fgpu_stage3_find_neighbors(ctx.h, starts.ctypes.data, idx.ctypes.data, n, mrl, out.ctypes.data, C.byref(probes), text.ctypes.data, stride)
        if stride == words:
            assert rc == L.OK and probes.value == want_probes and out.tobytes() == want.tobytes()
            codes = (text[:n * words].reshape(n, words)[:, :, None] >> (2 * np.arange(32, dtype=np.uint64))[None, None, :]) & np.uint64(3)
            chars = np.frombuffer(b"ACTG", dtype=np.uint8)[codes.reshape(n, words * 32).astype(np.int64)]
            for i, e in enumerate(kat):
                if not e.get("abort"):
                    assert chars[i, :e["len"]].tobytes().decode() == e["contig"], e
            assert text[n * words] == 0xA5A5A5A5A5A5A5A5
        else:
            assert rc == L.ERR_ARG and probes.value == 12345
            assert (out.view(np.uint8) == 0x5A).all() and (text == 0xA5A5A5A5A5A5A5A5).all()
    again, again_probes = ctx.stage3_find_neighbors(starts, idx, mrl)                   # the refused call left the context usable
    assert again_probes == want_probes and again.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_walks_repeated_over_block_and_grid_edges_scale_exactly():
    """one call with a fixture's walks repeated to just over 256 and just over 65 536 entries (more than one block; more than 256 blocks, with a
    last block and a last wave that are partly empty): every copy equals the first, contigs included, and the per-wave probe sums add up to
    exactly the multiple of one copy's"""
    name = "twohash_k31_L150__shift"
    c, bloom, keys, recs, mrl, kat, _ = _fixture(name)
    kat = kat[::13]
    assert len(kat) == 38 and any(e.get("abort") for e in kat) and any(e.get("node") == 0 for e in kat)
    ctx = _device(name)
    ctx.stage3_set_junctions(keys, recs)
    starts, idx = _starts(kat)
    one, probes, contigs = ctx.stage3_find_neighbors(starts, idx, mrl, contigs=True)
    _same_as_reference(kat, one, contigs)
    assert probes > 0
    got, p, text = ctx.stage3_find_neighbors(np.tile(starts, 7), np.tile(idx, 7), mrl, contigs=True)        # 266 walks
    assert p == 7 * probes and got.tobytes() == one.tobytes() * 7 and text == contigs * 7
    reps = 65536 // len(kat) + 1                                                                             # 65 550 walks
    got, p = ctx.stage3_find_neighbors(np.tile(starts, reps), np.tile(idx, reps), mrl)
    assert len(got) > 65536 and len(got) % 64 and p == reps * probes and got.tobytes() == one.tobytes() * reps


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(REF_KAT), reason="oracle/_ref/ref_kat was not built (make -C oracle ref)")
@pytest.mark.parametrize("seed", range(8))
def test_whole_walks_on_the_device_against_the_live_reference_on_a_random_run(seed, tmp_path, monkeypatch):
    """no stored answer: the product's own `faucet` writes .bloom and .junctions of a random single-end run (every second one at an even k), one
    drawn variant is applied, and `ref_kat neighbors` and fgpu_stage3_find_neighbors have to agree call for call, contigs included"""
    from faucet_amd import _lib as L
    from faucet_amd import api
    from tests.test_oracle_vs_reference_fuzz import random_run
    rng = np.random.default_rng(4100 + seed)
    if seed % 2:
        monkeypatch.setenv("FUZZ_K", str(int(rng.choice([8, 14, 20, 26, 30]))))
    else:
        monkeypatch.delenv("FUZZ_K", raising=False)
    path, fastq, args = random_run(620 + seed, tmp_path)            # (runs whose scan finds junctions: one without errors and repeats has none)
    args = [a for a in args if a != "--paired_ends"]
    if "--no_cleaning" not in args:
        args.append("--no_cleaning")                  # (the files are written either way; without it the command line ends with status 3)
    opt = lambda f, d: int(args[args.index(f) + 1]) if f in args else d      # noqa: E731
    k, j, mrl = opt("-size_kmer", 0), opt("-j", 1), opt("-max_read_length", 0)
    r = subprocess.run([EXE, "-read_load_file", path, "-read_scan_file", path, "-file_prefix", str(tmp_path / "out")] + args,
                       capture_output=True, text=True, errors="replace", timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    nh = int(re.search(r"Number of hash functions: (\d+)", r.stdout).group(1))
    bloom = np.fromfile(str(tmp_path / "out.bloom"), dtype=np.uint8)
    lines = (tmp_path / "out.junctions").read_text().split("\n")[:-1]
    assert lines
    kind = V.KINDS[int(rng.integers(0, len(V.KINDS)))]
    bloom, lines, mrl = V.apply(kind, int(rng.integers(0, 2**31)), bloom, lines, mrl)
    bloom.tofile(str(tmp_path / "v.bloom"))
    (tmp_path / "v.junctions").write_text("\n".join(lines) + "\n")
    r = subprocess.run([REF_KAT, "neighbors", str(tmp_path / "v.bloom"), str(len(bloom) * 8 - 1), str(nh), str(k), str(j), str(tmp_path / "v.junctions"), str(mrl)],
                       capture_output=True, text=True, timeout=300)
    kat = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"kat":"neighbor"')]
    assert r.returncode == 0 and kat, (r.returncode, r.stderr[-500:])
    ctx = api.Context(k, len(bloom) * 8, nh, j=j)
    ctx.bloom_upload(L.BLOO2, bloom)
    ctx.stage3_set_junctions(*_map_of(lines))
    starts, idx = _starts(kat)
    got, probes, contigs = ctx.stage3_find_neighbors(starts, idx, mrl, contigs=True)
    _same_as_reference(kat, got, contigs)


@pytest.mark.gpu
def test_whole_walks_on_the_device_equal_the_lock_step_walker_on_a_scanned_map():
    """a map two orders of magnitude larger than the goldens (the scan's own result on 60 k reads): every covered extension of every junction,
    device walks against the lock-step walker; plus the argument checks"""
    import bench
    import torch
    from faucet_amd import _lib as L
    from faucet_amd import api
    dev = torch.device("cuda", 0)
    n = 60_000
    reads = bench.make_reads(bench.make_genome(2 * n, 2, dev), n, 100, 0.01, 1000, dev)
    tai, nh = api.load_filter_shape(10 * n, 2 * n)
    ctx = api.Context(31, tai, nh)
    with pytest.raises(api.FaucetGpuError):
        ctx.stage3_find_neighbors(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int8), 100)      # no map yet
    lst, sst, b2, keys, recs = bench.step_single(ctx, bench.device_batches(reads, 20_000))
    assert len(keys) > 2000
    starts, idx = [], []
    for i in range(5):
        m = (recs["dist"][:, i] > 0) & ((recs["cov"][:, i] > 0) if i < 4 else True)
        starts.append(keys[m])
        idx.append(np.full(int(m.sum()), i))
    starts, idx = np.concatenate(starts), np.concatenate(idx)
    ctx.stage3_set_junctions(keys, recs)
    got, probes = ctx.stage3_find_neighbors(starts, idx, 100)
    w = stage3.NeighborWalker(ctx, keys, recs, 31, 100)
    want = w.find_neighbors(starts, idx)
    for f in ("kmer", "node", "rindex", "dist", "len", "abort"):
        assert np.array_equal(got[f], want[f]), f
    assert probes == w.probes and (got["node"] == 1).sum() > 1000
    _, _, contigs = ctx.stage3_find_neighbors(starts[:5000], idx[:5000], 100, contigs=True)
    assert [len(t) for t in contigs] == [int(v) for v in got["len"][:5000]] and all(set(t) <= set("ACGT") for t in contigs)
    # a start that is no junction of the map, an index out of range: flagged per walk, the others are unaffected
    bad, _ = ctx.stage3_find_neighbors(np.array([starts[0], 12345, starts[1]], dtype=np.uint64), np.array([idx[0], 0, 7], dtype=np.int8), 100)
    assert list(bad["abort"]) == [int(got["abort"][0]), 2, 2] and bad["kmer"][0] == got["kmer"][0]
    with pytest.raises(api.FaucetGpuError):
        ctx.stage3_set_junctions(np.array([5, 5], dtype=np.uint64), recs[:2])                        # a k-mer twice
