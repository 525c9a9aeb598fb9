"""Pass 1 by FILTER SLICES under --mercy (fgpu_load_slice_mercy_*): N contexts in one process on the one device, each
loading the WHOLE stream into its slice of the filters' bit positions, in the lockstep of the five-step protocol -- batch, OR of its fail plane
across the contexts, probe; then the OR of every block of miss planes, commit, end.  The concatenation of the slices must be the ORACLE's
--mercy bloo1 and bloo2 byte for byte (the compiled reference's .bloom where a golden holds one), every rank's arrays zero outside its slice,
the stats the oracle's on every rank, and the commit's counts the same on every rank.  Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api, sharded, synth
from oracle import pyoracle as po
from tests.golden_util import Case
from tests.test_gpu_parity import _random_case, chunks
from tests.test_gpu_slices import WORLDS, assert_slices_equal, close_all, equal_slices, ramped, refused, shape
from tests.test_slices_mercy_cpu import MercySliceShard

pytestmark = pytest.mark.gpu

MERCY_GOLDENS = ["mercy_k21", "pe_mercy_k21", "pe_mercy_fp6_k21"]


def or_across(ctxs, planes):
    """planes = (device pointer, bytes) per context, complete on the device: afterwards every one holds the OR of all (reduced into the first
    context's, then ORed from there into the others)"""
    assert len({nb for _, nb in planes}) == 1 and planes[0][1] % 16 == 0       # identical batches: identical layouts
    for p, nb in planes[1:]:
        ctxs[0].bitmap_or(planes[0][0], p, nb)
    ctxs[0].synchronize()
    for ctx, (p, nb) in zip(ctxs[1:], planes[1:]):
        ctx.bitmap_or(p, planes[0][0], nb)
        ctx.synchronize()


def run_mercy_slices(k, tai, nh, batches, bounds, **ctx_kw):
    """one mercy context per slice, side by side, in lockstep.  Returns (contexts, stats per rank, fgpu_diag_slice_mercy per rank)."""
    ctxs = [api.Context(k, tai, nh, mercy=True, **ctx_kw) for _ in bounds]
    for ctx, (lo, hi) in zip(ctxs, bounds):
        ctx.load_slice_mercy_begin(lo, hi)
    for b in batches:
        before = ctxs[0].load_slice_state()[2]
        for ctx in ctxs:
            ctx.load_slice_batch(b)
        assert len({ctx.load_slice_state()[2] for ctx in ctxs}) == 1
        n = ctxs[0].load_slice_state()[2]
        if n == before:                                      # an empty batch: no plane, no probe owed
            continue
        for ctx in ctxs:
            ctx.synchronize()
        or_across(ctxs, [ctx.load_slice_plane(n - 1) for ctx in ctxs])
        for ctx in ctxs:
            ctx.load_slice_mercy_probe()
    for ctx in ctxs:
        assert ctx.load_slice_state()[0]
        ctx.synchronize()
    for i in range(ctxs[0].load_slice_state()[2]):
        blocks = [ctx.load_slice_mercy_planes(i) for ctx in ctxs]
        assert blocks[0][1] == 4 * (blocks[0][1] // 4) and blocks[0][1] // 4 >= ctxs[0].load_slice_plane(i)[1]      # four planes of the fail plane's stride
        or_across(ctxs, blocks)
    stats = []
    for ctx in ctxs:
        ctx.load_slice_commit()
        stats.append(ctx.load_slice_end())
    return ctxs, stats, [ctx.diag_slice_mercy() for ctx in ctxs]


def assert_counts(diags, want=None):
    """[1:] -- the commit's counts -- the same on every rank; all non-zero where the input is known to bring out all four kinds of answer"""
    assert all(d[1:] == diags[0][1:] for d in diags), diags
    assert len({d[0] for d in diags}) == 1, "every rank probes the same superset of positions"
    if want is not None:
        assert all(c > 0 for c in diags[0][1:]), diags[0]
        assert diags[0] == want, "the counts differ from the CPU stand-in's"


def mercy_oracle(bases, offs, k, tai, nh):
    """the oracle's --mercy load; the input must exercise the feature: its bloo2 differs from the plain load's"""
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    lst = po.load_two_filters(b1, b2, bases, offs, k, mercy=True)
    p1, p2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    po.load_two_filters(p1, p2, bases, offs, k)
    assert not np.array_equal(b2.bits(), p2.bits()), "--mercy changes nothing on this input: it tests nothing"
    return b1, b2, lst


def standin_counts(bases, offs, k, tai, nh):
    """the CPU stand-in of tests/test_slices_mercy_cpu.py on one rank that owns every bit: its six counts"""
    be = MercySliceShard(k, tai, nh, 1, 100)
    sharded.load_sliced(be, [(bases, offs)], 0, 1)
    return be.counts


# ---- 1. the mercy goldens x N --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden(name):
    c = Case(name)
    assert c.mercy
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    b1, b2, lst = mercy_oracle(bases, offs, c.k, tai, nh)
    return c, bases, offs, tai, nh, b1, b2, lst, standin_counts(bases, offs, c.k, tai, nh)


@pytest.mark.parametrize("n_batches", [1, 3])
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", MERCY_GOLDENS)
def test_mercy_goldens_by_slices(name, world, n_batches):
    c, bases, offs, tai, nh, b1, b2, lst, counts = golden(name)
    assert np.array_equal(b2.bits(), c.bloom())              # the oracle's --mercy bloo2 is the compiled reference's .bloom
    bounds = equal_slices(tai, world)
    batches = chunks(bases, offs, n_batches)
    ctxs, stats, diags = run_mercy_slices(c.k, tai, nh, batches, bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, c.counters["load_reads_processed"])
    assert stats[0]["unambiguous_reads"] == c.counters["load_unambiguous"]
    assert_counts(diags, counts)
    if world == 1:                                           # [0, tai) is the plain --mercy pass of one context
        plain = api.Context(c.k, tai, nh, mercy=True)
        st = api.load_two_filters(api.Bloom(plain, L.BLOO1), api.Bloom(plain, L.BLOO2), batches)
        assert st == stats[0]
        for which in (L.BLOO1, L.BLOO2):
            assert np.array_equal(plain.bloom_download(which), ctxs[0].bloom_download(which))
        plain.close()
    close_all(ctxs)


# ---- 2. scheduling invariance --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def low_coverage_case():
    k, E, S = 27, 600_000, 120_000
    bases, offs = _random_case(4000, 100, k, 80_000, 0.012, 313, 0.002, 3)      # 5x
    tai, nh = api.load_filter_shape(E, S)
    return (k, bases, offs, tai, nh) + mercy_oracle(bases, offs, k, tai, nh)


@pytest.mark.parametrize("sweeps", [None, "0/1", "1000000/1", "0/1 at any epoch size"], ids=["default", "every", "never", "every-unbarred"])
@pytest.mark.parametrize("batching", ["many", "ramped"])
def test_mercy_scheduling_invariance(batching, sweeps, monkeypatch):
    """batch boundaries and the moments at which the carry is brought up to date change against which carry a probe reads its first-set times
    -- never a bit of the result: the fold of a batch is deferred behind its probe whatever the policy"""
    if sweeps:
        monkeypatch.setenv("FGPU_SWEEP_RATIO", sweeps.split()[0])
        if " " in sweeps:
            monkeypatch.setenv("FGPU_SWEEP_MIN_FRAC", "0")   # (by default a sweep also waits for an epoch of tai / 16 accesses)
    k, bases, offs, tai, nh, b1, b2, lst = low_coverage_case()
    batches = chunks(bases, offs, 23) if batching == "many" else ramped(bases, offs)
    bounds = equal_slices(tai, 3)
    ctxs, stats, diags = run_mercy_slices(k, tai, nh, batches, bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    assert_counts(diags)
    assert all(c > 0 for c in diags[0][1:]), diags[0]
    close_all(ctxs)


def test_mercy_two_slices_of_two_to_the_31_bits():
    """2^31 bits: the carry of the slice is kept by re-hashing the batch's own bits (k_slice_carry_set, here deferred behind the probe), the times
    restart at 0 in every batch"""
    k, tai, nh = 31, 1 << 31, 3
    bases, offs = _random_case(12000, 100, k, 240_000, 0.01, 2131, 0.001, 3)      # 5x
    b1, b2, lst = mercy_oracle(bases, offs, k, tai, nh)
    bounds = equal_slices(tai, 2)
    ctxs, stats, diags = run_mercy_slices(k, tai, nh, chunks(bases, offs, 5), bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    assert_counts(diags)
    assert all(c > 0 for c in diags[0][1:]), diags[0]
    close_all(ctxs)


# ---- 3. hash counts ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_case(nh):
    """the reads and filter shapes of tests/test_gpu_filter_shapes.py's mercy case"""
    bases, offs = _random_case(8000, 100, 25, 20000, 0.012, 500 + nh, 0.002, 3)
    tai, nh = shape(nh)
    return (bases, offs, tai, nh) + mercy_oracle(bases, offs, 25, tai, nh)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("nh", [1, 3, 5, 7, 10], ids=lambda n: f"nh{n}")
def test_mercy_hash_counts_one_to_ten_by_slices(nh, world):
    """more hash functions than the mark kernel keeps missing planes for (4); the probe walks all of them for every candidate"""
    bases, offs, tai, nh_, b1, b2, lst = shape_case(nh)
    assert nh_ == nh
    bounds = equal_slices(tai, world)
    ctxs, stats, diags = run_mercy_slices(25, tai, nh, chunks(bases, offs, 4), bounds)
    assert ctxs[0].n_hash == nh
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    assert_counts(diags)
    close_all(ctxs)


# ---- 4. degenerate slices --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["an_empty_slice_among_others", "eight_ranks_on_a_tiny_filter"])
def test_mercy_degenerate_slices(how):
    if how == "eight_ranks_on_a_tiny_filter":                # 2048 bits: four ranks own 512 bits, four own nothing at all
        k, tai, nh = 15, 2048, 3
        bases, offs = _random_case(40, 60, k, 400, 0.01, 91, 0.01, 0)
        bounds = equal_slices(tai, 8)
        assert sum(1 for lo, hi in bounds if lo == hi) == 4
    else:
        k, tai, nh = 21, 1 << 18, 3
        bases, offs = _random_case(400, 90, k, 6000, 0.01, 92, 0.003, 2)
        bounds = [(0, 1 << 16), (1 << 16, 1 << 16), (1 << 16, 3 << 16), (3 << 16, tai)]
    b1, b2, lst = mercy_oracle(bases, offs, k, tai, nh)
    ctxs, stats, diags = run_mercy_slices(k, tai, nh, chunks(bases, offs, 5), bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    assert_counts(diags)
    close_all(ctxs)


# ---- 5. a scan behind the sliced mercy pass ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reuse", [True, False], ids=["same-batches", "other-batches"])
def test_scan_after_a_sliced_mercy_pass(reuse):
    """rank 0's context, the other slices ORed into its bloo2 on the device: the junction lines are the golden's -- with the kept `sure` planes
    reused (the same batches: valid & ~fail, what the plain --mercy pass leaves) and without"""
    c, bases, offs, tai, nh, b1, b2, lst, _ = golden("mercy_k21")
    bounds = equal_slices(tai, 3)
    ctxs, stats, _ = run_mercy_slices(c.k, tai, nh, chunks(bases, offs, 3), bounds, j=c.j, max_spacer_dist=c.spacer)
    dst, nbytes = ctxs[0].bloom_devptr(L.BLOO2)
    for other in ctxs[1:]:
        other.synchronize()
        src, _ = other.bloom_devptr(L.BLOO2)
        ctxs[0].bitmap_or(dst, src, nbytes)
    assert np.array_equal(ctxs[0].bloom_download(L.BLOO2), c.bloom())
    sc = api.ReadScanner(ctxs[0])
    sst = sc.scanReads(chunks(bases, offs, 3 if reuse else 2))
    assert sst["valid_reused"] == (lst.to_bloo2 if reuse else 0)
    keys, recs = sc.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines())
    assert sst["n_junctions"] == c.counters["distinct_junctions"]
    close_all(ctxs)


@pytest.mark.parametrize("name,world,ordered", [("mercy_k21", 3, False), ("pe_mercy_fp6_k21", 4, True)])
def test_run_in_turn_with_mercy_slices_on_the_device(name, world, ordered):
    """sharded.run_in_turn(protocol="slices") with the product backend on mercy contexts: GpuShard's lockstep -- the fail plane of every batch
    ORed slice-wise and copied across the contexts before the probes, the blocks of miss planes before the commit -- fenced on the host, or
    (`ordered`) every context on torch's current stream.  after_load once, with the final filters."""
    import torch
    c, bases, offs, tai, nh, b1, b2, lst, counts = golden(name)
    dev = torch.device("cuda", 0)
    cuts = np.linspace(0, len(offs) - 1, world + 1).astype(int)
    shards = [chunks(bases, offs[cuts[r]:cuts[r + 1] + 1].copy(), 2) for r in range(world)]
    calls, backs = [], []

    def after_load(r, stats, bloo1, bloo2):
        calls.append(r)
        torch.cuda.synchronize(dev)
        assert np.array_equal(bloo1.cpu().numpy(), b1.bits()) and np.array_equal(bloo2.cpu().numpy(), b2.bits())
        assert (stats["kmers"], stats["to_bloo2"]) == (lst.kmers, lst.to_bloo2)
        assert all(b.ctx.diag_slice_mercy() == counts for b in backs[:world])

    def make():
        stream = torch.cuda.current_stream(dev).cuda_stream if ordered else None
        backs.append(sharded.GpuShard(api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer, stream=stream, mercy=True), dev))
        assert backs[-1].mercy
        return backs[-1]

    load_stats, _, last = sharded.run_in_turn(make, shards, "slices", after_load)
    assert calls == [world - 1] and len(load_stats) == world
    assert all(s["to_bloo2"] == lst.to_bloo2 for s in load_stats)
    last.close()


# ---- 6. fuzz -------------------------------------------------------------------------------------------------------------------------------
# seeds of the recipe below on which --mercy changes bloo2 (checked with the oracle, on the CPU: of the first eighteen, 3 and 9 -- filters
# close to full -- change nothing and are left out)
FUZZ_SEEDS = [0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17]


def fuzz_case(seed):
    """low coverage, reads with N (several unambiguous segments per read, met right to left), random k, filter size and hash count"""
    rng = np.random.default_rng(9100 + seed)
    k = int(rng.integers(7, 32))
    G = int(rng.integers(2000, 20000))
    cov = float(rng.choice([2.0, 4.0, 8.0]))
    bases, offs = _random_case(max(4, int(G * cov / 100)), 100, k, G, float(rng.choice([0.0, 0.01, 0.03])), 9200 + seed,
                               float(rng.choice([0.004, 0.01])), int(rng.integers(0, 4)))
    tai = 1 << int(rng.integers(12, 20))
    nh = int(rng.integers(1, 11))
    return rng, k, bases, offs, tai, nh


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_mercy_fuzz_by_slices(seed, monkeypatch):
    rng, k, bases, offs, tai, nh = fuzz_case(seed)
    world = int(rng.integers(1, 9))
    n_batches = int(rng.integers(1, 6))
    if rng.random() < 0.5:                                   # sweeps after every batch: the later batches meet a carry
        monkeypatch.setenv("FGPU_SWEEP_RATIO", "0/1")
        monkeypatch.setenv("FGPU_SWEEP_MIN_FRAC", "0")
    raw = bases.tobytes()
    assert b"N" in raw and any(raw[int(a):int(z)].strip(b"N").count(b"N") for a, z in zip(offs[:200], offs[1:201]))
    b1, b2, lst = mercy_oracle(bases, offs, k, tai, nh)
    bounds = equal_slices(tai, world)
    ctxs, stats, diags = run_mercy_slices(k, tai, nh, chunks(bases, offs, n_batches), bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    assert_counts(diags)
    close_all(ctxs)


# ---- 6b. segments on the 64-position words of `bad` ----------------------------------------------------------------------------------------
WORD_EDGE_LENGTHS = [62, 63, 64, 126, 127, 128, 20, 21, 22, 85]


@functools.lru_cache(maxsize=None)
def word_boundary_case():
    """reads of 62..128 and of k - 1, k, k + 1 bases, one after the other in the stream: the unambiguous runs start on every bit of a 64-position
    word of `bad`, end a base short of k, at k and past it, and cross up to three words.  Returns the input, the oracle's --mercy load, the
    stand-in's counts and (start, length) of every run of good stream positions."""
    k, tai, nh = 21, 1 << 22, 3
    g = synth.make_genome(40000, 313)
    r = synth.make_reads(g, 3000, 128, 0.012, 314, n_rate=0.004)
    bases, offs = po.reads_from_lines([r[i, :WORD_EDGE_LENGTHS[i % 10]].tobytes() for i in range(len(r))])
    T = len(bases) + len(offs) - 1                           # the stream: every read's bases, then its separator
    good = np.zeros(T, bool)
    at = np.arange(len(bases)) + np.searchsorted(offs[1:].astype(np.int64), np.arange(len(bases)), side="right")
    good[at] = np.isin(bases, np.frombuffer(b"ACGT", np.uint8))
    edge = np.diff(np.concatenate(([0], good.astype(np.int8), [0])))
    start = np.flatnonzero(edge == 1)
    return k, tai, nh, bases, offs, T, mercy_oracle(bases, offs, k, tai, nh), standin_counts(bases, offs, k, tai, nh), start, np.flatnonzero(edge == -1) - start


@pytest.mark.parametrize("how,n", [("plain", 1), ("plain", 3), ("slices", 1), ("slices", 2), ("slices", 3)])
def test_mercy_segments_on_word_boundaries(how, n):
    """the segment walker and the state machine that the plain and the sliced --mercy pass share, at the edges of the 64-position word: the
    plain pass in n batches, the sliced one on n ranks, each against the oracle"""
    k, tai, nh, bases, offs, T, (b1, b2, lst), counts, start, length = word_boundary_case()
    # what the input is for, before the device sees it
    assert T == 218_400
    on_bit = np.bincount(start % 64, minlength=64)
    assert on_bit.min() > 0 and (on_bit[0], on_bit[63]) == (123, 160)
    assert [int((length == x).sum()) for x in (k - 1, k, k + 1)] == [296, 297, 291]
    assert int((length >= 127).sum()) == 374                # a window of 64 positions lies inside the run: it crosses three words
    assert counts == [70098, 43, 1799, 720, 349, 5543]
    if how == "plain":
        ctx = api.Context(k, tai, nh, mercy=True)
        st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, n))
        assert np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits()) and np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits())
        assert (st["kmers"], st["to_bloo2"], st["unambiguous_reads"]) == (lst.kmers, lst.to_bloo2, lst.unambiguous_reads)
        ctx.close()
        return
    bounds = equal_slices(tai, n)
    ctxs, stats, diags = run_mercy_slices(k, tai, nh, chunks(bases, offs, 3), bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    assert_counts(diags, counts)
    close_all(ctxs)


# ---- 7. state and argument errors ------------------------------------------------------------------------------------------------------------
def test_mercy_state_and_argument_errors():
    lib = L.load()
    tai = 1 << 19
    batch = api.ReadBatch.from_lines([b"ACGTTGCAAGGCTTAACCGGTTACGATCGATCGGATCGATTAGCTAGCTAGGCTAGCTAGGATCGATCGAT"] * 40)
    empty = api.ReadBatch.from_lines([])
    s, e = batch.c_struct(), empty.c_struct()
    p, n = C.c_void_p(), C.c_uint64()
    # a context without FGPU_FLAG_MERCY: no mercy pass, and the new calls are refused inside its plain sliced pass
    plain = api.Context(21, tai, 3)
    refused(plain, L.ERR_STATE, lib.fgpu_load_slice_mercy_begin, 0, tai)
    refused(plain, L.ERR_STATE, lib.fgpu_load_slice_mercy_probe)
    refused(plain, L.ERR_STATE, lib.fgpu_load_slice_mercy_planes, 0, C.byref(p), C.byref(n))
    plain.load_slice_begin(0, tai)
    plain.load_slice_batch(batch)
    plain.load_slice_batch(batch)                                              # no probe is owed in a plain sliced pass
    refused(plain, L.ERR_STATE, lib.fgpu_load_slice_mercy_probe)
    refused(plain, L.ERR_STATE, lib.fgpu_load_slice_mercy_planes, 0, C.byref(p), C.byref(n))
    plain.load_slice_commit()
    plain.load_slice_end()
    assert plain.diag_slice_mercy() == [0] * 6
    plain.close()
    # a mercy context: the three-step protocol stays refused, and its message names the way in
    ctx = api.Context(21, tai, 3, mercy=True)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_begin, 0, tai)
    assert b"fgpu_load_slice_mercy_begin" in lib.fgpu_last_error(ctx.h)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_mercy_probe)                # outside a pass
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_mercy_planes, 0, C.byref(p), C.byref(n))
    for lo, hi in ((0, tai - 256), (64, tai), (1024, 512), (0, tai + 512)):
        refused(ctx, L.ERR_ARG, lib.fgpu_load_slice_mercy_begin, lo, hi)
    ctx.load_slice_mercy_begin(0, tai // 2)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_mercy_begin, 0, tai)
    ctx.load_slice_mercy_probe()                                               # nothing owed: FGPU_OK, nothing done
    ctx.load_slice_batch(empty)                                                # an empty batch keeps no plane and owes no probe
    assert ctx.load_slice_state()[2] == 0
    ctx.load_slice_batch(batch)
    assert ctx.load_slice_state()[2] == 1
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch, C.byref(s))           # while a probe is owed
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch, C.byref(e))
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_commit)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_mercy_planes, 0, C.byref(p), C.byref(n))     # ... its planes do not exist yet
    ctx.load_slice_plane(0)
    ctx.load_slice_mercy_probe()
    ctx.load_slice_mercy_probe()
    ptr, nb = ctx.load_slice_mercy_planes(0)
    assert ptr and nb % 16 == 0 and nb // 4 >= ctx.load_slice_plane(0)[1]
    refused(ctx, L.ERR_ARG, lib.fgpu_load_slice_mercy_planes, 1, C.byref(p), C.byref(n))      # a batch that does not exist
    ctx.load_slice_batch(batch)
    ctx.load_slice_mercy_probe()
    ctx.load_slice_commit()
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch, C.byref(s))           # after the commit
    ctx.load_slice_end()
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_mercy_probe)
    ctx.close()
    # nine bits per stream position stay resident: without room the batch is refused, and the message names the budget
    lean = api.Context(21, tai, 3, mercy=True, keep_resident=False)
    lean.load_slice_mercy_begin(0, tai)
    refused(lean, L.ERR_NOMEM, lib.fgpu_load_slice_batch, C.byref(s))
    assert b"budget" in lib.fgpu_last_error(lean.h) and b"miss planes" in lib.fgpu_last_error(lean.h)
    lean.close()


# ---- 8. full size --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_mercy_full_size_by_four_slices():
    """10^6 reads x 100 bp of synth_det reads at 5x on 4 slices side by side, ten batches, against the oracle's --mercy load"""
    import torch

    from faucet_amd import synth_det as sd
    dev = torch.device("cuda", 0)
    k, n = 31, 1_000_000
    g = sd.make_genome(20_000_000, 77, dev)
    reads = sd.make_reads(g, n, 100, 0.01, 78, dev)
    bases, offs = po.reads_from_matrix(reads.cpu().numpy())
    del g, reads
    tai, nh = api.load_filter_shape(40_000_000, 16_000_000)
    b1, b2, lst = mercy_oracle(bases, offs, k, tai, nh)
    bounds = equal_slices(tai, 4)
    ctxs, stats, diags = run_mercy_slices(k, tai, nh, chunks(bases, offs, 10), bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, n)
    assert_counts(diags)
    assert all(c > 0 for c in diags[0][1:]), diags[0]
    print(f"\n10^6 reads by 4 slices under --mercy: probed {diags[0][0]} of {lst.kmers} windows; tests and runs {diags[0][1:]}")
    close_all(ctxs)
