"""Pass 1 by FILTER SLICES (fgpu_load_slice_*): N contexts in one process on the one device, each loading the WHOLE
stream into its slice of the filters' bit positions; the ranks' fail planes ORed with fgpu_bitmap_or; every rank commits its own bloo2 bits.
The concatenation of the slices must be the ORACLE's bloo1 and bloo2 byte for byte (and the compiled reference's .bloom where a golden holds
one), every rank's arrays zero outside its slice, to_bloo2 the oracle's on every rank.  Needs an MI355X."""
import functools
import hashlib
import json
import os
import time

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api, sharded
from oracle import pyoracle as po
from tests import golden_util
from tests.golden_util import Case
from tests.test_gpu_parity import _random_case, _scan_equals_oracle, chunks, oracle_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = [1, 2, 3, 4, 8]


def equal_slices(tai, world):
    """the bit ranges load_sliced gives the ranks: equal, on 64-byte boundaries, the last ones short or empty"""
    return [(lo * 8, hi * 8) for lo, hi in sharded._slices(tai // 8, world, 64)]


def run_slices(k, tai, nh, batches, bounds, **ctx_kw):
    """one context per slice, side by side: the pass over all batches, the OR of every fail plane across the contexts (reduced into the first
    context's plane, then ORed from there into the others: all hold the OR), commit, end.  Returns (contexts, stats per rank)."""
    ctxs = [api.Context(k, tai, nh, **ctx_kw) for _ in bounds]
    for ctx, (lo, hi) in zip(ctxs, bounds):
        ctx.load_slice_begin(lo, hi)
        for b in batches:
            ctx.load_slice_batch(b)
        ready, _, n_planes = ctx.load_slice_state()
        assert ready
    for ctx in ctxs:
        ctx.synchronize()
    assert len({ctx.load_slice_state()[2] for ctx in ctxs}) == 1
    for i in range(n_planes):
        planes = [ctx.load_slice_plane(i) for ctx in ctxs]
        assert len({nb for _, nb in planes}) == 1 and planes[0][1] % 16 == 0       # identical batches: identical layouts
        for p, nb in planes[1:]:
            ctxs[0].bitmap_or(planes[0][0], p, nb)
        ctxs[0].synchronize()
        for ctx, (p, nb) in zip(ctxs[1:], planes[1:]):
            ctx.bitmap_or(p, planes[0][0], nb)
    stats = []
    for ctx in ctxs:
        ctx.load_slice_commit()
        assert not ctx.load_slice_state()[0]
        stats.append(ctx.load_slice_end())
    return ctxs, stats


def assert_slices_equal(ctxs, stats, bounds, tai, want1, want2, lst, reads_processed=None):
    got1, got2 = np.zeros(tai // 8, np.uint8), np.zeros(tai // 8, np.uint8)
    for ctx, st, (lo, hi) in zip(ctxs, stats, bounds):
        b1, b2 = ctx.bloom_download(L.BLOO1), ctx.bloom_download(L.BLOO2)
        for b in (b1, b2):                                   # zero outside the own slice
            assert not b[:lo // 8].any() and not b[hi // 8:].any()
        got1[lo // 8:hi // 8] = b1[lo // 8:hi // 8]
        got2[lo // 8:hi // 8] = b2[lo // 8:hi // 8]
        assert st["to_bloo2"] == lst.to_bloo2, "to_bloo2 is the global count on every rank"
        assert st["kmers"] == lst.kmers and st["unambiguous_reads"] == lst.unambiguous_reads
        if reads_processed is not None:
            assert st["reads_processed"] == reads_processed
    assert np.array_equal(got1, want1), "concatenated bloo1 slices differ from the oracle"
    assert np.array_equal(got2, want2), "concatenated bloo2 slices differ from the oracle"


def close_all(ctxs):
    for c in ctxs:
        c.close()


# ---- 1. goldens and synthetic shapes x N -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden(name):
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    b1, b2, lst, osc = oracle_run((bases, offs), c.k, tai, nh, c.j, c.spacer)
    return c, bases, offs, tai, nh, b1, b2, lst, osc


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ["c1_k21", "ragged_k31", "twohash_k31_L150", "onehash_k25", "se_fp7_k21"])
def test_goldens_by_slices(name, world):
    c, bases, offs, tai, nh, b1, b2, lst, _ = golden(name)
    assert np.array_equal(b2.bits(), c.bloom())              # the oracle's bloo2 is the compiled reference's .bloom
    bounds = equal_slices(tai, world)
    batches = chunks(bases, offs, 3)
    ctxs, stats = run_slices(c.k, tai, nh, batches, bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, c.counters["load_reads_processed"])
    assert stats[0]["unambiguous_reads"] == c.counters["load_unambiguous"]
    if world == 1:                                           # [0, tai) is the plain load
        plain = api.Context(c.k, tai, nh)
        st = api.load_two_filters(api.Bloom(plain, L.BLOO1), api.Bloom(plain, L.BLOO2), batches)
        assert st == stats[0]
        for which in (L.BLOO1, L.BLOO2):
            assert np.array_equal(plain.bloom_download(which), ctxs[0].bloom_download(which))
        plain.close()
    close_all(ctxs)


def shape(nh, E=1_000_000):
    """(tai, n_hash) as the product sizes a filter from reads for `nh` hash functions (tests/test_gpu_filter_shapes.py: S = 0.95 E at the
    default fp for one, S = E / 5 and a smaller fp for the others)"""
    if nh == 1:
        tai, got = api.load_filter_shape(E, E * 95 // 100)
    else:
        fp = golden_util.fp_for(E, E // 5, nh, lambda e, s, f: api.load_filter_shape(e, s, f)[1])
        assert fp is not None
        tai, got = api.load_filter_shape(E, E // 5, fp)
    assert got == nh
    return tai, got


@functools.lru_cache(maxsize=None)
def shape_case(nh):
    bases, offs = _random_case(8000, 100, 25, 20000, 0.012, 500 + nh, 0.002, 3)
    tai, nh = shape(nh)
    b1, b2, lst, osc = oracle_run((bases, offs), 25, tai, nh, 1, 100)
    return bases, offs, tai, nh, b1, b2, lst, osc


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("nh", [1, 3, 5, 6, 7, 10], ids=lambda n: f"nh{n}")
def test_hash_counts_one_to_ten_by_slices(nh, world):
    """more hash functions than the kernels keep missing planes for (4): the bits past the planes are tested against the carry again"""
    bases, offs, tai, nh_, b1, b2, lst, _ = shape_case(nh)
    assert nh_ == nh
    bounds = equal_slices(tai, world)
    ctxs, stats = run_slices(25, tai, nh, chunks(bases, offs, 4), bounds)
    assert ctxs[0].n_hash == nh
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    close_all(ctxs)


# ---- 2. unequal and degenerate slices ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["one_line_and_the_rest", "an_empty_slice_among_others", "eight_ranks_on_a_tiny_filter"])
def test_unequal_and_degenerate_slices(how):
    if how == "eight_ranks_on_a_tiny_filter":                # 2048 bits: four ranks own 512 bits, four own nothing at all
        k, tai, nh = 15, 2048, 3
        bases, offs = _random_case(300, 60, k, 400, 0.01, 91, 0.01, 0)
        bounds = equal_slices(tai, 8)
        assert sum(1 for lo, hi in bounds if lo == hi) == 4
    else:
        k, tai, nh = 21, 1 << 18, 3
        bases, offs = _random_case(3000, 90, k, 6000, 0.01, 92, 0.003, 2)
        bounds = [(0, 512), (512, tai)] if how == "one_line_and_the_rest" else [(0, 1 << 16), (1 << 16, 1 << 16), (1 << 16, 3 << 16), (3 << 16, tai)]
    b1, b2, lst, _ = oracle_run((bases, offs), k, tai, nh)
    assert lst.to_bloo2 > 0
    ctxs, stats = run_slices(k, tai, nh, chunks(bases, offs, 5), bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    close_all(ctxs)


# ---- 3. scheduling invariance ------------------------------------------------------------------------------------------------------------
def ramped(bases, offs):
    n = len(offs) - 1
    cuts = sorted({0, n // 64, n // 32, n // 16, n // 8, n // 4, n // 2, n})
    return [api.ReadBatch(bases, offs[a:z + 1].copy()) for a, z in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("sweeps", [None, "0/1", "1000000/1", "0/1 at any epoch size"], ids=["default", "every", "never", "every-unbarred"])
@pytest.mark.parametrize("batching", ["one", "many", "ramped"])
def test_scheduling_invariance(batching, sweeps, monkeypatch):
    """batch boundaries and the moments at which the carry is brought up to date change which occurrences go through the resolve kernel and
    against which carry -- never a bit of the result"""
    if sweeps:
        monkeypatch.setenv("FGPU_SWEEP_RATIO", sweeps.split()[0])
        if " " in sweeps:
            monkeypatch.setenv("FGPU_SWEEP_MIN_FRAC", "0")   # (by default a sweep also waits for an epoch of tai / 16 accesses)
    k, E, S = 27, 600_000, 120_000
    bases, offs = _random_case(9000, 100, k, 15000, 0.012, 303, 0.002, 3)
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, _ = oracle_run((bases, offs), k, tai, nh)
    batches = {"one": lambda: chunks(bases, offs, 1), "many": lambda: chunks(bases, offs, 37), "ramped": lambda: ramped(bases, offs)}[batching]()
    bounds = equal_slices(tai, 3)
    ctxs, stats = run_slices(k, tai, nh, batches, bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    close_all(ctxs)


@pytest.mark.parametrize("nh", [3, 7])
def test_two_slices_of_two_to_the_31_bits(nh):
    """2^31 bits: the carry of the slice is kept by re-hashing the batch's own bits, the times restart at 0 in every batch"""
    k, tai = 31, 1 << 31
    bases, offs = _random_case(30000, 100, k, 60000, 0.01, 2031 + nh, 0.001, 3)
    b1, b2, lst, _ = oracle_run((bases, offs), k, tai, nh)
    bounds = equal_slices(tai, 2)
    ctxs, stats = run_slices(k, tai, nh, chunks(bases, offs, 5), bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(offs) - 1)
    close_all(ctxs)


# ---- 4. fuzz ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_fuzz_small_inputs_by_slices(seed, monkeypatch):
    """random k in [5, 31], 1 to 8 slices, reads with N and other bytes, reads shorter than k, random filter sizes and batchings"""
    from faucet_amd import synth
    rng = np.random.default_rng(7000 + seed)
    k = int(rng.integers(5, 32))
    world = int(rng.integers(1, 9))
    G = int(rng.integers(200, 4000))
    g = synth.make_genome(G, seed, repeats=int(rng.integers(0, 4)), repeat_len=min(G // 4, 3 * k))
    alphabet = np.frombuffer(rng.choice([b"ACGT", b"ACGTN", b"ACGTNacgt-"]), dtype=np.uint8)
    lines = []
    for _ in range(int(rng.integers(1, 1500))):
        ln = int(rng.integers(0, min(G, int(rng.choice([40, 130, 400])))))
        s = int(rng.integers(0, G - ln + 1))
        r = g[s:s + ln].copy()
        m = rng.random(ln) < rng.choice([0.0, 0.01, 0.05])
        r[m] = alphabet[rng.integers(0, len(alphabet), size=int(m.sum()))]
        lines.append(bytes(r))
    bases, offs = po.reads_from_lines(lines)
    tai = 1 << int(rng.integers(10, 20))
    nh = int(rng.integers(1, 11))
    if rng.random() < 0.5:                                   # sweeps after every batch: the later batches meet a carry
        monkeypatch.setenv("FGPU_SWEEP_RATIO", "0/1")
        monkeypatch.setenv("FGPU_SWEEP_MIN_FRAC", "0")
    b1, b2, lst, _ = oracle_run((bases, offs), k, tai, nh)
    bounds = equal_slices(tai, world)
    ctxs, stats = run_slices(k, tai, nh, chunks(bases, offs, int(rng.integers(1, 6))), bounds)
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, len(lines))
    close_all(ctxs)


# ---- 5. a scan after the sliced pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reuse", [True, False], ids=["same-batches", "other-batches"])
@pytest.mark.parametrize("name", ["c1_k21", "ragged_k31", "se_fp7_k21"])
def test_scan_after_a_sliced_pass(name, reuse):
    """rank 0's context, the other slices ORed into its bloo2 on the device: junction keys in creation order, records and counters are the
    oracle's -- with the kept `sure` planes reused (the same batches: they hold the GLOBAL routing decision) and without"""
    c, bases, offs, tai, nh, b1, b2, lst, osc = golden(name)
    bounds = equal_slices(tai, 3)
    ctxs, stats = run_slices(c.k, tai, nh, chunks(bases, offs, 3), bounds, j=c.j, max_spacer_dist=c.spacer)
    dst, nbytes = ctxs[0].bloom_devptr(L.BLOO2)
    for other in ctxs[1:]:
        other.synchronize()
        src, _ = other.bloom_devptr(L.BLOO2)
        ctxs[0].bitmap_or(dst, src, nbytes)
    assert np.array_equal(ctxs[0].bloom_download(L.BLOO2), b2.bits())
    sc = api.ReadScanner(ctxs[0])
    sst = sc.scanReads(chunks(bases, offs, 3 if reuse else 2))
    assert sst["valid_reused"] == (lst.to_bloo2 if reuse else 0)
    _scan_equals_oracle(sc, sst, osc)
    close_all(ctxs)


@pytest.mark.parametrize("name,world,ordered", [("c1_k21", 3, False), ("ragged_k31", 4, False), ("se_fp7_k21", 2, True)])
def test_run_in_turn_with_slices_on_the_device(name, world, ordered):
    """sharded.run_in_turn(protocol="slices") with the product backend: the N contexts open at once, GpuShard's planes as device tensors, the
    slice-wise OR of every plane, the copies across contexts between the library's OR and commit kernels (fenced on the host, or -- `ordered`
    -- every context on torch's current stream), the gather; then pass 2 from the gathered bloo2.  after_load once, with the final filters."""
    import torch
    c, bases, offs, tai, nh, b1, b2, lst, osc = golden(name)
    dev = torch.device("cuda", 0)
    cuts = np.linspace(0, len(offs) - 1, world + 1).astype(int)
    shards = [chunks(bases, offs[cuts[r]:cuts[r + 1] + 1].copy(), 2) for r in range(world)]
    calls = []

    def after_load(r, stats, bloo1, bloo2):
        calls.append(r)
        torch.cuda.synchronize(dev)
        assert np.array_equal(bloo1.cpu().numpy(), b1.bits()) and np.array_equal(bloo2.cpu().numpy(), b2.bits())
        assert (stats["kmers"], stats["to_bloo2"]) == (lst.kmers, lst.to_bloo2)

    def make():
        stream = torch.cuda.current_stream(dev).cuda_stream if ordered else None
        return sharded.GpuShard(api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer, stream=stream), dev)

    load_stats, sst, last = sharded.run_in_turn(make, shards, "slices", after_load)
    assert calls == [world - 1] and len(load_stats) == world
    assert all(s["to_bloo2"] == lst.to_bloo2 for s in load_stats)
    _scan_equals_oracle(last.ctx, sst, osc)
    last.close()


# ---- 6. state and argument errors --------------------------------------------------------------------------------------------------------
def refused(ctx, code, call, *args):
    rc = call(ctx.h, *args)
    assert rc == code, (call.__name__, rc)
    assert L.load().fgpu_last_error(ctx.h), call.__name__


def test_state_and_argument_errors():
    import ctypes as C
    lib = L.load()
    tai = 1 << 19
    ctx = api.Context(21, tai, 3)
    batch = api.ReadBatch.from_lines([b"ACGTTGCAAGGCTTAACCGGTTACGATCGATCGGATCGATTAGCTAGCTAGGCTAGCTAGGATCGATCGAT"] * 40)
    s = batch.c_struct()
    st = L.LoadStats()
    p, n = C.c_void_p(), C.c_uint64()
    # outside a sliced pass
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch, C.byref(s))
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_commit)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_end, C.byref(st))
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_plane, 0, C.byref(p), C.byref(n))
    assert ctx.load_slice_state() == (False, 0, 0)
    # arguments
    for lo, hi in ((0, tai - 256), (64, tai), (1024, 512), (0, tai + 512)):
        refused(ctx, L.ERR_ARG, lib.fgpu_load_slice_begin, lo, hi)
    # a plain pass is open
    ctx.load_begin()
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_begin, 0, tai)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch, C.byref(s))
    ctx.load_batch(batch)
    ctx.load_end()
    # a sliced pass is open
    ctx.load_slice_begin(0, tai // 2)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_begin, 0, tai)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_begin, 0)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_batch, C.byref(s))
    refused(ctx, L.ERR_STATE, lib.fgpu_scan_begin)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_end, C.byref(st))          # before the commit
    ctx.load_slice_batch(batch)
    assert ctx.load_slice_state()[0] and ctx.load_slice_state()[2] == 1
    ctx.load_slice_plane(0)
    refused(ctx, L.ERR_ARG, lib.fgpu_load_slice_plane, 1, C.byref(p), C.byref(n))
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_end, C.byref(st))
    with pytest.raises(api.FaucetGpuError):
        ctx.bloom_download(L.BLOO1)                                            # the filters are interleaved until the pass ends
    ctx.load_slice_commit()
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_commit)                     # twice
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch, C.byref(s))          # after the commit
    ctx.load_slice_end()
    # no fix-up after a sliced pass
    assert ctx.load_fixup_state()[0] is False
    prefix, _ = ctx.bloom_devptr(L.BLOO1)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_fixup, prefix, C.byref(st))
    ctx.close()
    # --mercy needs time-aware membership tests of other slices' bits
    mercy = api.Context(21, tai, 3, mercy=True)
    refused(mercy, L.ERR_STATE, lib.fgpu_load_slice_begin, 0, tai)
    mercy.close()
    # a sliced pass keeps every batch: without room for resident batches the batch is refused, and the message names the budget
    lean = api.Context(21, tai, 3, keep_resident=False)
    lean.load_slice_begin(0, tai)
    refused(lean, L.ERR_NOMEM, lib.fgpu_load_slice_batch, C.byref(s))
    assert b"budget" in lib.fgpu_last_error(lean.h)
    lean.close()


# ---- 7. the slice state is sized by the slice ----------------------------------------------------------------------------------------------
def test_working_bytes_follow_the_slice():
    """4 bytes of time + 2 x 1/8 byte of filter per OWN bit; at 2^33 bits the slice states of 8 ranks exist on the device at once
    (8 x 4.25 GiB -- whole-filter state would be 8 x 34 GiB)"""
    tai = 1 << 31
    lo, hi = equal_slices(tai, 8)[5]
    ctx = api.Context(31, tai, 3)
    ctx.load_slice_begin(lo, hi)
    wb = ctx.load_slice_state()[1]
    assert 4 * (hi - lo) <= wb <= 4.25 * (hi - lo) + (1 << 20)
    ctx.load_slice_commit()
    ctx.load_slice_end()
    ctx.close()
    tai = 1 << 33
    ctxs = []
    for lo, hi in equal_slices(tai, 8):
        ctx = api.Context(31, tai, 3)
        ctx.load_slice_begin(lo, hi)
        ctxs.append(ctx)
    for ctx in ctxs:
        ctx.synchronize()
        assert ctx.load_slice_state()[1] <= 4.25 * (tai // 8) + (1 << 20)
    for ctx in ctxs:
        ctx.load_slice_commit()
        st = ctx.load_slice_end()
        assert st["kmers"] == 0 and st["to_bloo2"] == 0
    close_all(ctxs)


# ---- 8. full size ----------------------------------------------------------------------------------------------------------------------
with open(os.path.join(ROOT, "tests", "golden", "fullsize.json")) as _f:
    FULL = json.load(_f)


def _sha_dev(t) -> str:
    h = hashlib.sha256()
    for lo in range(0, t.numel(), 1 << 28):
        h.update(t[lo:lo + (1 << 28)].cpu().numpy().tobytes())
    return h.hexdigest()


def sliced_full_size(batches, k, tai, nh, world, dev, groups=1):
    """load_sliced's phases on one device through sharded.GpuShard: the ranks' contexts side by side (groups = 1), or -- where the device is
    short of memory on the day -- in `groups` groups one after the other: a first round per group for the planes (kept ORed as tensors), a
    second one that loads again, takes the global planes and commits.  Returns (bloo1, bloo2, stats of the last rank, seconds per phase)."""
    import torch
    sl = sharded._slices(tai // 8, world, 64)
    out1, out2 = (torch.zeros(tai // 8, dtype=torch.uint8, device=dev) for _ in range(2))
    times = {"slice_load": [], "commit": []}
    per = -(-world // groups)
    acc, stats = None, None

    def load(ranks):
        backs = []
        for r in ranks:
            b = sharded.GpuShard(api.Context(k, tai, nh), dev)
            t0 = time.perf_counter()
            b.slice_load(batches, sl[r][0] * 8, sl[r][1] * 8)
            b.ctx.synchronize()
            times["slice_load"].append(time.perf_counter() - t0)
            backs.append(b)
        return backs

    def reduce_into_acc(backs):
        nonlocal acc
        for b in backs:
            planes = b.slice_planes()
            if acc is None:
                acc = [p.clone() for p in planes]
                torch.cuda.synchronize(dev)
            else:
                for a, p in zip(acc, planes):
                    b.or_tensor(a, p)
                b.ctx.synchronize()

    def finish(backs, ranks):
        nonlocal stats
        for b, r in zip(backs, ranks):
            for a, p in zip(acc, b.slice_planes()):
                p.copy_(a)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            b.slice_commit()
            stats = b.slice_end()
            times["commit"].append(time.perf_counter() - t0)
            lo, hi = sl[r]
            out1[lo:hi].copy_(b.bloom_tensor(L.BLOO1)[lo:hi])
            out2[lo:hi].copy_(b.bloom_tensor(L.BLOO2)[lo:hi])
            torch.cuda.synchronize(dev)
            b.close()

    rank_groups = [list(range(g * per, min((g + 1) * per, world))) for g in range(groups)]
    if groups == 1:
        backs = load(rank_groups[0])
        reduce_into_acc(backs)
        finish(backs, rank_groups[0])
    else:
        for ranks in rank_groups:
            backs = load(ranks)
            reduce_into_acc(backs)
            for b in backs:
                b.close()
        for ranks in rank_groups:
            finish(load(ranks), ranks)
    return out1, out2, stats, times


@pytest.mark.parametrize("name,world", [("config2", 4), ("config4", 8)])
def test_full_size_by_slices(name, world):
    """BASELINE config 2 on 4 slices; config 4 -- 2.0e10 stream positions through ONE rank's 32-bit clock, 2^33-bit filters, the shape the
    sliced pass exists for -- on 8, the contexts side by side on the one device: bloo1, bloo2 and to_bloo2 by the oracle's digests"""
    import torch

    import bench
    from faucet_amd import synth_det as sd
    assert name in FULL and "bloo2_sha256" in FULL[name], f"tests/golden/fullsize.json has lost the final digests of {name}"
    fx = FULL[name]
    c = fx["params"]
    dev = torch.device("cuda", 0)
    free, total = torch.cuda.mem_get_info(dev)
    tai, nh = fx["tai"], fx["n_hash"]
    positions = c["reads"] * (c["read_len"] + 1)
    # per rank: the resident stream (5 bits per position), two filters, the slice state, the batch in hand; beside the reads
    need = c["reads"] * c["read_len"] + world * (positions * 5 // 8 + 2 * (tai // 8) + 4.25 * tai / world + (2 << 30)) + (4 << 30)
    if total < need / 2:
        pytest.skip(f"{name} by {world} slices needs an MI355X-class device")
    groups = 1 if free >= need else 2
    g = sd.make_genome(c["genome"], c["genome_seed"], dev)
    if "repeats" in c:
        sd.plant_repeats(g, c["genome_seed"] + 100, *c["repeats"])
    reads = sd.make_reads(g, c["reads"], c["read_len"], c["err"], c["read_seed"], dev)
    del g
    if "reads_checksum" in fx:
        chk = 0
        for lo in range(0, c["reads"], 20_000_000):
            chk = (chk + sd.checksum(reads[lo:lo + 20_000_000], first_row=lo)) & ((1 << 64) - 1)
        assert chk == fx["reads_checksum"] & ((1 << 64) - 1), "the read generator gives other bytes here than where the fixture was made"
    batches = bench.device_batches(reads, bench.batch_bounds(c["reads"], 2_500_000 if name == "config4" else 1_000_000, 2))
    bloo1, bloo2, st, times = sliced_full_size(batches, c["k"], tai, nh, world, dev, groups)
    print(f"\n{name} by {world} slices ({groups} group(s)): slice_load per rank " + " ".join(f"{t * 1e3:.0f}" for t in times["slice_load"]) +
          " ms; commit per rank " + " ".join(f"{t * 1e3:.0f}" for t in times["commit"]) + " ms")
    assert (st["kmers"], st["to_bloo2"]) == (fx["kmers"], fx["to_bloo2"])
    assert _sha_dev(bloo1) == fx["bloo1_sha256"], "bloo1 differs from the oracle's at full size"
    assert _sha_dev(bloo2) == fx["bloo2_sha256"], "bloo2 differs from the oracle's at full size"
    del reads, bloo1, bloo2
    torch.cuda.empty_cache()
