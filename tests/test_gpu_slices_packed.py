"""The sliced pass 1 from PACKED batches (fgpu_load_slice_pack / _expect / _batch_packed, fgpu_scan_resident_base, fgpu_group_allgather): a batch
is packed once, its block is copied device to device into another context's expected block, and loading it from the packed form must be the
very same thing as fgpu_load_slice_batch of the reads -- fail planes (and miss planes under --mercy) byte for byte, and after OR, commit and
gather the ORACLE's bloo1 / bloo2 / stats.  N contexts share the one device.  Needs an MI355X."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from oracle import pyoracle as po
from tests.golden_util import Case
from tests.test_gpu_parity import chunks, oracle_run
from tests.test_gpu_slices import assert_slices_equal, close_all, equal_slices, refused
from tests.test_gpu_slices_mercy import or_across

pytestmark = pytest.mark.gpu

PADW = 8           # FGPU_PADW: padding words of every plane


@functools.lru_cache(maxsize=None)
def golden(name):
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    b1, b2, lst, osc = oracle_run((bases, offs), c.k, tai, nh, c.j, c.spacer, mercy=c.mercy)
    assert np.array_equal(b2.bits(), c.bloom())              # the oracle's bloo2 is the compiled reference's .bloom
    return c, bases, offs, tai, nh, b1, b2, lst


def stream_positions(offs, a, z):
    """T of the batch of reads [a, z): its bases and one separator per read"""
    return int(offs[z] - offs[a]) + (z - a)


def three_batches(bases, offs):
    """three batches whose first has a stream length that is an exact multiple of 64 (no partial last word) while another has not"""
    n = len(offs) - 1
    a = next(b for b in range(n // 3, n) if stream_positions(offs, 0, b) % 64 == 0)
    z = next(b for b in range(max(a + 1, 2 * n // 3), n) if stream_positions(offs, a, b) % 64 != 0)
    assert 0 < a < z < n
    assert stream_positions(offs, 0, a) % 64 == 0 and stream_positions(offs, a, z) % 64 != 0
    return [api.ReadBatch(bases, offs[lo:hi + 1].copy()) for lo, hi in ((0, a), (a, z), (z, n))]


def batches_of(bases, offs, n_batches):
    return chunks(bases, offs, 1) if n_batches == 1 else three_batches(bases, offs)


def bounds_of(tai, world):
    if world == "3 with an empty slice":
        return [(0, tai // 4), (tai // 4, tai // 4), (tai // 4, tai)]
    return equal_slices(tai, world)


class Reader:
    """device bytes on the host, through the filter buffer of a context of its own (the ABI hands out no other copy to the host)"""

    def __init__(self):
        self.ctx = api.Context(21, 1 << 23, 3)
        self.ptr, self.cap = self.ctx.bloom_devptr(L.BLOO1)

    def read(self, owner, ptr, nbytes):
        assert nbytes <= self.cap
        owner.synchronize()
        assert self.ctx.lib.fgpu_device_copy(self.ctx.h, self.ptr, ptr, nbytes) == 0
        return self.ctx.bloom_download(L.BLOO1)[:nbytes].copy()

    def close(self):
        self.ctx.close()


def begin(ctx, lo, hi):
    (ctx.load_slice_mercy_begin if ctx.mercy else ctx.load_slice_begin)(lo, hi)


def hand_over(packer, pk, loader):
    """the packed block of `packer` into a block `loader` expects, device to device on the loader's stream (the packer's work is complete)"""
    want = loader.load_slice_expect(pk.T, pk.n_reads)
    assert want.nbytes == pk.nbytes == 24 * ((pk.T + 63) // 64 + PADW) + 16 and want.T == pk.T and want.n_reads == pk.n_reads
    assert want.block_dev and want.block_dev != pk.block_dev
    assert loader.lib.fgpu_device_copy(loader.h, want.block_dev, pk.block_dev, pk.nbytes) == 0
    return want


# ---- 1. equivalence with fgpu_load_slice_batch, and the oracle's filters -------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3, "3 with an empty slice"], ids=lambda w: str(w).replace(" ", "_"))
@pytest.mark.parametrize("n_batches", [1, 3])
@pytest.mark.parametrize("name", ["c1_k21", "ragged_k31", "mercy_k21"])
def test_packed_batches_load_as_the_reads_do(name, n_batches, world):
    c, bases, offs, tai, nh, b1, b2, lst = golden(name)
    if name == "ragged_k31":                                 # reads with N inside: k_pack_fix lays their tokens out in reverse order
        raw = bases.tobytes()
        assert any(raw[int(a):int(z)].strip(b"N").count(b"N") for a, z in zip(offs[:-1], offs[1:]))
    bounds = bounds_of(tai, world)
    batches = batches_of(bases, offs, n_batches)
    rd = Reader()
    packer = api.Context(c.k, tai, nh, mercy=c.mercy)
    begin(packer, 0, 0)                                      # packs only: it owns no bit
    packed = [packer.load_slice_pack(b) for b in batches]
    packer.synchronize()
    loaders = [api.Context(c.k, tai, nh, mercy=c.mercy) for _ in bounds]      # fed packed blocks
    readers = [api.Context(c.k, tai, nh, mercy=c.mercy) for _ in bounds]      # fed the reads: what the blocks must amount to
    for group in (loaders, readers):
        for ctx, (lo, hi) in zip(group, bounds):
            begin(ctx, lo, hi)
    for i, (b, pk) in enumerate(zip(batches, packed)):
        for ctx in loaders:
            ctx.load_slice_batch_packed(hand_over(packer, pk, ctx))
        for ctx in readers:
            ctx.load_slice_batch(b)
        for a, z in zip(loaders, readers):
            assert a.load_slice_state()[2] == z.load_slice_state()[2] == i + 1
            (pa, na), (pz, nz) = a.load_slice_plane(i), z.load_slice_plane(i)
            assert na == nz and np.array_equal(rd.read(a, pa, na), rd.read(z, pz, nz)), "fail planes differ"
        if c.mercy:                                          # the lockstep: the batch's fail plane over the ranks, then its probe
            for group in (loaders, readers):
                for ctx in group:
                    ctx.synchronize()
                or_across(group, [ctx.load_slice_plane(i) for ctx in group])
                for ctx in group:
                    ctx.load_slice_mercy_probe()
    for ctx in loaders + readers:
        ctx.synchronize()
    for i in range(len(batches)):
        if c.mercy:
            for a, z in zip(loaders, readers):
                (pa, na), (pz, nz) = a.load_slice_mercy_planes(i), z.load_slice_mercy_planes(i)
                assert na == nz and np.array_equal(rd.read(a, pa, na), rd.read(z, pz, nz)), "miss planes differ"
            or_across(loaders, [ctx.load_slice_mercy_planes(i) for ctx in loaders])
        else:
            or_across(loaders, [ctx.load_slice_plane(i) for ctx in loaders])
    stats = []
    for ctx in loaders:
        ctx.load_slice_commit()
        stats.append(ctx.load_slice_end())
    assert_slices_equal(loaders, stats, bounds, tai, b1.bits(), b2.bits(), lst, c.counters["load_reads_processed"])
    assert stats[0]["unambiguous_reads"] == c.counters["load_unambiguous"]
    close_all(loaders + readers + [packer])
    rd.close()


# ---- 2. one pass that mixes reads and packed blocks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_k31", "mercy_k21"])
def test_a_pass_that_mixes_reads_and_packed_batches(name):
    """two ranks; of five batches the second and fourth come as blocks the rank packed ITSELF (no digest check: the block never left it), the
    fifth as a block packed ahead of its turn -- before the third batch is loaded -- and handed over by another context"""
    c, bases, offs, tai, nh, b1, b2, lst = golden(name)
    bounds = equal_slices(tai, 2)
    batches = chunks(bases, offs, 5)
    packer = api.Context(c.k, tai, nh, mercy=c.mercy)
    begin(packer, 0, 0)
    last = packer.load_slice_pack(batches[4])
    packer.synchronize()
    ctxs = [api.Context(c.k, tai, nh, mercy=c.mercy) for _ in bounds]
    for ctx, (lo, hi) in zip(ctxs, bounds):
        begin(ctx, lo, hi)
    for i, b in enumerate(batches):
        for ctx in ctxs:
            if i in (1, 3):
                ctx.load_slice_batch_packed(ctx.load_slice_pack(b))
            elif i == 4:
                ctx.load_slice_batch_packed(hand_over(packer, last, ctx))
            else:
                ctx.load_slice_batch(b)
        if c.mercy:
            for ctx in ctxs:
                ctx.synchronize()
            or_across(ctxs, [ctx.load_slice_plane(i) for ctx in ctxs])
            for ctx in ctxs:
                ctx.load_slice_mercy_probe()
    for ctx in ctxs:
        ctx.synchronize()
    for i in range(len(batches)):
        or_across(ctxs, [(ctx.load_slice_mercy_planes if c.mercy else ctx.load_slice_plane)(i) for ctx in ctxs])
    stats = []
    for ctx in ctxs:
        ctx.load_slice_commit()
        stats.append(ctx.load_slice_end())
    assert_slices_equal(ctxs, stats, bounds, tai, b1.bits(), b2.bits(), lst, c.counters["load_reads_processed"])
    close_all(ctxs + [packer])


# ---- 3. state and argument errors --------------------------------------------------------------------------------------------------------
def test_packed_state_and_argument_errors():
    lib = L.load()
    tai = 1 << 19
    line = b"ACGTTGCAAGGCTTAACCGGTTACGATCGATCGGATCGATTAGCTAGCTAGGCTAGCTAGGATCGATCGAT"
    T = 40 * (len(line) + 1)
    batch = api.ReadBatch.from_lines([line] * 40)
    empty = api.ReadBatch.from_lines([])
    s = batch.c_struct()
    pk = L.Packed()
    ctx = api.Context(21, tai, 3)
    # outside a sliced pass: idle, and inside a plain load pass
    for inside_a_plain_pass in (False, True):
        if inside_a_plain_pass:
            ctx.load_begin()
        refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_pack, C.byref(s), C.byref(pk))
        refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_expect, 100, 2, C.byref(pk))
        refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch_packed, C.byref(pk))
    ctx.load_batch(batch)
    ctx.load_end()
    # a first pass: its blocks, and what is refused inside it
    ctx.load_slice_begin(0, tai)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_batch, C.byref(s))                      # the plain call inside a sliced pass
    assert lib.fgpu_load_slice_pack(ctx.h, C.byref(s), None) == L.ERR_ARG
    assert lib.fgpu_load_slice_expect(ctx.h, 100, 2, None) == L.ERR_ARG
    assert lib.fgpu_load_slice_batch_packed(ctx.h, None) == L.ERR_ARG
    refused(ctx, L.ERR_ARG, lib.fgpu_load_slice_expect, 10, 11, C.byref(pk))        # more separators than positions
    refused(ctx, L.ERR_ARG, lib.fgpu_load_slice_expect, 10, 0, C.byref(pk))         # positions without a read
    refused(ctx, L.ERR_ARG, lib.fgpu_load_slice_expect, 1 << 40, 5, C.byref(pk))    # beyond max_batch_bases
    nothing = ctx.load_slice_pack(empty)                                            # a batch without reads: no block
    assert (nothing.block_dev, nothing.nbytes, nothing.T, nothing.n_reads) == (None, 0, 0, 0)
    ctx.load_slice_batch_packed(nothing)
    assert ctx.load_slice_state()[2] == 0
    assert ctx.load_slice_expect(0, 0).block_dev is None
    first = ctx.load_slice_pack(batch)
    assert first.T == T and first.n_reads == 40 and first.nbytes == 24 * ((first.T + 63) // 64 + PADW) + 16
    wrong = L.Packed(first.block_dev, first.nbytes, first.T + 1, first.n_reads)
    refused(ctx, L.ERR_ARG, lib.fgpu_load_slice_batch_packed, C.byref(wrong))       # not the description the block was made with
    stray = L.Packed(first.block_dev + 64, first.nbytes, first.T, first.n_reads)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch_packed, C.byref(stray))     # not a block of this pass at all
    ctx.load_slice_batch_packed(first)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch_packed, C.byref(first))     # loaded twice
    assert b"already" in lib.fgpu_last_error(ctx.h)
    assert ctx.load_slice_state()[2] == 1
    ctx.load_slice_commit()
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_pack, C.byref(s), C.byref(pk))    # after the commit
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_expect, 100, 2, C.byref(pk))
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch_packed, C.byref(first))
    st1 = ctx.load_slice_end()                                                      # ... and the pass can still be finished
    assert st1["reads_processed"] == 40 and st1["kmers"] == 40 * (len(line) - 21 + 1)
    # a second pass: a block of the first one is not its block
    ctx.load_slice_begin(0, tai)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_batch_packed, C.byref(first))
    assert b"earlier pass" in lib.fgpu_last_error(ctx.h)
    ctx.load_slice_batch_packed(ctx.load_slice_pack(batch))
    ctx.load_slice_commit()
    assert ctx.load_slice_end() == st1
    ctx.close()
    # a mercy pass: a packed batch owes its probe like any other
    m = api.Context(21, tai, 3, mercy=True)
    m.load_slice_mercy_begin(0, tai)
    m.load_slice_batch_packed(m.load_slice_pack(batch))
    again = m.load_slice_pack(batch)                                                # packing is allowed while the probe is owed, loading is not
    refused(m, L.ERR_STATE, lib.fgpu_load_slice_batch_packed, C.byref(again))
    refused(m, L.ERR_STATE, lib.fgpu_load_slice_commit)
    m.load_slice_mercy_probe()
    m.load_slice_batch_packed(again)
    m.load_slice_mercy_probe()
    m.load_slice_commit()
    assert m.load_slice_end()["reads_processed"] == 80
    m.close()
    # no room for resident batches: a block is counted when it is made, and the message names the numbers
    lean = api.Context(21, tai, 3, keep_resident=False)
    lean.load_slice_begin(0, tai)
    refused(lean, L.ERR_NOMEM, lib.fgpu_load_slice_pack, C.byref(s), C.byref(pk))
    assert b"budget" in lib.fgpu_last_error(lean.h) and str(T).encode() in lib.fgpu_last_error(lean.h)
    refused(lean, L.ERR_NOMEM, lib.fgpu_load_slice_expect, T, 40, C.byref(pk))
    lean.close()


# ---- 4. the digest ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", [None, "codes", "bad plane", "trailer"])
def test_a_block_that_is_not_what_its_trailer_says_is_reported(damage):
    """16 bytes of an expected block zeroed after the copy: the pass reports FGPU_ERR_ARG by fgpu_load_slice_end at the latest; the same block
    untouched loads"""
    c, bases, offs, tai, nh, b1, b2, lst = golden("c1_k21")
    lib = L.load()
    batch = chunks(bases, offs, 4)[1]
    packer, loader = api.Context(c.k, tai, nh), api.Context(c.k, tai, nh)
    packer.load_slice_begin(0, 0)
    pk = packer.load_slice_pack(batch)
    packer.synchronize()
    loader.load_slice_begin(0, tai)
    got = hand_over(packer, pk, loader)
    stride = ((pk.T + 63) // 64 + PADW) * 8
    if damage:                           # (the codes of 64 random bases, the first words of the bad plane with their separators, digest and T)
        at = {"codes": 0, "bad plane": 2 * stride, "trailer": 3 * stride}[damage]
        assert lib.fgpu_device_zero(loader.h, got.block_dev + at, 16) == 0
    loader.load_slice_batch_packed(got)
    loader.load_slice_commit()
    st = L.LoadStats()
    rc = lib.fgpu_load_slice_end(loader.h, C.byref(st))
    if damage:
        assert rc == L.ERR_ARG and b"trailer" in lib.fgpu_last_error(loader.h)
    else:
        assert rc == L.OK and st.reads_processed == batch.n_reads
    close_all([packer, loader])


# ---- 5. fgpu_scan_resident_base ------------------------------------------------------------------------------------------------------------
def test_scan_resident_base_pairs_a_scan_shard_with_its_own_batches():
    """a sliced pass over three batches on the whole filter, then a scan of batches 1-2 only -- the scan shard of a rank above 0.  With base 1
    every occurrence of those batches that the pass routed to bloo2 is answered from the kept planes; with base 0 the scan compares against
    the wrong batches and reuses nothing.  Junctions as the oracle's either way.

    What full reuse amounts to comes from the oracle: the occurrences of batches 1-2 routed to bloo2 = to_bloo2 of the whole load minus
    to_bloo2 of a load of batch 0 alone (routing never depends on later reads).  A pass over JUST batches 1-2 routes fewer of their
    occurrences (their k-mers' earlier copies in batch 0 are missing), so its reuse is a lower bound here, not the same number."""
    c, bases, offs, tai, nh, b1, b2, lst = golden("c1_k21")
    n = len(offs) - 1
    cuts = np.linspace(0, n, 4).astype(int)
    batches = chunks(bases, offs, 3)
    tail_offs = offs[cuts[1]:].copy()
    o1, o2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    first_alone = po.load_two_filters(o1, o2, bases, offs[:cuts[1] + 1].copy(), c.k)
    want_reuse = lst.to_bloo2 - first_alone.to_bloo2
    osc = po.Scanner(c.k, c.j, c.spacer, b2)
    osc.scan_reads(bases, tail_offs, paired_ends=False, no_cleaning=True)
    okeys, orecs = osc.junctions("creation")

    def scan_tail(ctx, base):
        if base is not None:
            ctx.scan_resident_base(base)
        sc = api.ReadScanner(ctx)
        sst = sc.scanReads(batches[1:])
        keys, recs = sc.junctions()
        assert np.array_equal(keys, okeys) and np.array_equal(recs["dist"], orecs["dist"]) and np.array_equal(recs["cov"], orecs["cov"])
        return sst["valid_reused"]

    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer)
    ctx.load_slice_begin(0, tai)
    for b in batches:
        ctx.load_slice_batch_packed(ctx.load_slice_pack(b))
    ctx.load_slice_commit()
    assert ctx.load_slice_end()["to_bloo2"] == lst.to_bloo2
    assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits())
    with_base = scan_tail(ctx, 1)
    ctx.scan_resident_base(0)
    without = scan_tail(ctx, None)
    # the same two batches after a pass over just those two (the filter is then theirs alone, so only the reuse is looked at)
    two = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer)
    two.load_slice_begin(0, tai)
    for b in batches[1:]:
        two.load_slice_batch(b)
    two.load_slice_commit()
    two_stats = two.load_slice_end()
    sc2 = api.ReadScanner(two)
    own_reuse = sc2.scanReads(batches[1:])["valid_reused"]
    print(f"\nvalid_reused: base 1 {with_base} (oracle {want_reuse}), base 0 {without}, after a pass over batches 1-2 alone {own_reuse}")
    assert own_reuse == two_stats["to_bloo2"] > 0
    assert with_base == want_reuse > 0
    assert with_base >= own_reuse
    assert without < with_base
    # inside a pass the call is refused; the next load pass puts the base back to 0
    ctx.scan_resident_base(1)
    ctx.load_slice_begin(0, tai)
    refused(ctx, L.ERR_STATE, L.load().fgpu_scan_resident_base, 1)
    for b in batches[1:]:
        ctx.load_slice_batch(b)
    ctx.load_slice_commit()
    ctx.load_slice_end()
    sc = api.ReadScanner(ctx)
    assert sc.scanReads(batches[1:])["valid_reused"] == own_reuse
    close_all([ctx, two])


# ---- 6. fgpu_group_allgather -----------------------------------------------------------------------------------------------------------------
def test_group_allgather_between_four_contexts_on_one_device():
    """four ranks (threads) on device 0, ranges of unequal size that are no multiple of anything, one of them empty, bytes outside the ranges
    left alone: against numpy"""
    lib = L.load()
    n, nbytes = 4, 1 << 17
    rng = np.random.default_rng(12)
    for bounds in ([5, 40_001, 40_001, 99_990, 131_000], [0, 0, 64, 128, nbytes]):
        data = [rng.integers(0, 256, nbytes, dtype=np.uint8) for _ in range(n)]
        ctxs = [api.Context(21, 1 << 20, 3) for _ in range(n)]
        g = C.c_void_p()
        assert lib.fgpu_group_create(n, L.TRANSPORT_COPY, C.byref(g)) == 0
        got, errs = [None] * n, []

        def rank(r):
            try:
                ctx = ctxs[r]
                assert lib.fgpu_group_attach(g, r, ctx.h) == 0
                ptr, _ = ctx.bloom_devptr(L.BLOO1)
                ctx.bloom_upload(L.BLOO1, data[r])
                if r == 0:               # descending offsets, offsets past the buffer: refused before anything moves
                    bad = (C.c_uint64 * 5)(0, 10, 5, 20, 30)
                    assert lib.fgpu_group_allgather(g, r, ptr, nbytes, bad) == L.ERR_ARG
                    assert lib.fgpu_group_allgather(g, r, ptr, bounds[-1] - 1, (C.c_uint64 * 5)(*bounds)) == L.ERR_ARG
                    assert lib.fgpu_group_allgather(g, r, ptr, nbytes, None) == L.ERR_ARG
                assert api.group_allgather(g, r, ptr, nbytes, bounds) == 0, lib.fgpu_group_last_error(g, r)
                got[r] = ctx.bloom_download(L.BLOO1).copy()
            except BaseException as e:   # noqa: BLE001
                errs.append((r, e))
                lib.fgpu_group_abort(g)

        th = [threading.Thread(target=rank, args=(r,)) for r in range(n)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=120)
        lib.fgpu_group_destroy(g)
        close_all(ctxs)
        assert not errs, errs
        for r in range(n):
            want = data[r].copy()
            for q in range(n):
                want[bounds[q]:bounds[q + 1]] = data[q][bounds[q]:bounds[q + 1]]
            assert np.array_equal(got[r], want), r
