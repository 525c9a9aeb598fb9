"""A sliced pass 1 that keeps its reads (fgpu_load_slice_keep_reads, _packed_reads, _expect_reads, _adopt_reads) and the scan of kept batches
behind it (fgpu_scan_kept_range, fgpu_scan_batch_kept, fgpu_scan_prepare_kept).  Two contexts share the one device: A packs every batch with
its reads kept, B expects the blocks, gets blocks and read offsets device to device and adopts them; both load and commit.  What B's scans of
the kept batches produce is compared with the goldens of the compiled reference and with the oracle (tests/test_gpu_scan_kept.py's checks).
The offsets B adopts are checked on the device against their block: every corruption below must come back as FGPU_ERR_ARG naming the batch --
an error path that is bounds-checked by construction (every position is compared with T before a plane is read); nothing here relies on a
fault.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from tests.test_gpu_scan_kept import assert_scan_is_the_references, context_for, ref, scan_kept, set_pair_filters
from tests.test_gpu_slices import close_all, equal_slices
from tests.test_gpu_slices_mercy import or_across
from tests.test_gpu_slices_packed import Reader, begin, hand_over, three_batches

pytestmark = pytest.mark.gpu

STATE, ARG = f"error {L.ERR_STATE}:", f"error {L.ERR_ARG}:"


class Writer:
    """host bytes into device memory of another context, through the filter buffer of a context of its own (the ABI has no other way in)"""

    def __init__(self):
        self.ctx = api.Context(21, 1 << 23, 3)
        self.ptr, self.cap = self.ctx.bloom_devptr(L.BLOO1)

    def write(self, owner, ptr, data):
        buf = np.zeros(self.cap, dtype=np.uint8)
        buf[:len(data)] = np.frombuffer(data, dtype=np.uint8)
        self.ctx.bloom_upload(L.BLOO1, buf)
        self.ctx.synchronize()
        assert owner.lib.fgpu_device_copy(owner.h, ptr, self.ptr, len(data)) == 0
        owner.synchronize()

    def close(self):
        self.ctx.close()


def sliced_pass(r, batches, keep):
    """A owns the lower half of the filter bits and packs every batch, B the upper half and is handed the blocks; planes ORed, committed,
    ended, both filters gathered.  Returns the contexts, the blocks as each knows them, the stats and the ORed fail planes' addresses"""
    bounds = equal_slices(r.tai, 2)
    A, B = context_for(r), context_for(r)
    for ctx, (lo, hi) in zip((A, B), bounds):
        begin(ctx, lo, hi)
        if keep:
            ctx.load_slice_keep_reads()
    own, theirs = [], []
    for i, b in enumerate(batches):
        pk = A.load_slice_pack(b)
        A.synchronize()
        q = hand_over(A, pk, B)
        A.load_slice_batch_packed(pk)
        B.load_slice_batch_packed(q)
        own.append(pk)
        theirs.append(q)
        if r.c.mercy:
            for ctx in (A, B):
                ctx.synchronize()
            or_across([A, B], [ctx.load_slice_plane(i) for ctx in (A, B)])
            for ctx in (A, B):
                ctx.load_slice_mercy_probe()
    for ctx in (A, B):
        ctx.synchronize()
    for i in range(len(batches)):
        or_across([A, B], [(ctx.load_slice_mercy_planes if r.c.mercy else ctx.load_slice_plane)(i) for ctx in (A, B)])
    planes = [A.load_slice_plane(i) for i in range(len(batches))]
    stats = []
    for ctx in (A, B):
        ctx.load_slice_commit()
        stats.append(ctx.load_slice_end())
    for which in (L.BLOO1, L.BLOO2):                         # each holds its own slice and zeros elsewhere: the gather is an OR both ways
        (pa, n), (pb, _) = A.bloom_devptr(which), B.bloom_devptr(which)
        A.bitmap_or(pa, pb, n)
        A.synchronize()
        B.bitmap_or(pb, pa, n)
        B.synchronize()
    return A, B, own, theirs, stats, planes


def hand_offsets(A, pk, B, q, longest):
    src = A.load_slice_packed_reads(pk)
    dst = B.load_slice_expect_reads(q)
    assert dst.n_reads == src.n_reads == pk.n_reads and dst.offsets_dev and dst.offsets_dev != src.offsets_dev
    assert B.lib.fgpu_device_copy(B.h, dst.offsets_dev, src.offsets_dev, (pk.n_reads + 1) * 8) == 0
    dst.max_read_len = longest
    B.load_slice_adopt_reads(q, dst)


def scan_kept_two_step(ctx, sizes):
    """scan_kept with every batch prepared first (fgpu_scan_prepare_kept) and all of them walked by fgpu_scan_walk_prepared"""
    ctx.scan_begin()
    for i, n in enumerate(sizes):
        assert ctx.scan_prepare_kept(i) == n
    ctx.scan_walk_prepared()
    sst = ctx.scan_end()
    lists, seqs = [], []
    while True:
        t = ctx.take_stops()
        if t is None:
            break
        seq, st = t
        seqs.append(seq)
        per_read = [[] for _ in range(sizes[seq])]
        for e in st:
            per_read[int(e["read"])].append(int(e["ext"]))
        lists.extend(per_read)
    assert seqs == list(range(len(sizes)))
    return sst, lists


def assert_filters_are_the_references(ctx, r):
    assert np.array_equal(ctx.bloom_download(L.BLOO2), r.c.bloom()), "bloo2 differs from the reference's .bloom file"
    assert np.array_equal(ctx.bloom_download(L.BLOO1), r.b1.bits())


# ---- 1. the scans of kept batches behind a sliced pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21"])
def test_kept_scans_after_a_sliced_pass_equal_the_reference(name):
    r = ref(name)
    batches = three_batches(r.bases, r.offs)
    sizes = [b.n_reads for b in batches]
    longest = int(np.diff(r.offs).max())
    rd = Reader()
    # a sliced pass WITHOUT keeping: what the filters, stats and fail planes must stay
    C0, D0, _, _, plain_stats, plain_planes = sliced_pass(r, batches, keep=False)
    plain = [rd.read(C0, p, n) for p, n in plain_planes]
    assert C0.scan_kept_state()["complete"] is False and C0.scan_kept_range(0, 3) is False
    close_all([C0, D0])
    A, B, own, theirs, stats, planes = sliced_pass(r, batches, keep=True)
    assert stats == plain_stats and stats[0] == stats[1]
    assert stats[0] == {"reads_processed": r.c.counters["load_reads_processed"], "unambiguous_reads": r.c.counters["load_unambiguous"],
                        "kmers": r.lst.kmers, "to_bloo2": r.lst.to_bloo2}
    for (p, n), want in zip(planes, plain):
        assert np.array_equal(rd.read(A, p, n), want), "fail planes differ from those of a pass that keeps no reads"
    for ctx in (A, B):
        assert_filters_are_the_references(ctx, r)
    # A packed every batch: it holds every batch's offsets.  B holds none yet
    assert A.scan_kept_state()["complete"] is True and A.scan_kept_range(0, 3, longest) is True
    assert A.load_slice_packed_reads(own[0]).max_read_len == longest
    assert B.scan_kept_state()["complete"] is False and B.scan_kept_range(0, 3, longest) is False and B.scan_kept_range(0, 0) is True
    B.scan_begin()
    with pytest.raises(api.FaucetGpuError, match=STATE):
        B.scan_batch_kept(0)                                 # resident, but without its read offsets
    with pytest.raises(api.FaucetGpuError, match=STATE):
        B.scan_prepare_kept(2)
    B.scan_end()
    with pytest.raises(api.FaucetGpuError, match=STATE):
        B.load_slice_packed_reads(theirs[0])                 # not packed here, nothing adopted
    hand_offsets(A, own[1], B, theirs[1], longest)           # in any order; a range is complete once all of ITS batches have theirs
    assert B.scan_kept_range(1, 2, longest) is True and B.scan_kept_range(0, 2, longest) is False
    hand_offsets(A, own[2], B, theirs[2], longest)
    hand_offsets(A, own[0], B, theirs[0], longest)
    B.synchronize()
    assert B.scan_kept_range(0, 3, longest) is True and B.scan_kept_state()["complete"] is True
    assert B.scan_kept_state()["n_reads"] == len(r.offs) - 1
    with pytest.raises(api.FaucetGpuError, match=STATE):
        B.load_slice_expect_reads(theirs[0])                 # it has them already
    B.scan_resident_base(2)                                  # does not shift the index of a kept scan
    for ctx in (B, A):
        set_pair_filters(ctx, r)
        sst, lists = scan_kept(ctx, sizes)
        assert_scan_is_the_references(ctx, r, sst, lists)
        assert sst["valid_reused"] == r.lst.to_bloo2 > 0     # the sure planes are those of the plain pass: every routed occurrence is reused
        sst2, lists2 = scan_kept_two_step(ctx, sizes)
        assert_scan_is_the_references(ctx, r, sst2, lists2)
        assert sst2["valid_reused"] == r.lst.to_bloo2
    with pytest.raises(api.FaucetGpuError, match=ARG):
        B.scan_begin()
        try:
            B.scan_prepare_kept(3)
        finally:
            B.scan_end()
    close_all([A, B])
    rd.close()


# ---- 2. the check of adopted offsets ---------------------------------------------------------------------------------------------------------
def equal_thirds(r):
    """three batches of which the first two hold the same number of reads (of different lengths: ragged_k31)"""
    n = len(r.offs) - 1
    m = n // 3
    return [api.ReadBatch(r.bases, r.offs[a:b + 1].copy()) for a, b in ((0, m), (m, 2 * m), (2 * m, n))]


def clean_read(r, first, last):
    """index (within the batch) of a read of the batch [first, last) that is not empty and all A/C/G/T: its first stream position is good"""
    raw = r.bases.tobytes()
    for i in range(first + 1, last):
        s = raw[int(r.offs[i]):int(r.offs[i + 1])]
        if s and not s.strip(b"ACGT"):
            return i - first
    raise AssertionError("no clean read in the batch")


def fill_and_adopt(B, wr, blocks, arrays, longest):
    """every allocation filled first (the writer waits for the context, and a wait reports a failed check), then all of them adopted"""
    filled = []
    for pk, arr in zip(blocks, arrays):
        dst = B.load_slice_expect_reads(pk)
        wr.write(B, dst.offsets_dev, arr.tobytes())
        dst.max_read_len = longest
        filled.append(dst)
    for pk, dst in zip(blocks, filled):
        B.load_slice_adopt_reads(pk, dst)


@pytest.mark.parametrize("damage", ["swapped", "one raised by 1", "first is 1", "last lowered", "one is 2^40"])
def test_adopted_offsets_that_are_not_their_blocks_are_reported(damage):
    r = ref("ragged_k31")
    batches = equal_thirds(r)
    sizes = [b.n_reads for b in batches]
    assert sizes[0] == sizes[1] and len(set(np.diff(r.offs).tolist())) > 2
    longest = int(np.diff(r.offs).max())
    lib = L.load()
    rd, wr = Reader(), Writer()
    A, B, own, theirs, _, _ = sliced_pass(r, batches, keep=True)
    true = [rd.read(A, A.load_slice_packed_reads(pk).offsets_dev, (pk.n_reads + 1) * 8).view(np.uint64).copy() for pk in own]
    for t, b in zip(true, batches):
        assert t[0] == 0 and np.array_equal(t, b.offsets - b.offsets[0])
    given = [t.copy() for t in true]
    first_bad = 1
    if damage == "swapped":
        given[0], given[1] = given[1], given[0]
        assert not np.array_equal(given[0], given[1])
        first_bad = 0
    elif damage == "one raised by 1":
        m = sizes[0]
        given[1][clean_read(r, m, 2 * m)] += 1               # the "separator" in front of that read is then the read's first base
    elif damage == "first is 1":
        given[1][0] = 1
    elif damage == "last lowered":
        given[1][-1] -= 1
    else:
        given[1][sizes[1] // 2] = 1 << 40                    # far beyond the block: compared with T, never used as an index
    fill_and_adopt(B, wr, theirs, given, longest)
    assert lib.fgpu_synchronize(B.h) == L.ERR_ARG            # the next synchronising call
    msg = lib.fgpu_last_error(B.h).decode()
    assert f"batch {first_bad} " in msg and "offsets" in msg, msg
    assert lib.fgpu_synchronize(B.h) == L.OK                 # reported once; the context goes on
    assert B.scan_kept_range(0, 3, longest) is False         # what was adopted since the last look has been dropped again
    B.scan_begin()
    with pytest.raises(api.FaucetGpuError, match=STATE):
        B.scan_batch_kept(first_bad)
    B.scan_end()
    # the same allocations, filled with the true offsets: a clean run in the same process, on the same context
    fill_and_adopt(B, wr, theirs, true, longest)
    assert B.scan_kept_range(0, 3, longest) is True
    set_pair_filters(B, r)
    sst, lists = scan_kept(B, sizes)
    assert_scan_is_the_references(B, r, sst, lists)
    close_all([A, B])                                        # (and a context that has reported the error is destroyed like any other)
    rd.close()
    wr.close()


# ---- 3. state and argument errors, the budget ------------------------------------------------------------------------------------------------
def test_keep_reads_state_errors_and_the_budget():
    lib = L.load()
    tai = 1 << 19
    line = b"ACGTTGCAAGGCTTAACCGGTTACGATCGATCGGATCGATTAGCTAGCTAGGCTAGCTAGGATCGATCGAT"
    batch = api.ReadBatch.from_lines([line] * 40)
    kr, pk = L.KeptReads(), L.Packed()
    ctx = api.Context(21, tai, 3)
    assert lib.fgpu_load_slice_keep_reads(ctx.h) == L.ERR_STATE           # outside a sliced pass
    ctx.load_begin()
    assert lib.fgpu_load_slice_keep_reads(ctx.h) == L.ERR_STATE           # inside a plain one
    ctx.load_end()
    ctx.load_slice_begin(0, tai)
    first = ctx.load_slice_pack(batch)
    assert lib.fgpu_load_slice_keep_reads(ctx.h) == L.ERR_STATE           # after the pass' first block
    assert lib.fgpu_load_slice_packed_reads(ctx.h, C.byref(first), C.byref(kr)) == L.ERR_STATE      # a pass that keeps no reads
    ctx.load_slice_batch_packed(first)
    ctx.load_slice_commit()
    ctx.load_slice_end()
    ctx.load_slice_begin(0, tai)
    ctx.load_slice_keep_reads()
    assert lib.fgpu_load_slice_packed_reads(ctx.h, None, C.byref(kr)) == L.ERR_ARG
    own = ctx.load_slice_pack(batch)
    got = ctx.load_slice_packed_reads(own)
    assert got.n_reads == 40 and got.offsets_dev and got.max_read_len == 0              # the longest read is known once the pass has ended
    other = ctx.load_slice_expect(own.T, own.n_reads)
    dst = ctx.load_slice_expect_reads(other)
    assert ctx.load_slice_expect_reads(other).offsets_dev == dst.offsets_dev            # the same allocation until it is adopted
    assert lib.fgpu_load_slice_adopt_reads(ctx.h, C.byref(other), C.byref(dst)) == L.ERR_STATE      # the block has not been loaded
    assert lib.fgpu_device_copy(ctx.h, other.block_dev, own.block_dev, own.nbytes) == 0
    ctx.load_slice_batch_packed(own)
    ctx.load_slice_batch_packed(other)
    wrong = L.KeptReads(got.offsets_dev, 40, 0)
    assert lib.fgpu_load_slice_adopt_reads(ctx.h, C.byref(other), C.byref(wrong)) == L.ERR_ARG      # another allocation
    assert lib.fgpu_device_copy(ctx.h, dst.offsets_dev, got.offsets_dev, 41 * 8) == 0
    ctx.load_slice_adopt_reads(other, dst)
    ctx.load_slice_commit()
    assert ctx.load_slice_end()["reads_processed"] == 80                  # (a synchronising call: the check passed)
    assert ctx.load_slice_packed_reads(own).max_read_len == len(line)
    assert ctx.scan_kept_range(0, 2, len(line)) is True and ctx.scan_kept_range(0, 3) is False
    empty = L.Packed()
    assert ctx.load_slice_packed_reads(empty).offsets_dev is None         # a batch without reads has neither block nor offsets
    # fgpu_load_slice_batch keeps its batch's offsets the same way (counted from 0, whatever offsets[0] was): the batch can be scanned
    shifted = api.ReadBatch(batch.bases, batch.offsets[20:].copy())
    ctx.load_slice_begin(0, tai)
    ctx.load_slice_keep_reads()
    ctx.load_slice_batch(shifted)
    ctx.load_slice_commit()
    assert ctx.load_slice_end()["reads_processed"] == 20
    assert ctx.scan_kept_state()["complete"] is True and ctx.scan_kept_range(0, 1, len(line)) is True
    ctx.scan_begin()
    assert ctx.scan_batch_kept(0) == 20
    kept_scan = ctx.scan_end()
    ctx.scan_begin()
    ctx.scan_batch(shifted)
    text_scan = ctx.scan_end()
    for key in ("reads_processed", "unambiguous_reads", "kmers", "n_junctions", "nb_processed", "nb_skipped", "nb_jcheck_kmer", "nb_no_juncs"):
        assert kept_scan[key] == text_scan[key], key
    ctx.load_begin()                                                      # the next load pass forgets all of it
    ctx.load_end()
    assert lib.fgpu_load_slice_packed_reads(ctx.h, C.byref(own), C.byref(kr)) == L.ERR_STATE
    assert ctx.scan_kept_range(0, 1) is False
    ctx.close()
    # the offsets are charged to the resident budget with the block: without room the message names the numbers
    lean = api.Context(21, tai, 3, keep_resident=False)
    lean.load_slice_begin(0, tai)
    lean.load_slice_keep_reads()
    s = batch.c_struct()
    assert lib.fgpu_load_slice_pack(lean.h, C.byref(s), C.byref(pk)) == L.ERR_NOMEM
    err = lib.fgpu_last_error(lean.h)
    assert b"budget" in err and str(41 * 8).encode() in err and b"read offsets" in err
    lean.close()
