"""Pass 0 that keeps what it packs, and the plain pass 1 that loads from it (fgpu_estimate_keep / _keep_state / _take_kept,
fgpu_load_batch_packed): keeping changes no counter of the sketch, the kept blocks are byte for byte the blocks of the sliced pass, they outlive
the placeholder context, and a load from them is the load of the reads -- the reference's .bloom, the oracle's bloo1 and stats, and a scan
behind it that still finds its load batches.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from tests import estimate_ref as R
from tests.test_gpu_estimate import assert_counts, placeholder, refused, sketch
from tests.test_gpu_parity import chunks
from tests.test_gpu_slices_packed import PADW, Reader, batches_of, golden

pytestmark = pytest.mark.gpu

GOLDENS = ["c1_k21", "ragged_k31", "pe_fastq_k21", "mercy_k21"]
BITS = 14
NO_LIMIT = 1 << 62


def charged(T):
    """what a kept block of T stream positions costs the budget: 4 bits per position of the padded planes"""
    return 4 * ((T + 63) // 64 + PADW) * 8


def block_bytes(T):
    return 24 * ((T + 63) // 64 + PADW) + 16


def keep_pass(ctx, batches, budget=NO_LIMIT, r_bits=BITS):
    ctx.estimate_begin(r_bits)
    ctx.estimate_keep(budget)
    for b in batches:
        ctx.estimate_batch(b)
    return ctx.estimate_end()


def kept_blocks(k, batches):
    """the blocks of `batches` from a placeholder context that is gone when they are used"""
    ctx = placeholder(k)
    keep_pass(ctx, batches)
    blocks = ctx.estimate_take_kept()
    ctx.close()
    return blocks


def free_blocks(ctx, blocks):
    for pk in blocks:
        assert ctx.lib.fgpu_device_free(ctx.h, pk.block_dev) == 0


def stream_T(batch):
    offs = batch.offsets
    return int(offs[-1] - offs[0]) + len(offs) - 1


def with_an_empty_batch(bases, offs):
    three = batches_of(bases, offs, 3)
    return [three[0], api.ReadBatch(bases, three[0].offsets[-1:].copy()), three[1], three[2]]


def batches_for(bases, offs, shape):
    return with_an_empty_batch(bases, offs) if shape == "empty_in_the_middle" else batches_of(bases, offs, shape)


def device_free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


# ---- 1. keeping changes neither the sketch nor the packing ------------------------------------------------------------------------------
@pytest.mark.parametrize("n_batches", [1, 3])
@pytest.mark.parametrize("name", GOLDENS)
def test_keeping_changes_no_counter_and_the_blocks_are_the_sliced_pass_blocks(name, n_batches):
    c, bases, offs, tai, nh, _, _, _ = golden(name)
    batches = batches_of(bases, offs, n_batches)
    want = R.golden_counts(name, BITS)
    ctx = placeholder(c.k)
    plain = sketch(ctx, batches, BITS)
    assert ctx.estimate_keep_state() == (False, 0, 0)
    ctx.estimate_begin(BITS)
    ctx.estimate_keep(NO_LIMIT)
    total = 0
    for i, b in enumerate(batches):
        ctx.estimate_batch(b)
        total += charged(stream_T(b))
        assert ctx.estimate_keep_state() == (True, i + 1, total)
    kept = ctx.estimate_end()
    assert kept == plain
    assert_counts(kept, want, BITS)
    assert ctx.estimate_keep_state() == (True, len(batches), total)         # valid after the end, until the blocks are taken
    blocks = ctx.estimate_take_kept()
    assert ctx.estimate_keep_state() == (False, 0, 0)
    assert [(pk.T, pk.n_reads, pk.nbytes) for pk in blocks] == [(stream_T(b), len(b.offsets) - 1, block_bytes(stream_T(b))) for b in batches]
    # the same batches through fgpu_load_slice_pack of a one-slice pass: planes, padding words, trailer digest and T
    rd = Reader()
    packer = api.Context(c.k, tai, nh)
    packer.load_slice_begin(0, tai)
    for b, pk in zip(batches, blocks):
        ref = packer.load_slice_pack(b)
        assert (ref.T, ref.n_reads, ref.nbytes) == (pk.T, pk.n_reads, pk.nbytes)
        a, z = rd.read(ctx, pk.block_dev, pk.nbytes), rd.read(packer, ref.block_dev, ref.nbytes)
        assert np.array_equal(a, z), "a kept block differs from the sliced pass' block"
        assert int(a[-8:].view(np.uint64)[0]) == pk.T
    free_blocks(ctx, blocks)
    packer.close()
    ctx.close()
    rd.close()


# ---- 2. across contexts: the blocks outlive the placeholder, the load is the load of the reads -----------------------------------------------
def load_packed(ctx, items):
    """one plain pass: L.Packed items through load_batch_packed, ReadBatch items through load_batch"""
    ctx.load_begin()
    for it in items:
        (ctx.load_batch_packed if isinstance(it, L.Packed) else ctx.load_batch)(it)
    return ctx.load_end()


def assert_load_is_the_oracles(ctx, c, st, b1, b2, lst):
    assert np.array_equal(ctx.bloom_download(L.BLOO2), c.bloom()), "bloo2 differs from the reference's .bloom file"
    assert np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits())
    assert st == {"reads_processed": c.counters["load_reads_processed"], "unambiguous_reads": c.counters["load_unambiguous"], "kmers": lst.kmers,
                  "to_bloo2": lst.to_bloo2}


@pytest.mark.parametrize("shape", [1, 3, "empty_in_the_middle"])
@pytest.mark.parametrize("name", GOLDENS)
def test_a_new_context_loads_what_the_placeholder_kept(name, shape):
    c, bases, offs, tai, nh, b1, b2, lst = golden(name)
    batches = batches_for(bases, offs, shape)
    blocks = kept_blocks(c.k, batches)
    assert len(blocks) == sum(1 for b in batches if len(b.offsets) > 1)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer, mercy=c.mercy)
    st = load_packed(ctx, blocks)
    assert_load_is_the_oracles(ctx, c, st, b1, b2, lst)
    # the scan of the same reads pairs its batches with the adopted blocks and takes the routed occurrences from their `sure` planes
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(batches)
    keys, recs = sc.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines())
    assert sst["n_junctions"] == c.counters["distinct_junctions"] and sst["nb_processed"] == c.counters["nb_processed"]
    assert sst["valid_reused"] > 0
    if not c.mercy:
        assert sst["valid_reused"] == lst.to_bloo2
    ctx.close()


# ---- 3. word edges ------------------------------------------------------------------------------------------------------------------------
def edge_batch(T, seed):
    """three reads whose stream has T positions: one with Ns inside (its tokens are laid out in reverse order), one shorter than k, one filler"""
    rng = np.random.default_rng(seed)
    with_n = b"ACGTTGCAGATTACAG" + b"NN" + b"CCGTATTGACCAGTA"      # k-mers on both sides of the Ns
    short = b"ACG"
    filler = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), T - 3 - len(with_n) - len(short)))
    b = api.ReadBatch.from_lines([with_n, short, filler])
    assert stream_T(b) == T
    return b


@pytest.mark.parametrize("T", [63, 64, 65, 129])
def test_streams_that_end_at_and_around_a_word_edge(T):
    k, tai, nh = 15, 1 << 12, 2
    batches = [edge_batch(T, 1), edge_batch(T, 2)]          # the second batch meets a carry
    blocks = kept_blocks(k, batches)
    assert [pk.T for pk in blocks] == [T, T]
    a, z = api.Context(k, tai, nh), api.Context(k, tai, nh)
    sa, sz = load_packed(a, blocks), load_packed(z, batches)
    assert sa == sz and sa["reads_processed"] == 6 and sa["kmers"] > 0
    for which in (L.BLOO1, L.BLOO2):
        assert np.array_equal(a.bloom_download(which), z.bloom_download(which))
    # `sure` is not handed out: a scan of the same reads reads it, and must reuse the same occurrences on both
    ra, rz = api.ReadScanner(a).scanReads(batches), api.ReadScanner(z).scanReads(batches)
    assert ra == rz and ra["valid_reused"] == sa["to_bloo2"]
    a.close()
    z.close()


# ---- 4. one pass that mixes reads and blocks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_k31", "mercy_k21"])
def test_a_pass_that_mixes_reads_and_blocks(name):
    c, bases, offs, tai, nh, b1, b2, lst = golden(name)
    five = chunks(bases, offs, 5)
    blocks = kept_blocks(c.k, [five[1], five[3]])
    ctx = api.Context(c.k, tai, nh, mercy=c.mercy)
    st = load_packed(ctx, [five[0], blocks[0], five[2], blocks[1], five[4]])
    assert_load_is_the_oracles(ctx, c, st, b1, b2, lst)
    sst = api.ReadScanner(ctx).scanReads(five)
    assert sst["n_junctions"] == c.counters["distinct_junctions"] and sst["valid_reused"] > 0
    ctx.close()


# ---- 5. nothing kept resident, nothing leaked -------------------------------------------------------------------------------------------------
def big_batch(n_reads=40000, length=150, seed=5):
    """6 M bases: a block of 2.3 MB, so that one that is not given back shows in the device's free memory"""
    rng = np.random.default_rng(seed)
    mat = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n_reads, length))
    return api.ReadBatch.from_matrix(mat)


LEAK_ROUNDS = 4          # a leaked block per round would be 9 MB in all; other users of the device move the figure too: half of that is the bar
LEAK_BAR = 2 * block_bytes(40000 * 151)


def test_a_context_that_keeps_nothing_resident_gives_the_block_back():
    c, bases, offs, tai, nh, b1, b2, lst = golden("c1_k21")
    batches = batches_of(bases, offs, 3)
    ctx = api.Context(c.k, tai, nh, keep_resident=False)
    st = load_packed(ctx, kept_blocks(c.k, batches))
    assert_load_is_the_oracles(ctx, c, st, b1, b2, lst)
    assert api.ReadScanner(ctx).scanReads(batches)["valid_reused"] == 0
    # blocks large enough to be seen: after load_end the device is where a plain load of the same reads leaves it
    big = big_batch()
    load_packed(ctx, [big])
    before = device_free_bytes()
    for _ in range(LEAK_ROUNDS):
        load_packed(ctx, kept_blocks(c.k, [big]))
    assert before - device_free_bytes() < LEAK_BAR
    ctx.close()


def test_blocks_nobody_took_go_with_the_context_or_the_next_pass():
    big = big_batch()
    ctx = placeholder(21)
    for _ in range(2):                       # warm: host batches go through two staging sets in turn, both are as large as they get
        keep_pass(ctx, [big])
        free_blocks(ctx, ctx.estimate_take_kept())
    before = device_free_bytes()
    for _ in range(LEAK_ROUNDS):             # never taken: the next estimate_begin releases them
        keep_pass(ctx, [big])
    keep_pass(ctx, [])
    assert ctx.estimate_keep_state() == (True, 0, 0)
    assert before - device_free_bytes() < LEAK_BAR
    ctx.close()
    before = device_free_bytes()
    for _ in range(LEAK_ROUNDS):             # destroyed with untaken blocks, and destroyed inside a keeping pass
        ctx = placeholder(21)
        keep_pass(ctx, [big])
        ctx.close()
        ctx = placeholder(21)
        ctx.estimate_begin(BITS)
        ctx.estimate_keep(NO_LIMIT)
        ctx.estimate_batch(big)
        ctx.close()
    assert before - device_free_bytes() < LEAK_BAR


# ---- 6. the budget ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget_blocks", [1, 0])
def test_a_batch_beyond_the_budget_ends_the_keeping_not_the_pass(budget_blocks):
    c, bases, offs, _, _, _, _, _ = golden("c1_k21")
    batches = batches_of(bases, offs, 3)
    budget = budget_blocks * max(charged(stream_T(b)) for b in batches)
    stops_at = 1 if budget_blocks else 0
    ctx = placeholder(c.k)
    ctx.estimate_begin(BITS)
    ctx.estimate_keep(budget)
    for i, b in enumerate(batches):
        ctx.estimate_batch(b)
        assert ctx.estimate_keep_state() == ((True, i + 1, sum(charged(stream_T(x)) for x in batches[:i + 1])) if i < stops_at else (False, 0, 0))
    assert_counts(ctx.estimate_end(), R.golden_counts("c1_k21", BITS), BITS)
    out, n = (L.Packed * 4)(), C.c_uint64(7)
    refused(ctx, L.ERR_NOMEM, ctx.lib.fgpu_estimate_take_kept, out, 4, C.byref(n))
    msg = ctx.lib.fgpu_last_error(ctx.h).decode()
    assert n.value == 0 and str(budget) in msg and str(charged(stream_T(batches[stops_at]))) in msg, msg
    assert_counts(sketch(ctx, batches, BITS), R.golden_counts("c1_k21", BITS), BITS)      # the next pass is an ordinary one
    ctx.close()


# ---- 7. state and argument errors ------------------------------------------------------------------------------------------------------------
def test_keep_and_take_keep_to_their_places():
    c, bases, offs, tai, nh, _, _, _ = golden("c1_k21")
    lib = L.load()
    batches = batches_of(bases, offs, 3)
    ctx = placeholder(c.k)
    out, n = (L.Packed * 4)(), C.c_uint64(0)
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_keep, NO_LIMIT)                           # outside a pass
    ctx.estimate_begin(BITS)
    ctx.estimate_batch(batches[0])
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_keep, NO_LIMIT)                           # after the first batch
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_take_kept, out, 4, C.byref(n))            # inside a pass
    ctx.estimate_end()
    assert ctx.estimate_take_kept() == []                                                 # a pass that was never asked to keep
    keep_pass(ctx, batches)
    refused(ctx, L.ERR_ARG, lib.fgpu_estimate_take_kept, out, 2, C.byref(n))              # cap too small: counted, nothing taken
    assert n.value == 3 and ctx.estimate_keep_state()[1] == 3
    assert lib.fgpu_estimate_take_kept(ctx.h, out, 4, C.byref(n)) == 0 and n.value == 3
    assert lib.fgpu_estimate_keep_state(ctx.h, None, None, None) == 0
    free_blocks(ctx, list(out)[:3])
    ctx.close()


def test_a_sketch_too_full_still_hands_out_its_blocks():
    """fgpu_estimate_end answers FGPU_ERR_CAPACITY (6 M random 21-mers in 2^8 cells per level): the pass is over, and what it kept is there to take"""
    big = big_batch()
    ctx = placeholder(21)
    ctx.estimate_begin(8)
    ctx.estimate_keep(NO_LIMIT)
    ctx.estimate_batch(big)
    with pytest.raises(api.FaucetGpuError, match="raise r_bits"):
        ctx.estimate_end()
    assert ctx.estimate_keep_state() == (True, 1, charged(stream_T(big)))
    blocks = ctx.estimate_take_kept()
    assert [(pk.T, pk.n_reads) for pk in blocks] == [(stream_T(big), 40000)]
    kmers = ctx.last_estimate["kmers"]
    ctx.close()
    loader = api.Context(21, 1 << 24, 3)
    st = load_packed(loader, blocks)
    assert st["kmers"] == kmers == 40000 * 130 and st["reads_processed"] == 40000
    loader.close()


def test_load_batch_packed_refuses_what_it_cannot_load():
    import torch
    c, bases, offs, tai, nh, b1, b2, lst = golden("c1_k21")
    lib = L.load()
    batches = batches_of(bases, offs, 3)
    blocks = kept_blocks(c.k, batches)
    ctx = api.Context(c.k, tai, nh)
    pk = blocks[0]
    refused(ctx, L.ERR_STATE, lib.fgpu_load_batch_packed, C.byref(pk))                    # outside a pass
    ctx.load_slice_begin(0, tai)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_batch_packed, C.byref(pk))                    # in a sliced pass
    ctx.load_slice_commit()
    ctx.load_slice_end()
    ctx.load_begin(shard_times=True)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_batch_packed, C.byref(pk))                    # in a read shard's pass
    ctx.load_end()
    ctx.load_begin()
    for field, value in (("nbytes", pk.nbytes + 8), ("T", pk.T + 64), ("T", 1 << 40), ("n_reads", pk.T + 1)):
        bad = L.Packed(pk.block_dev, pk.nbytes, pk.T, pk.n_reads)
        setattr(bad, field, value)
        refused(ctx, L.ERR_ARG, lib.fgpu_load_batch_packed, C.byref(bad))
    refused(ctx, L.ERR_ARG, lib.fgpu_load_batch_packed, C.byref(L.Packed(None, 0, 5, 0)))  # no block: all zeros or nothing
    ctx.load_batch_packed(L.Packed())                                                     # ... which does nothing
    st = ctx.load_end()
    assert st["reads_processed"] == 0 and st["kmers"] == 0
    # refused blocks are still the caller's, and still good
    st = load_packed(ctx, blocks)
    assert_load_is_the_oracles(ctx, c, st, b1, b2, lst)

    # a block with one word zeroed, and one whose trailer holds another T: FGPU_ERR_ARG from load_end
    for damage in ("word", "trailer"):
        blocks = kept_blocks(c.k, batches)
        victim = blocks[1]
        if damage == "word":
            at = next(w for w in range(8, 64) if word_is_set(ctx, victim, w))
            assert lib.fgpu_device_zero(ctx.h, victim.block_dev + 8 * at, 8) == 0
        else:
            other = torch.tensor([victim.T - 1], dtype=torch.int64).cuda()
            torch.cuda.synchronize()
            assert lib.fgpu_device_copy(ctx.h, victim.block_dev + victim.nbytes - 8, other.data_ptr(), 8) == 0
        ctx.load_begin()
        for b in blocks:
            ctx.load_batch_packed(b)
        e = L.LoadStats()
        refused(ctx, L.ERR_ARG, lib.fgpu_load_end, C.byref(e))
        assert "trailer" in lib.fgpu_last_error(ctx.h).decode()
    ctx.close()


def word_is_set(ctx, pk, w):
    """word w of a block, through a device-to-host copy by torch (non-zero words can be zeroed visibly)"""
    import torch
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.synchronize()
    assert ctx.lib.fgpu_device_copy(ctx.h, t.data_ptr(), pk.block_dev + 8 * w, 8) == 0
    ctx.synchronize()
    return int(t.cpu()[0]) != 0
