"""The long pair filter's SPARSE state (fgpu_scan_long_pairs, FGPU_LONG_PAIRS_FILTER_SPARSE; faucet_amd/csrc/pairs.hip): the first-set times of
the check-then-insert fixed point kept in a per-batch table keyed by bit position instead of 4 bytes per filter bit.  Same fixed point, so
the same filter, counts and diagnostics as the dense form and the oracle -- whatever the batching, on filters small enough that most items
are decided by what earlier items of the batch inserted, with bit positions beyond 32 bits, through a replay, and from the Python host.
Needs an MI355X."""
import functools

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from oracle import pyoracle as po
from tests.test_gpu_parity import _paired_oracle, _pairs_in_repeats, _random_case, _scan_equals_oracle, chunks

pytestmark = pytest.mark.gpu

K, E, S = 21, 400_000, 150_000
SPARSE = 3


@functools.lru_cache(maxsize=None)
def _recipe(n_pairs, seed):
    """R(n, seed): read pairs in planted repeats, the main filters loaded by the oracle, the oracle's scan with both pair filters as the CLI
    would size them.  Computed once per (n, seed); nobody writes to it."""
    bases, offs = _pairs_in_repeats(n_pairs, seed)
    tai, nh = api.load_filter_shape(E, S)
    b2, short, long_, osc = _paired_oracle(bases, offs, K, tai, nh, E)
    return dict(bases=bases, offs=offs, tai=tai, nh=nh, b2=b2, short=short, long=long_, osc=osc, ost=osc.stats())


def _context(d, long_shape, mode, short=True):
    ctx = api.Context(K, d["tai"], d["nh"], record_stops=True)
    ctx.bloom_upload(L.BLOO2, d["b2"].bits())
    if short:
        ctx.scan_short_pairs(d["short"].tai, d["short"].n_hash, False)
    ctx.scan_long_pairs(long_shape[0], long_shape[1], mode)
    return ctx


def _scan(ctx, batches):
    ctx.scan_begin()
    for b in batches:
        ctx.scan_batch(b)
    sst = ctx.scan_end()
    assert ctx.take_stops() is None
    return sst


def _is_sparse_and_clean(ctx):
    st = ctx.diag_long_pairs_state()
    assert st["form"] == "sparse" and st["error"] == 0, st
    slots = st["table_slots_high"]
    assert slots > 0 and slots & (slots - 1) == 0, st
    return st


def _equals_case_one(ctx, d, batches):
    """what case 1 asks of a sparse context: both filters and the two counts are the oracle's"""
    long_, ost = d["long"], d["ost"]
    sst = _scan(ctx, batches)
    bits, empty, not_empty = ctx.scan_long_pairs_download(long_.tai)
    assert (empty, not_empty) == (ost["empty_count"], ost["not_empty_count"])
    assert bits.any() and np.array_equal(bits, long_.bits())
    assert np.array_equal(ctx.scan_short_pairs_download(d["short"].tai), d["short"].bits())
    return sst


@pytest.mark.parametrize("n_chunks", [1, 4, 7])
def test_sparse_state_equals_the_oracle_and_the_dense_form(n_chunks):
    """an odd number of pairs; 7 chunks cut pairs in two (first ends wait for the next batch).  Two scans in a row: the second starts from
    an empty filter.  The dense context is fed the same chunks: same fixed point, so the same items, inserts, rounds and most rounds."""
    d = _recipe(4001, 5)
    shape = (d["long"].tai, d["long"].n_hash)
    batches = chunks(d["bases"], d["offs"], n_chunks)
    sparse, dense = _context(d, shape, SPARSE), _context(d, shape, 2)
    assert dense.diag_long_pairs_state()["form"] == "dense"
    for attempt in range(2):
        sst = _equals_case_one(sparse, d, batches)
        _scan(dense, batches)
        assert np.array_equal(dense.scan_long_pairs_download(shape[0])[0], d["long"].bits())
        ds, dd = sparse.diag_long_pairs(), dense.diag_long_pairs()
        assert ds == dd and ds["items"] > 0 and ds["inserts"] > 0, (ds, dd)
        _is_sparse_and_clean(sparse)
    _scan_equals_oracle(sparse, sst, d["osc"])
    sparse.close()
    dense.close()


@functools.lru_cache(maxsize=None)
def _oracle_long(n_pairs, seed, tai, n_hash):
    """the oracle's scan of R(n, seed) with a long pair filter of the given shape: (filter, stats)"""
    d = _recipe(n_pairs, seed)
    short, long_ = po.Bloom(d["short"].tai, d["short"].n_hash), po.Bloom(tai, n_hash)
    osc = po.Scanner(K, 1, 100, d["b2"], short_pf=short, long_pf=long_)
    osc.scan_reads(d["bases"], d["offs"], paired_ends=True, no_cleaning=False)
    return long_, osc.stats(), osc


def _by_reads(bases, offs, per_batch):
    n = len(offs) - 1
    return [api.ReadBatch(bases, offs[a:min(a + per_batch, n) + 1].copy()) for a in range(0, n, per_batch)]


@pytest.mark.parametrize("tai_log2,n_hash,reads_per_batch", [(10, 1, 0), (12, 2, 0), (14, 3, 0), (16, 6, 0), (18, 32, 0), (12, 2, 7)],
                         ids=lambda v: str(v))
def test_small_filters_where_earlier_inserts_of_the_batch_decide(tai_log2, n_hash, reads_per_batch):
    """filters between a fifth and 85 % full at the end: most checks are answered by bits that items of the same batch set, so by the table.
    Five chunks; (2^12, 2) also in batches of 7 reads: tables of the minimum size whose probes wrap, a waiting first end in every other
    batch."""
    d = _recipe(1501, 5)
    tai = 1 << tai_log2
    long_, ost, _ = _oracle_long(1501, 5, tai, n_hash)
    weight = int(np.unpackbits(long_.bits()).sum()) / tai
    print(f"oracle's long pair filter 2^{tai_log2} x {n_hash}: weight {weight:.3f}")
    assert 0.2 <= weight <= 0.85, weight
    batches = _by_reads(d["bases"], d["offs"], reads_per_batch) if reads_per_batch else chunks(d["bases"], d["offs"], 5)
    ctx = _context(d, (tai, n_hash), SPARSE)
    _scan(ctx, batches)
    bits, empty, not_empty = ctx.scan_long_pairs_download(tai)
    assert (empty, not_empty) == (ost["empty_count"], ost["not_empty_count"])
    assert np.array_equal(bits, long_.bits())
    _is_sparse_and_clean(ctx)
    if reads_per_batch:
        assert len(batches) > 400
    ctx.close()


def test_sparse_state_with_ragged_reads_and_empty_records():
    """reads with N (several pieces per read), empty records between them (each still toggles firstEnd) and a batch without a single valid
    piece: the recipe of test_long_pair_filter_with_ragged_reads_and_empty_records"""
    k, e_, s_ = 25, 1_000_000, 200_000
    bases, offs = _random_case(12001, 110, k, 30000, 0.012, 99, 0.003, 3)
    lines = [bytes(bases[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]
    for at in (5, 6, 400, 2001, 2002, 2003, 9000):
        lines.insert(at, b"")
    junk = [b"NNNN", b"", b"ACGTN"] * 7
    batches = [api.ReadBatch.from_lines(x) for x in (lines[:3001], junk, lines[3001:3002], lines[3002:])]
    whole = api.ReadBatch.from_lines(lines[:3001] + junk + lines[3001:])
    tai, nh = api.load_filter_shape(e_, s_)
    b2, short, long_, osc = _paired_oracle(whole.bases, whole.offsets, k, tai, nh, e_)
    ost = osc.stats()
    ctx = api.Context(k, tai, nh, record_stops=True)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    ctx.scan_short_pairs(short.tai, short.n_hash, False)
    ctx.scan_long_pairs(long_.tai, long_.n_hash, SPARSE)
    _scan(ctx, batches)
    bits, empty, not_empty = ctx.scan_long_pairs_download(long_.tai)
    assert (empty, not_empty) == (ost["empty_count"], ost["not_empty_count"])
    assert bits.any() and np.array_equal(bits, long_.bits())
    _is_sparse_and_clean(ctx)
    ctx.close()


def test_bit_positions_beyond_32_bits():
    """a 2^33-bit filter: its keys do not fit 32 bits, and the dense form would need 32 GiB of first-set times beside the 1 GiB of bits"""
    d = _recipe(1501, 5)
    tai, n_hash = 1 << 33, 6
    long_, ost, _ = _oracle_long(1501, 5, tai, n_hash)
    ctx = _context(d, (tai, n_hash), SPARSE, short=False)
    _scan(ctx, chunks(d["bases"], d["offs"], 3))
    bits, empty, not_empty = ctx.scan_long_pairs_download(tai)
    assert (empty, not_empty) == (ost["empty_count"], ost["not_empty_count"])
    want = long_.bits()
    assert want[1 << 29:].any(), "no bit beyond position 2^32 in the oracle's filter"
    assert np.array_equal(bits, want)
    st = _is_sparse_and_clean(ctx)
    assert st["working_bytes"] < 1 << 30, st
    ctx.close()
    _oracle_long.cache_clear()          # (1 GiB of host memory)


def test_auto_takes_the_sparse_state_only_where_the_dense_one_does_not_fit(monkeypatch):
    d = _recipe(4001, 5)
    shape = (d["long"].tai, d["long"].n_hash)
    batches = chunks(d["bases"], d["offs"], 4)
    monkeypatch.setenv("FGPU_DEBUG_LONG_PAIRS_DENSE_NOMEM", "1")
    ctx = _context(d, shape, 2)
    _equals_case_one(ctx, d, batches)
    _is_sparse_and_clean(ctx)
    monkeypatch.delenv("FGPU_DEBUG_LONG_PAIRS_DENSE_NOMEM")
    ctx.scan_long_pairs(shape[0], shape[1], 2)
    assert ctx.diag_long_pairs_state()["form"] == "dense"
    monkeypatch.setenv("FGPU_LONG_PAIRS_STATE", "sparse")
    ctx.scan_long_pairs(shape[0], shape[1], 2)
    assert ctx.diag_long_pairs_state()["form"] == "sparse"
    # dense asked for, and the 4 bytes per bit "do not fit": FGPU_ERR_NOMEM as before, nothing left on the device
    monkeypatch.setenv("FGPU_LONG_PAIRS_STATE", "dense")
    monkeypatch.setenv("FGPU_DEBUG_LONG_PAIRS_DENSE_NOMEM", "1")
    assert ctx.lib.fgpu_scan_long_pairs(ctx.h, shape[0], shape[1], 2) == L.ERR_NOMEM
    assert ctx.diag_long_pairs_state()["form"] is None
    monkeypatch.setenv("FGPU_LONG_PAIRS_STATE", "neither")
    assert ctx.lib.fgpu_scan_long_pairs(ctx.h, shape[0], shape[1], 2) == L.ERR_ARG
    ctx.close()


def test_sparse_state_through_an_absorbed_overflow():
    """the recipe of tests/test_gpu_replay_consumers.py: a junction table far too small, five batches, both pair filters on the device and no
    list to the host.  The library scans its journal again; both filters and the counts are the oracle's afterwards."""
    from tests import test_gpu_replay_consumers as rc
    d = rc._data()
    batches = rc.cut(d["bases"], d["offs"], rc.CUTS)
    assert len(batches) >= 3
    ctx = api.Context(rc.K, d["tai"], d["nh"], record_stops=True, junction_capacity=rc.CAPACITY)
    ctx.bloom_upload(L.BLOO2, d["b2"].bits())
    ctx.scan_short_pairs(d["short"].tai, d["short"].n_hash, False)
    ctx.scan_long_pairs(d["long"].tai, d["long"].n_hash, SPARSE)
    sst = _scan(ctx, batches)
    assert np.array_equal(ctx.scan_short_pairs_download(d["short"].tai), d["short"].bits())
    bits, empty, not_empty = ctx.scan_long_pairs_download(d["long"].tai)
    assert bits.any() and np.array_equal(bits, d["long"].bits())
    assert (empty, not_empty) == (d["ost"]["empty_count"], d["ost"]["not_empty_count"])
    _scan_equals_oracle(ctx, sst, d["osc"])
    assert ctx.diag_scan_replays() >= 1
    _is_sparse_and_clean(ctx)
    ctx.close()


def test_python_host_hands_a_sparse_long_pair_filter_from_shard_to_shard(monkeypatch):
    """faucet_amd/sharded.py: only the filter's bits travel between the shards, so the host needs no change -- FGPU_LONG_PAIRS_STATE=sparse
    around pairs_setup is all.  Ranks in turn in one process, empty shards among them."""
    import torch
    from faucet_amd import sharded
    cuts = (0, 0, 2600, 2600, 8000)
    d = _recipe(4000, 5)
    bases, offs, short, long_, ost = d["bases"], d["offs"], d["short"], d["long"], d["ost"]
    assert len(offs) - 1 == cuts[-1]
    dev = torch.device("cuda", 0)
    shards = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        inner = sorted({lo, hi, lo + (hi - lo) // 3 | 1 if hi - lo > 3 else hi, lo + 2 * (hi - lo) // 3 if hi - lo > 3 else hi})   # odd cuts inside
        shards.append([api.ReadBatch(bases, offs[a:b + 1].copy()) for a, b in zip(inner[:-1], inner[1:]) if b > a])
    counts, forms = [], []

    def make():
        g = sharded.GpuShard(api.Context(K, d["tai"], d["nh"], record_stops=True), dev)
        monkeypatch.setenv("FGPU_LONG_PAIRS_STATE", "sparse")
        g.pairs_setup(short=(short.tai, short.n_hash), long=(long_.tai, long_.n_hash))
        monkeypatch.delenv("FGPU_LONG_PAIRS_STATE")
        forms.append(g.ctx.diag_long_pairs_state()["form"])
        return g

    def after_scan(r, stats, backend):
        counts.append(backend.pair_counts())

    lst, sst, last = sharded.run_in_turn(make, shards, "fixup", None, after_scan)
    assert forms and set(forms) == {"sparse"}
    assert (sum(c[0] for c in counts), sum(c[1] for c in counts)) == (ost["empty_count"], ost["not_empty_count"])
    assert np.array_equal(last.ctx.scan_short_pairs_download(short.tai), short.bits())
    bits, _, _ = last.ctx.scan_long_pairs_download(long_.tai)
    assert bits.any() and np.array_equal(bits, long_.bits())
    _scan_equals_oracle(last.ctx, sst, d["osc"])
    assert last.ctx.diag_long_pairs_state()["error"] == 0
    last.close()
