"""Replays that absorb a failed scan, seen from what consumes the scan's lists: scanInputRead's lists handed to the caller, the
short pair filter and the long pair filter on the device.  A walk that outgrows the junction table drops records, so its lists are wrong; the
library scans its journal again on a larger table, and none of the wrong lists may reach a consumer on the way -- not when the caller takes
lists while the scan is still running, not when a later batch reuses the buffers, not inside the replay itself.  Every case compares with the
oracle.  Needs an MI355X."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api, synth
from oracle import pyoracle as po
from tests.test_gpu_parity import _oracle_lists, _paired_oracle, _scan_equals_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31
N_PAIRS = 15_000
# Batch 0 creates too few records for the table to be grown before batch 1 (the library keeps it below a quarter full between batches),
# batch 1 creates far more than the table of the first pass and of the first two replays hold: three more batches behind it, so a replay
# walks batches after the one that overflowed it.  All cuts are at even reads: pairs stay whole.
CUTS = (0, 40, 20_000, 24_000, 28_000, 30_000)
CAPACITY = 1 << 10
TRIGGERS = {"capacity": (CAPACITY, {}), "lazy": (0, {"FGPU_DEBUG_LAZY_FAIL": "2"}), "both": (CAPACITY, {"FGPU_DEBUG_LAZY_FAIL": "2"})}
PATHS = ("stream", "prepared", "stream_then_prepared", "shard")
CONSUMERS = ("take_each", "take_at_end", "short_long_to_host", "long_not_to_host")


def cut(bases, offs, cuts):
    """ReadBatch objects of reads [cuts[i], cuts[i + 1])"""
    return [api.ReadBatch(bases, offs[a:b + 1].copy()) for a, b in zip(cuts[:-1], cuts[1:])]


@functools.lru_cache(maxsize=1)
def _data():
    """paired reads on a filter they overfill (several junction records per read), with everything the oracle says about them"""
    g = synth.make_genome(20 * N_PAIRS, 78)
    bases, offs = po.reads_from_matrix(np.ascontiguousarray(synth.make_pairs(g, N_PAIRS, 100, 260, 20, 0.01, 79)))
    n = len(offs) - 1
    assert n == CUTS[-1]
    E = 10 * n
    tai, nh = api.load_filter_shape(E, 2 * n)
    b2, short, long_, osc = _paired_oracle(bases, offs, K, tai, nh, E)
    _, want = _oracle_lists(bases, offs, K, 1, 100, b2.bits(), tai, nh)
    made = []                                    # records the map holds after each cut
    for c in CUTS[1:]:
        s = po.Scanner(K, 1, 100, b2)
        s.scan_reads(bases, offs[:c + 1].copy(), paired_ends=False, no_cleaning=True)
        made.append(s.stats()["n_junctions"])
    return dict(bases=bases, offs=offs, tai=tai, nh=nh, b2=b2, short=short, long=long_, osc=osc, ost=osc.stats(), want=want, made=made)


def test_the_data_overflows_where_intended():
    """the records of the overflowing batch exceed every table it is walked on before the third replay, and the batch before it does not
    make the table grow first (fgpu_scan_reserve: only past a quarter full)"""
    d = _data()
    assert d["made"][-1] == d["ost"]["n_junctions"]
    assert d["made"][0] * 4 <= CAPACITY                  # batch 0: no growth before batch 1, in the first pass nor in a replay
    assert d["made"][1] - d["made"][0] > 16 * CAPACITY   # batch 1: more than the first pass (2^10 slots) and two replays (2^12, 2^14) hold


def _lists_of(batch, st):
    lists = [[] for _ in range(batch.n_reads)]
    assert np.all(np.diff(st["read"].astype(np.int64)) >= 0)
    for e in st:
        lists[int(e["read"])].append(int(e["ext"]))
    return lists


class _Taker:
    """takes lists from a context and keeps them by batch number"""

    def __init__(self, ctx, batches):
        self.ctx, self.batches, self.seqs, self.lists = ctx, batches, [], []

    def take(self, until_none=False):
        while True:
            t = self.ctx.take_stops()
            if t is None:
                return
            seq, st = t
            self.seqs.append(seq)
            self.lists.extend(_lists_of(self.batches[seq], st))
            if not until_none:
                return


def _setup_consumer(ctx, consumer, d):
    if consumer in ("short_long_to_host", "long_not_to_host"):
        ctx.scan_short_pairs(d["short"].tai, d["short"].n_hash, consumer == "short_long_to_host")
        ctx.scan_long_pairs(d["long"].tai, d["long"].n_hash, 2)


def _scan(ctx, batches, path, consumer, capacity=0):
    """one scan of `batches` on ctx (scan_begin already called; capacity: its junction_capacity, where it matters); returns (taker, stats)"""
    tk = _Taker(ctx, batches)
    during = consumer != "take_at_end"
    if path == "prepared":
        for b in batches:
            ctx.scan_prepare(b)
            if during:
                tk.take()
        ctx.scan_walk_prepared()
        if during:
            for _ in batches:                # the walks of the last batches may still run: lists taken mid-scan
                tk.take()
    elif path == "stream_then_prepared":
        # The overflowing batch is walked by the streaming calls and nobody asks for lists before the next batch is PREPARED: the prepare finds
        # the oldest buffers still holding lists, fetches them, sees the overflow there and has to replay before it can go on (scan_prepare_from's
        # own replay: no other path reaches it).  The synchronisation lets the overflowing walk finish without anybody looking at its flags.
        for b in batches[:2]:
            ctx.scan_batch(b)
        ctx.synchronize()
        for i, b in enumerate(batches[2:]):
            ctx.scan_prepare(b)
            if i == 0 and capacity == CAPACITY and "FGPU_DEBUG_LAZY_FAIL" not in os.environ:
                assert ctx.diag_scan_replays() >= 1, "the first prepare did not replay"
            if during:
                tk.take()
        ctx.scan_walk_prepared()
        if during:
            for _ in batches:
                tk.take()
    else:
        for b in batches:
            ctx.scan_batch(b)
            if during:
                tk.take()
    sst = ctx.scan_end()
    tk.take(until_none=True)
    return tk, sst


def _run_cell(capacity, path, consumer):
    """one cell of the matrix, checked against the oracle"""
    import torch
    d = _data()
    bases, offs, tai, nh = d["bases"], d["offs"], d["tai"], d["nh"]
    batches = cut(bases, offs, CUTS)
    pairs = consumer in ("short_long_to_host", "long_not_to_host")
    to_host = consumer != "long_not_to_host"
    counts = (0, 0)
    if path == "shard":
        # shard A scans the first batch and hands its table and both pair filters to shard B, which scans the rest (on the small table)
        # (test_two_shard_scan_table_handover_is_exact; faucet_amd/sharded.py's pair_tensors)
        a = api.Context(K, tai, nh, record_stops=True)
        a.bloom_upload(L.BLOO2, d["b2"].bits())
        _setup_consumer(a, consumer, d)
        a.scan_begin()
        tk_a, st_a = _scan(a, batches[:1], "stream", consumer)
        n = a.table_entries()
        table = torch.empty(max(n, 1) * L.TABLE_ENTRY_BYTES, dtype=torch.uint8, device="cuda")
        assert a.export_table(table.data_ptr(), table.numel()) == n
        pair_state = []
        if pairs:
            for which in (0, 1):
                ptr, nbytes = a.scan_pairs_devptr(which)
                t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                _dev_copy(t, ptr, nbytes)
                pair_state.append(t)
            counts = a.scan_long_pairs_download(0)[1:]
        a.synchronize()
        torch.cuda.synchronize()
        ctx = api.Context(K, tai, nh, record_stops=True, junction_capacity=capacity)
        ctx.bloom_upload(L.BLOO2, d["b2"].bits())
        _setup_consumer(ctx, consumer, d)
        ctx.scan_begin()
        ctx.synchronize()                    # (scan_begin empties the filters on the context's stream)
        for which, t in enumerate(pair_state):
            ptr, nbytes = ctx.scan_pairs_devptr(which)
            assert nbytes == t.numel()
            _dev_copy_to(ptr, t, nbytes)
        torch.cuda.synchronize()
        ctx.import_table(table.data_ptr(), n, carried=st_a)
        tk, sst = _scan(ctx, batches[1:], "stream", consumer)
        first = CUTS[1]
        a_lists, a_seqs = tk_a.lists, tk_a.seqs
        a.close()
    else:
        ctx = api.Context(K, tai, nh, record_stops=True, junction_capacity=capacity)
        ctx.bloom_upload(L.BLOO2, d["b2"].bits())
        _setup_consumer(ctx, consumer, d)
        ctx.scan_begin()
        tk, sst = _scan(ctx, batches, path, consumer, capacity)
        first = 0
    cell = (capacity, path, consumer)
    n_b = len(batches) - (1 if path == "shard" else 0)
    if to_host:
        assert tk.seqs == list(range(n_b)), (cell, tk.seqs)            # every batch's lists exactly once, in order
        assert tk.lists == d["want"][first:], cell                     # ... and what scanInputRead returns for each read
        if path == "shard":
            assert a_seqs == [0] and a_lists == d["want"][:first], cell
    else:
        assert tk.seqs == [], cell
    if pairs:
        assert np.array_equal(ctx.scan_short_pairs_download(d["short"].tai), d["short"].bits()), cell
        bits, empty, not_empty = ctx.scan_long_pairs_download(d["long"].tai)
        assert np.array_equal(bits, d["long"].bits()), cell
        assert (empty + counts[0], not_empty + counts[1]) == (d["ost"]["empty_count"], d["ost"]["not_empty_count"]), cell
    _scan_equals_oracle(ctx, sst, d["osc"])
    assert ctx.diag_scan_replays() >= 1, cell
    ctx.close()


def _dev_copy(dst, src_ptr, nbytes):
    """device-to-device copy of nbytes from a raw device pointer into the tensor dst"""
    from faucet_amd.sharded import _DevView
    import torch
    dst.copy_(torch.as_tensor(_DevView(src_ptr, nbytes), device=dst.device))


def _dev_copy_to(dst_ptr, src, nbytes):
    from faucet_amd.sharded import _DevView
    import torch
    torch.as_tensor(_DevView(dst_ptr, nbytes), device=src.device).copy_(src)


def run_cells(trigger, paths, consumers):
    """every (path, consumer) cell of one trigger in this process; reports the cells that fail instead of stopping at the first"""
    capacity, _ = TRIGGERS[trigger]
    failed = []
    for path in paths:
        for consumer in consumers:
            try:
                _run_cell(capacity, path, consumer)
            except (AssertionError, api.FaucetGpuError) as e:
                failed.append(f"{path}/{consumer}: {type(e).__name__} {str(e)[:200]}")
    return failed


def test_lists_and_pair_filters_of_an_absorbed_overflow_equal_the_oracles():
    """The default run's representative: the table overflows (trigger capacity), streaming, prepared and prepared behind streamed batches, both pair filters on the device with
    lists also to the host and without; lists taken after every batch."""
    failed = run_cells("capacity", ("stream", "prepared", "stream_then_prepared"), ("short_long_to_host", "long_not_to_host"))
    assert not failed, "\n".join(failed)


def _child(code, env, timeout):
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), cwd=ROOT, timeout=timeout)
    return r


@pytest.mark.slow
@pytest.mark.parametrize("buffers", ["2", "3"])
@pytest.mark.parametrize("trigger", list(TRIGGERS))
def test_replay_consumer_matrix(trigger, buffers):
    """Every path (streaming, prepared, an importing shard) x every consumer (lists taken after every batch or at the end, both pair filters
    with and without lists to the host) for one trigger of the replay: the table overflows, the lazy check fails (FGPU_DEBUG_LAZY_FAIL=2),
    or both; with two and three batch buffers.  The knobs are read once per process: a child process per (trigger, buffers)."""
    _, env = TRIGGERS[trigger]
    env = dict(env, FGPU_SCAN_BUFFERS=buffers)
    code = ("from tests.test_gpu_replay_consumers import run_cells, PATHS, CONSUMERS\n"
            f"failed = run_cells({trigger!r}, PATHS, CONSUMERS)\n"
            "print('\\n'.join(failed))\n"
            "print('cells ok' if not failed else f'{len(failed)} cells failed')\n")
    r = _child(code, env, 600)
    assert r.returncode == 0 and "cells ok" in r.stdout, r.stdout + r.stderr[-4000:]


def test_without_a_journal_no_list_of_an_overflowed_walk_comes_out():
    """FGPU_JOURNAL_MB=0: nothing to replay, so the overflow is the caller's FGPU_ERR_CAPACITY -- and every list handed out before it is the
    oracle's.  Lists taken after every batch (the overflowing batch's among them, while its flag is already up)."""
    code = (
        "from faucet_amd import _lib as L, api\n"
        "from tests.test_gpu_replay_consumers import _data, _lists_of, cut, CUTS, CAPACITY, K\n"
        "d = _data()\n"
        "batches = cut(d['bases'], d['offs'], CUTS)\n"
        "ctx = api.Context(K, d['tai'], d['nh'], record_stops=True, junction_capacity=CAPACITY)\n"
        "ctx.bloom_upload(L.BLOO2, d['b2'].bits())\n"
        "ctx.scan_begin()\n"
        "got, err = [], None\n"
        "try:\n"
        "    for b in batches:\n"
        "        ctx.scan_batch(b)\n"
        "        t = ctx.take_stops()\n"
        "        if t is not None: got.append(t)\n"
        "    ctx.scan_end()\n"
        "except api.FaucetGpuError as e:\n"
        "    err = str(e)\n"
        "assert err is not None and 'junction table full' in err, err\n"
        "first = 0\n"
        "for i, (seq, st) in enumerate(got):\n"
        "    assert seq == i, [s for s, _ in got]\n"
        "    assert _lists_of(batches[seq], st) == d['want'][first:first + batches[seq].n_reads], seq\n"
        "    first += batches[seq].n_reads\n"
        "print('taken', len(got), 'then', err)\n"
        "print('journal off ok')\n")
    r = _child(code, {"FGPU_JOURNAL_MB": "0"}, 300)
    assert r.returncode == 0 and "journal off ok" in r.stdout, r.stdout + r.stderr[-4000:]
