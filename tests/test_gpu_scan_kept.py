"""Pass 2 over the batches pass 1 kept (FGPU_LOAD_KEEP_READS, fgpu_scan_kept_state, fgpu_scan_batch_kept): a load pass that also keeps every
batch's read offsets, and a scan that takes the kept batches instead of their text -- no packing, no comparison, the sure planes reused.  What
such a scan produces (junction records in creation order, the reference's counters, scanInputRead's lists, both pair filters, the pair counts)
is compared with the goldens written by the compiled reference and with the oracle, never only with the text scan of this build.
Needs an MI355X."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from oracle import pyoracle as po
from tests.golden_util import Case
from tests.test_gpu_parity import _oracle_lists, _scan_equals_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = ["ragged_k31", "c1_k21", "j2_spacer20_k15", "mercy_k21", "se_cleaning_k21", "pe_fastq_k21", "pe_repeats_k25"]
BATCHINGS = ["one_batch", "single_reads", "odd_333", "empty_in_the_middle", "T_mod_64_is_0", "T_mod_64_is_1", "T_mod_64_is_63"]
STATE, ARG = f"error {L.ERR_STATE}:", f"error {L.ERR_ARG}:"


@functools.lru_cache(maxsize=None)
def ref(name):
    """a golden's reads with what the oracle makes of them: computed once per process, shared by every test, never written to.  The oracle
    scans with cleaning on (paired where the golden is): both pair filters, sized as src/Faucet.cpp:266-283 sizes them, and the pair counts"""
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    lst = po.load_two_filters(b1, b2, bases, offs, c.k, mercy=c.mercy)
    assert np.array_equal(b2.bits(), c.bloom())              # the oracle's bloo2 is the compiled reference's .bloom
    se, le = c.pair_filter_elements()
    _, stai, snh = api.size_optimal(se, np.float32(0.01))
    _, ltai, lnh = api.size_optimal(le, np.float32(0.01))
    short, long_ = po.Bloom(stai, snh), (po.Bloom(ltai, lnh) if c.paired else None)
    osc = po.Scanner(c.k, c.j, c.spacer, b2, short_pf=short, long_pf=long_)
    osc.scan_reads(bases, offs, paired_ends=c.paired, no_cleaning=False)
    _, want = _oracle_lists(bases, offs, c.k, c.j, c.spacer, b2.bits(), tai, nh)
    if not c.no_cleaning:                                    # ... and its pair filters are the compiled reference's files
        assert np.array_equal(short.bits(), c.pair_filter("short"))
        assert not c.paired or np.array_equal(long_.bits(), c.pair_filter("long"))
    for a in (bases, offs):
        a.setflags(write=False)
    return types.SimpleNamespace(c=c, bases=bases, offs=offs, tai=tai, nh=nh, b1=b1, b2=b2, lst=lst, short=short, long=long_, osc=osc,
                                 ost=osc.stats(), want=want)


def cuts_of(offs, batching):
    """read indices at which the batching cuts the golden's reads (a repeated index: an empty batch)"""
    n = len(offs) - 1
    if batching == "one_batch":
        return [0, n]
    if batching == "single_reads":
        return list(range(n + 1))
    if batching == "odd_333":                    # an odd number of reads per batch: a pair straddles two batches
        return list(range(0, n, 333)) + [n]
    if batching == "empty_in_the_middle":
        return [0, n // 3, n // 3, n]
    r = int(batching.rsplit("_", 1)[1])          # the first batch's stream length T = bases + reads is r modulo 64: the last plane word full, one bit, 63 bits
    T = (offs[1:n] - offs[0]).astype(np.int64) + np.arange(1, n)
    fits = np.flatnonzero(T % 64 == r) + 1
    assert len(fits), "no read boundary gives this stream length"
    return [0, int(fits[np.argmin(np.abs(fits - n // 2))]), n]


def batches_of(r, cuts):
    return [api.ReadBatch(r.bases, r.offs[a:b + 1].copy()) for a, b in zip(cuts[:-1], cuts[1:])]


def context_for(r, **kw):
    c = r.c
    return api.Context(c.k, r.tai, r.nh, j=c.j, max_spacer_dist=c.spacer, mercy=c.mercy, record_stops=True, **kw)


def load_keeping(ctx, batches, keep_reads=True, **kw):
    ctx.load_begin(keep_reads=keep_reads, **kw)
    for b in batches:
        ctx.load_batch(b)
    return ctx.load_end()


def assert_load_is_the_references(ctx, r, st):
    c = r.c
    assert np.array_equal(ctx.bloom_download(L.BLOO2), c.bloom()), "bloo2 differs from the reference's .bloom file"
    assert np.array_equal(ctx.bloom_download(L.BLOO1), r.b1.bits())
    assert st == {"reads_processed": c.counters["load_reads_processed"], "unambiguous_reads": c.counters["load_unambiguous"], "kmers": r.lst.kmers,
                  "to_bloo2": r.lst.to_bloo2}


def set_pair_filters(ctx, r):
    ctx.scan_short_pairs(r.short.tai, r.short.n_hash, True)            # (the lists come to the host as well)
    if r.c.paired:
        ctx.scan_long_pairs(r.long.tai, r.long.n_hash, 2)


def scan_kept(ctx, sizes, text_batch_at=None, text_batch=None):
    """one scan over the kept batches 0 .. len(sizes) - 1 (scan_begin to scan_end); returns (stats, lists per read in file order)"""
    ctx.scan_begin()
    for i, n in enumerate(sizes):
        if i == text_batch_at:
            ctx.scan_batch(text_batch)
        else:
            assert ctx.scan_batch_kept(i) == n
    sst = ctx.scan_end()
    lists, seqs = [], []
    while True:
        t = ctx.take_stops()
        if t is None:
            break
        seq, st = t
        seqs.append(seq)
        per_read = [[] for _ in range(sizes[seq])]
        assert np.all(np.diff(st["read"].astype(np.int64)) >= 0)
        for e in st:
            per_read[int(e["read"])].append(int(e["ext"]))
        lists.extend(per_read)
    assert seqs == list(range(len(sizes)))
    return sst, lists


def assert_scan_is_the_references(ctx, r, sst, lists):
    c, cn = r.c, r.c.counters
    for key, golden_key in (("n_junctions", "distinct_junctions"), ("nb_jcheck_kmer", "nb_jcheck_kmer"), ("nb_no_juncs", "nb_no_juncs"),
                            ("nb_processed", "nb_processed"), ("nb_skipped", "nb_skipped"), ("reads_no_errors", "reads_no_errors"),
                            ("reads_processed", "scan_reads_processed"), ("unambiguous_reads", "scan_unambiguous")):
        assert sst[key] == cn[golden_key], key
    _scan_equals_oracle(ctx, sst, r.osc)                     # the oracle's counters, keys in creation order, records
    keys, recs = ctx.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines())
    assert lists == r.want                                   # scanInputRead's return value, read by read
    assert np.array_equal(ctx.scan_short_pairs_download(r.short.tai), r.short.bits())
    if c.paired:
        bits, empty, not_empty = ctx.scan_long_pairs_download(r.long.tai)
        assert np.array_equal(bits, r.long.bits())
        assert (empty, not_empty) == (r.ost["empty_count"], r.ost["not_empty_count"]) == (cn["empty_count"], cn["not_empty_count"])


def run_case(name, batching, expect_replays=False, scans=1, **ctx_kw):
    """load with keep_reads, the state, then `scans` scans of the kept batches, each checked against the golden and the oracle"""
    r = ref(name)
    batches = batches_of(r, cuts_of(r.offs, batching))
    sizes = [b.n_reads for b in batches if b.n_reads]
    ctx = context_for(r, **ctx_kw)
    assert ctx.scan_kept_state()["complete"] is False        # before any load pass
    st = load_keeping(ctx, batches)
    assert_load_is_the_references(ctx, r, st)
    state = ctx.scan_kept_state()
    assert (state["complete"], state["n_batches"], state["n_reads"]) == (True, len(sizes), len(r.offs) - 1)
    T = [int(b.offsets[-1] - b.offsets[0]) + b.n_reads for b in batches if b.n_reads]
    assert state["bytes"] >= sum(4 * ((t + 63) // 64 + 8) * 8 + (n + 1) * 8 for t, n in zip(T, sizes))      # the offsets are charged to the budget
    set_pair_filters(ctx, r)
    for _ in range(scans):
        before = ctx.diag_scan_replays()
        sst, lists = scan_kept(ctx, sizes)
        assert_scan_is_the_references(ctx, r, sst, lists)
        if expect_replays:
            assert ctx.diag_scan_replays() >= before + 1
        else:
            assert ctx.diag_scan_replays() == before
            # every occurrence the load routed to bloo2 is answered from the kept plane (--mercy adds k-mers to bloo2 outside that count)
            assert sst["valid_reused"] > 0 and (r.c.mercy or sst["valid_reused"] == r.lst.to_bloo2)
    ctx.close()


@pytest.mark.parametrize("batching", BATCHINGS)
@pytest.mark.parametrize("name", GOLDENS)
def test_scan_of_kept_batches_equals_the_reference(name, batching):
    run_case(name, batching)


# ---- 1. adopted blocks: pass 0 keeps blocks and their reads, another context loads and scans them ----------------------------------------------
@pytest.mark.parametrize("batching", ["one_batch", "empty_in_the_middle", "odd_333"])
@pytest.mark.parametrize("name", ["ragged_k31", "pe_fastq_k21"])
def test_scan_of_adopted_blocks_equals_the_reference(name, batching):
    r = ref(name)
    batches = batches_of(r, cuts_of(r.offs, batching))
    sizes = [b.n_reads for b in batches if b.n_reads]
    p0 = api.Context(r.c.k, 128, 1)
    p0.estimate_begin(14)
    with pytest.raises(api.FaucetGpuError, match=STATE):
        p0.estimate_keep_reads()                             # before estimate_keep
    p0.estimate_keep(1 << 62)
    p0.estimate_keep_reads()
    for b in batches:
        p0.estimate_batch(b)
    p0.estimate_end()
    with pytest.raises(api.FaucetGpuError, match=STATE):
        p0.estimate_take_kept_reads()                        # the blocks first
    blocks = p0.estimate_take_kept()
    reads = p0.estimate_take_kept_reads()
    p0.close()                                               # blocks and offsets outlive the context that made them
    assert [pk.n_reads for pk in blocks] == sizes == [kr.n_reads for kr in reads]
    longest = int(np.diff(r.offs).max())
    assert all(kr.max_read_len == longest for kr in reads)
    ctx = context_for(r)
    ctx.load_begin()
    with pytest.raises(api.FaucetGpuError, match=STATE):
        ctx.load_batch_packed_reads(blocks[0], reads[0])     # a pass without keep_reads: nothing adopted
    ctx.load_end()
    ctx.load_begin(keep_reads=True)
    with pytest.raises(api.FaucetGpuError, match=ARG):
        ctx.load_batch_packed_reads(blocks[0], L.KeptReads(reads[0].offsets_dev, reads[0].n_reads + 1, 0))
    for pk, kr in zip(blocks, reads):
        ctx.load_batch_packed_reads(pk, kr)
    st = ctx.load_end()
    assert_load_is_the_references(ctx, r, st)
    state = ctx.scan_kept_state()
    assert (state["complete"], state["n_batches"], state["n_reads"]) == (True, len(sizes), len(r.offs) - 1)
    set_pair_filters(ctx, r)
    sst, lists = scan_kept(ctx, sizes)
    assert_scan_is_the_references(ctx, r, sst, lists)
    assert sst["valid_reused"] == r.lst.to_bloo2 > 0
    ctx.close()


def test_a_block_adopted_without_its_reads_leaves_the_state_incomplete():
    r = ref("c1_k21")
    batches = batches_of(r, cuts_of(r.offs, "one_batch"))
    p0 = api.Context(r.c.k, 128, 1)
    p0.estimate_begin(14)
    p0.estimate_keep(1 << 62)
    p0.estimate_batch(batches[0])
    p0.estimate_end()
    (pk,) = p0.estimate_take_kept()
    ctx = context_for(r)
    ctx.load_begin(keep_reads=True)
    ctx.load_batch_packed(pk)
    ctx.load_end()
    assert ctx.scan_kept_state()["complete"] is False
    ctx.scan_begin()
    with pytest.raises(api.FaucetGpuError, match=STATE):
        ctx.scan_batch_kept(0)
    ctx.scan_end()
    ctx.close()
    p0.close()


# ---- 2. a forced lazy failure is absorbed through the replay (the knob is read once per process: a child) ------------------------------------
def test_forced_lazy_failure_of_a_kept_scan_is_absorbed():
    code = ("from tests.test_gpu_scan_kept import run_case\n"
            "for name in ('ragged_k31', 'pe_fastq_k21'):\n"
            "    run_case(name, 'odd_333', expect_replays=True, scans=2)\n"
            "print('kept replay ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, FGPU_DEBUG_LAZY_FAIL="1"), cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "kept replay ok" in r.stdout, r.stdout + r.stderr[-4000:]


# ---- 3. a junction table that overflows: five batches, lists, both pair filters --------------------------------------------------------------
def test_table_overflow_of_a_kept_scan_is_absorbed():
    from tests.test_gpu_replay_consumers import CAPACITY, CUTS, K, _data, _lists_of, cut
    d = _data()
    batches = cut(d["bases"], d["offs"], CUTS)
    ctx = api.Context(K, d["tai"], d["nh"], record_stops=True, junction_capacity=CAPACITY)
    ctx.load_begin(keep_reads=True)
    for b in batches:
        ctx.load_batch(b)
    ctx.load_end()
    assert np.array_equal(ctx.bloom_download(L.BLOO2), d["b2"].bits())
    assert ctx.scan_kept_state()["complete"] and ctx.scan_kept_state()["n_batches"] == len(batches) >= 3
    ctx.scan_short_pairs(d["short"].tai, d["short"].n_hash, True)
    ctx.scan_long_pairs(d["long"].tai, d["long"].n_hash, 2)
    ctx.scan_begin()
    got, seqs = [], []

    def take(until_none):
        while True:
            t = ctx.take_stops()
            if t is None:
                return
            seqs.append(t[0])
            got.extend(_lists_of(batches[t[0]], t[1]))
            if not until_none:
                return
    for i, b in enumerate(batches):
        assert ctx.scan_batch_kept(i) == b.n_reads
        take(False)                                          # lists taken while the scan runs: none of an overflowed walk may come out
    sst = ctx.scan_end()
    take(True)
    assert ctx.diag_scan_replays() >= 1
    assert seqs == list(range(len(batches))) and got == d["want"]
    assert np.array_equal(ctx.scan_short_pairs_download(d["short"].tai), d["short"].bits())
    bits, empty, not_empty = ctx.scan_long_pairs_download(d["long"].tai)
    assert np.array_equal(bits, d["long"].bits())
    assert (empty, not_empty) == (d["ost"]["empty_count"], d["ost"]["not_empty_count"])
    _scan_equals_oracle(ctx, sst, d["osc"])
    ctx.close()


# ---- 4. the batches live until the next load pass: a second scan, batches in another order's worth of state ------------------------------------
@pytest.mark.parametrize("name", ["ragged_k31", "pe_repeats_k25"])
def test_a_second_scan_of_the_same_kept_batches_gives_the_same(name):
    run_case(name, "odd_333", scans=2)


# ---- 5. keep_reads leaves pass 1 alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_carry", [False, True])
@pytest.mark.parametrize("name", ["ragged_k31", "mercy_k21", "pe_fastq_k21"])
def test_keep_reads_changes_nothing_of_the_load_pass(name, keep_carry):
    r = ref(name)
    batches = batches_of(r, cuts_of(r.offs, "odd_333"))
    out = []
    for keep_reads in (False, True):
        ctx = context_for(r)
        st = load_keeping(ctx, batches, keep_reads=keep_reads, keep_carry=keep_carry)      # (bloo1 of a fresh context is empty: the same pass)
        out.append((st, ctx.bloom_download(L.BLOO1), ctx.bloom_download(L.BLOO2), ctx.diag_load_split()))
        assert ctx.scan_kept_state()["complete"] is keep_reads
        assert_load_is_the_references(ctx, r, st)
        ctx.close()
    assert out[0][0] == out[1][0] and out[0][3] == out[1][3]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_a_text_batch_in_a_kept_scan():
    r = ref("se_cleaning_k21")
    batches = batches_of(r, cuts_of(r.offs, "odd_333"))
    sizes = [b.n_reads for b in batches]
    ctx = context_for(r)
    with pytest.raises(api.FaucetGpuError, match=STATE):
        ctx.scan_batch_kept(0)                               # outside a scan
    load_keeping(ctx, batches, keep_reads=False)             # a load without the flag
    assert ctx.scan_kept_state() == {"complete": False, "n_batches": len(batches), "n_reads": 0, "bytes": ctx.scan_kept_state()["bytes"]}
    ctx.scan_begin()
    with pytest.raises(api.FaucetGpuError, match=STATE):
        ctx.scan_batch_kept(0)
    ctx.scan_end()
    for flags in ({"shard_times": True}, {"shard_planes": True}, {"shard_times": True, "keep_carry": True}):
        with pytest.raises(api.FaucetGpuError, match=STATE):
            ctx.load_begin(keep_reads=True, **flags)         # read shards keep batches of their own
    load_keeping(ctx, batches)
    assert ctx.scan_kept_state()["complete"]
    set_pair_filters(ctx, r)
    ctx.scan_begin()
    with pytest.raises(api.FaucetGpuError, match=ARG):
        ctx.scan_batch_kept(len(batches))                    # i == n_batches
    ctx.scan_end()
    while ctx.take_stops() is not None:
        pass
    # a text batch mixed into a kept scan: the same scan
    sst, lists = scan_kept(ctx, sizes, text_batch_at=1, text_batch=batches[1])
    assert_scan_is_the_references(ctx, r, sst, lists)
    # the next load pass forgets the batches; so does a filter from outside
    ctx.load_begin()
    assert ctx.scan_kept_state()["complete"] is False
    ctx.load_end()
    load_keeping(ctx, batches)
    ctx.bloom_upload(L.BLOO2, r.c.bloom())
    assert ctx.scan_kept_state()["complete"] is False
    ctx.close()
    # without resident batches nothing is kept
    ctx = context_for(r, keep_resident=False)
    load_keeping(ctx, batches)
    assert ctx.scan_kept_state()["complete"] is False and ctx.scan_kept_state()["n_batches"] == 0
    ctx.scan_begin()
    with pytest.raises(api.FaucetGpuError, match=STATE):
        ctx.scan_batch_kept(0)
    ctx.scan_end()
    ctx.close()
