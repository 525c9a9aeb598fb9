"""Parity of the HIP path (through the C ABI) against the oracle and the golden fixtures.  Needs an MI355X."""
import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api, synth
from oracle import pyoracle as po
from tests import getline_ref
from tests.golden_util import CASES, Case, kat

pytestmark = pytest.mark.gpu


def oracle_run(lines_or_batch, k, tai, nh, j=1, spacer=100, mercy=False):
    bases, offs = lines_or_batch
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    lst = po.load_two_filters(b1, b2, bases, offs, k, mercy=mercy)
    sc = po.Scanner(k, j, spacer, b2)
    sc.scan_reads(bases, offs, paired_ends=False, no_cleaning=True)
    return b1, b2, lst, sc


def chunks(bases, offs, n_chunks):
    """split a host batch into n_chunks ReadBatch objects at read boundaries"""
    n = len(offs) - 1
    cuts = np.linspace(0, n, n_chunks + 1).astype(int)
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out.append(api.ReadBatch(bases, offs[a:b + 1].copy()))
    return out


def test_library_is_the_hip_one():
    assert L.load().fgpu_device_count() >= 1


@pytest.mark.parametrize("d", kat("hash"), ids=lambda d: f"k{d['k']}")
def test_hash_kat_on_device(d):
    k, tai = d["k"], d["tai"]
    ctx = api.Context(k, tai, 3)
    kmers = np.array([int(e["fwd"], 16) for e in d["pos"]], dtype=np.uint64)
    c, a, b = ctx.probe_hash(kmers)
    assert list(c) == [min(int(e["fwd"], 16), int(e["rc"], 16)) for e in d["pos"]]
    assert list(a) == [e["hA"] for e in d["pos"]]
    assert list(b) == [e["hB"] for e in d["pos"]]
    # the reverse complement hashes to the same canonical values
    c2, a2, b2 = ctx.probe_hash(np.array([int(e["rc"], 16) for e in d["pos"]], dtype=np.uint64))
    assert np.array_equal(c, c2) and np.array_equal(a, a2) and np.array_equal(b, b2)


def test_hash_random_vs_oracle():
    rng = np.random.default_rng(3)
    for k, tai in ((31, 1 << 29), (21, 1 << 19), (5, 1 << 10), (15, 1 << 33)):
        kmers = rng.integers(0, 1 << (2 * k), size=5000, dtype=np.uint64)
        ctx = api.Context(k, tai, 3)
        c, a, b = ctx.probe_hash(kmers)
        lib = po.lib()
        for i in range(0, 5000, 7):
            cc = lib.fo_canon(int(kmers[i]), k)
            assert int(c[i]) == cc
            assert int(a[i]) == lib.fo_old_hash(cc, 0, tai) and int(b[i]) == lib.fo_old_hash(cc, 1, tai)
        ctx.close()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("n_batches", [1, 3])
def test_load_matches_reference_bloom(name, n_batches):
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer, mercy=c.mercy)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, n_batches))
    got2 = ctx.bloom_download(L.BLOO2)
    assert np.array_equal(got2, c.bloom()), "bloo2 differs from the reference's .bloom file"
    b1, b2, lst, _ = oracle_run((bases, offs), c.k, tai, nh, c.j, c.spacer, mercy=c.mercy)
    assert np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits())
    assert st["reads_processed"] == c.counters["load_reads_processed"]
    assert st["unambiguous_reads"] == c.counters["load_unambiguous"]
    assert st["kmers"] == lst.kmers and st["to_bloo2"] == lst.to_bloo2
    w = c.counters["weights_after_load"]
    assert f"{ctx.bloom_weight(L.BLOO1):f}" == w[0] and f"{ctx.bloom_weight(L.BLOO2):f}" == w[1]


def _scan_and_compare(c, bases, offs, n_batches, span, eager=False):
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer, walk_window_span=span, eager_flags=eager)
    ctx.bloom_upload(L.BLOO2, c.bloom())
    sc = api.ReadScanner(ctx)
    st = sc.scanReads(chunks(bases, offs, n_batches))
    cn = c.counters
    assert st["n_junctions"] == cn["distinct_junctions"]
    assert st["nb_jcheck_kmer"] == cn["nb_jcheck_kmer"]
    assert st["nb_no_juncs"] == cn["nb_no_juncs"]
    assert st["nb_processed"] == cn["nb_processed"]
    assert st["nb_skipped"] == cn["nb_skipped"]
    assert st["reads_no_errors"] == cn["reads_no_errors"]
    assert st["reads_processed"] == cn["scan_reads_processed"]
    assert st["unambiguous_reads"] == cn["scan_unambiguous"]
    keys, recs = sc.junctions()
    got = api.junction_lines(keys, recs, c.k)
    assert sorted(got) == sorted(c.junction_lines())
    # creation order == the oracle's insertion order, so the same container gives the reference's dump order
    b2 = po.Bloom(tai, nh)
    b2.set_bits(c.bloom())
    osc = po.Scanner(c.k, c.j, c.spacer, b2)
    osc.scan_reads(bases, offs, paired_ends=False, no_cleaning=True)
    okeys, orecs = osc.junctions("creation")
    assert np.array_equal(keys, okeys)
    assert got == po.junction_lines(okeys, orecs, c.k)
    return st


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("n_batches,span", [(1, 0), (4, 0), (1, 256), (2, 4096), (1, 1 << 20)])
def test_scan_matches_reference_junctions(name, n_batches, span):
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    _scan_and_compare(c, bases, offs, n_batches, span)


@pytest.mark.parametrize("name", ["c1_k21", "ragged_k31", "j2_spacer20_k15", "twohash_k31_L150"])
def test_key_ordered_walk_of_clusters_gives_the_same_result(name, monkeypatch):
    """FGPU_WALK_KO=2 with FGPU_WALK_KO_ALWAYS: every cluster of two or more pieces is walked by k_walk_ko -- one piece per wave, accesses ordered
    per junction k-mer by turn counters instead of pieces per cluster.  By default it takes clusters of 64 pieces and more,
    from the moment a scan has shown one; the results must not depend on who walks what.  (The whole GPU suite passes with these two settings;
    here: four goldens, tandem repeats -- the same k-mer several times on a piece -- and 40x random reads with a fake junction per read end.)"""
    monkeypatch.setenv("FGPU_WALK_KO", "2")
    monkeypatch.setenv("FGPU_WALK_KO_ALWAYS", "1")
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    for n_batches, span in ((1, 0), (3, 4096), (1, 256)):
        _scan_and_compare(c, bases, offs, n_batches, span)
    bases, offs = _random_case(20000, 110, 25, 50000, 0.012, 7, 0.002, 4)
    sst = _check_against_oracle(bases, offs, 25, 1_000_000, 200_000, 1, walk_window_span=1 << 14)
    assert sst["walk_parallel"] > 2000
    rng = np.random.default_rng(53)
    unit = synth._ACGT[rng.integers(0, 4, size=53)]
    genome = np.tile(unit, 20000 // 53 + 2)[:20000].copy()
    r = synth.make_reads(genome, 3000, 120, 0.004, 54)
    bases, offs = po.reads_from_matrix(r)
    assert _check_against_oracle(bases, offs, 21, 500_000, 100_000, 1, scan_chunks=3)["walk_parallel"] > 1000
    # reads of 300 bases: pieces of up to 270 windows (the turn bookkeeping holds 512), and of 2000 bases (their clusters stay with k_walk)
    long_bases, long_offs = _random_case(4000, 300, 27, 30000, 0.01, 11, 0.001, 3)
    assert _check_against_oracle(long_bases, long_offs, 27, 1_000_000, 200_000, 1)["walk_parallel"] > 1000
    long_bases, long_offs = _random_case(300, 2000, 31, 20000, 0.004, 12, 0.0, 2)
    _check_against_oracle(long_bases, long_offs, 31, 500_000, 100_000, 1)
    # and as a caller asks for it (what the CLI does): the flag instead of the environment, clusters of 32 pieces and more
    monkeypatch.delenv("FGPU_WALK_KO")
    monkeypatch.delenv("FGPU_WALK_KO_ALWAYS")
    assert _check_against_oracle(bases, offs, 21, 500_000, 100_000, 1, scan_chunks=3, key_order_from_start=True)["walk_parallel"] > 100


@pytest.mark.parametrize("rounds", ["0", "2", "12"])
def test_large_clusters_walked_optimistically_settle_or_are_handed_over(rounds, monkeypatch):
    """The optimistic walk of large clusters (k_ovw_round): every piece of such a cluster walks read-only on the events --
    creations, raised distances, with file-order times -- the earlier pieces posted in the round before, until no piece's log changes; the
    settled logs are applied with atomics.  Twenty copies of a 300-base repeat at 40x: junction map and counters equal the oracle's record for
    record with the default 12 rounds per window (everything settles), with 2 (the first windows, where the repeat's junctions are being
    created, cannot settle: they are handed to the key-ordered walk, k_walk_ko, which runs behind) and with 0 (key-ordered walk only)."""
    monkeypatch.setenv("FGPU_WALK_KO", "16")
    monkeypatch.setenv("FGPU_WALK_KO_ALWAYS", "1")
    monkeypatch.setenv("FGPU_OVW_ROUNDS", rounds)
    g = synth.make_genome(150_000, 91, repeats=20, repeat_len=300)
    r = synth.make_reads(g, 60_000, 100, 0.01, 92)
    bases, offs = po.reads_from_matrix(r)
    k, E, S = 31, 2_000_000, 500_000
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    okeys, orecs = osc.junctions("creation")
    for span, record in ((1 << 20, False), (0, True), (1 << 16, False)):
        ctx = api.Context(k, tai, nh, walk_window_span=span, record_stops=record)
        ctx.bloom_upload(L.BLOO2, b2.bits())
        sc = api.ReadScanner(ctx)
        sst = sc.scanReads(chunks(bases, offs, 3))
        _scan_equals_oracle(sc, sst, osc)
        d = ctx.diag_ovw()
        assert sst["walk_parallel"] > 1000
        if rounds == "0":
            assert d["pieces"] == 0 and d["windows"] == 0
        elif rounds == "2":
            assert d["fallback_windows"] > 0, d
        else:
            assert d["pieces"] > 1000 and d["fallback_windows"] == 0 and d["rounds"] >= 2 * d["windows"], d
        if record:     # scanInputRead's lists: the visits of the settled logs (or of the walk they were handed to)
            _, want = _oracle_lists(bases, offs, k, 1, 100, b2.bits(), tai, nh)
            got = []
            while True:
                t = ctx.take_stops()
                if t is None:
                    break
                lists = [[] for _ in range(int(t[1]["read"].max()) + 1 if len(t[1]) else 0)]
                for e in t[1]:
                    lists[int(e["read"])].append(int(e["ext"]))
                got.append(lists)
            parts = chunks(bases, offs, 3)
            flat = []
            for part, lists in zip(parts, got):
                flat.extend(lists + [[] for _ in range(part.n_reads - len(lists))])
            assert flat == want
        ctx.close()


def test_event_tables_of_the_optimistic_walk_grow_before_they_overflow(monkeypatch):
    """The event tables are sized by what the scan shows (fgpu_diag_ovw_tables): started at 2^10 entries on the twenty-copy repeat set, the first
    windows overflow them -- exact: they are handed to the key-ordered walk -- and report how many entries a round held; the next windows get
    tables eight times that.  Same map and counters as the oracle either way; with the default 2^23 entries nothing grows."""
    monkeypatch.setenv("FGPU_WALK_KO", "16")
    monkeypatch.setenv("FGPU_WALK_KO_ALWAYS", "1")
    g = synth.make_genome(150_000, 91, repeats=20, repeat_len=300)
    r = synth.make_reads(g, 60_000, 100, 0.01, 92)
    bases, offs = po.reads_from_matrix(r)
    k, E, S = 31, 2_000_000, 500_000
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    for start in ("10", None):
        if start:
            monkeypatch.setenv("FGPU_OVW_EV_LOG2", start)
        else:
            monkeypatch.delenv("FGPU_OVW_EV_LOG2")
        ctx = api.Context(k, tai, nh, walk_window_span=1 << 16)
        ctx.bloom_upload(L.BLOO2, b2.bits())
        sc = api.ReadScanner(ctx)
        sst = sc.scanReads(chunks(bases, offs, 6))
        _scan_equals_oracle(sc, sst, osc)
        t, d = ctx.diag_ovw_tables(), ctx.diag_ovw()
        assert t["high_water"] > 0 and d["pieces"] > 1000, (t, d)
        if start:
            assert t["capacity"] > 1 << 10 and t["capacity"] >= 4 * t["high_water"], (t, d)
        else:
            assert t["capacity"] == 1 << 23 and d["fallback_windows"] == 0, (t, d)


@pytest.mark.parametrize("name", CASES)
def test_scan_eager_flags_mode_gives_the_same_result(name):
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    _scan_and_compare(c, bases, offs, 5, 0, eager=True)


@pytest.mark.parametrize("name", ["ragged_k31", "twohash_k31_L150"])
def test_scan_prepare_then_walk_equals_scan_batch(name):
    c = Case(name)
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer)
    ctx.bloom_upload(L.BLOO2, c.bloom())
    ctx.scan_begin()
    for part in chunks(bases, offs, 3):
        ctx.scan_prepare(part)
    ctx.scan_walk_prepared()
    st = ctx.scan_end()
    cn = c.counters
    assert st["n_junctions"] == cn["distinct_junctions"] and st["nb_processed"] == cn["nb_processed"]
    assert st["nb_skipped"] == cn["nb_skipped"] and st["nb_jcheck_kmer"] == cn["nb_jcheck_kmer"]
    assert st["reads_processed"] == cn["scan_reads_processed"]
    keys, recs = ctx.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines())


def test_streaming_scan_after_a_prepared_shard_does_not_outrun_its_walk(monkeypatch):
    """A context that has walked a prepared shard keeps that shard's buffers (one set per batch).  A streaming scan afterwards must still
    reuse the buffers of two batches ago and wait for that walk: taken first in, first out, the deep pool let the pure stage run ahead of the
    walk by more batches than the created-key lists cover -- snapshot planes without keys that exist, a wrong map (round 5: config 4's first
    50 M reads streamed after a 60 M-read prepared shard came out with 9 887 records too many).  The walk stream is held up 3 ms per batch
    here (FGPU_DEBUG_WALK_STALL_US) so that the pure stage of these small batches WOULD run ahead as far as the host lets it."""
    bases, offs = _random_case(30000, 100, 31, 40000, 0.01, 77, 0.0, 3)
    k, E, S = 31, 2_000_000, 400_000
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    ctx = api.Context(k, tai, nh)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    ctx.scan_begin()
    for part in chunks(bases, offs, 24):
        ctx.scan_prepare(part)
    ctx.scan_walk_prepared()
    st = ctx.scan_end()
    assert st["n_junctions"] == osc.stats()["n_junctions"]
    monkeypatch.setenv("FGPU_DEBUG_WALK_STALL_US", "3000")
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, 24))
    _scan_equals_oracle(sc, sst, osc)
    # ... and inside ONE scan: the first half prepared and walked, the second half streamed behind it
    parts = chunks(bases, offs, 24)
    ctx.scan_begin()
    for part in parts[:12]:
        ctx.scan_prepare(part)
    ctx.scan_walk_prepared()
    for part in parts[12:]:
        ctx.scan_batch(part)
    sst = ctx.scan_end()
    _scan_equals_oracle(ctx, sst, osc)


def test_load_then_scan_end_to_end_on_device():
    """bloo2 stays resident between the passes (no upload), as in the CLI."""
    c = Case("c1_k21")
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    ctx = api.Context(c.k, tai, nh)
    api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), [api.ReadBatch(bases, offs)])
    sc = api.ReadScanner(ctx)
    st = sc.scanReads([api.ReadBatch(bases, offs)])
    keys, recs = sc.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines())
    assert st["n_junctions"] == c.counters["distinct_junctions"]


def _random_case(n_reads, L_, k, G, err, seed, n_rate=0.0, repeats=0):
    g = synth.make_genome(G, seed, repeats=repeats, repeat_len=3 * k if repeats else 0)
    r = synth.make_reads(g, n_reads, L_, err, seed + 1, n_rate=n_rate)
    return po.reads_from_matrix(r)


@pytest.mark.parametrize("n_reads,L_,k,G,err,E,S,j,n_rate,repeats", [
    (20000, 100, 31, 40000, 0.01, 2_000_000, 400_000, 1, 0.0, 0),
    (20000, 100, 31, 40000, 0.01, 2_000_000, 400_000, 1, 0.003, 5),
    (6000, 150, 27, 20000, 0.03, 1_000_000, 500_000, 1, 0.0, 3),      # 2 hash functions, spacer rule reachable
    (8000, 80, 15, 3000, 0.005, 300_000, 60_000, 0, 0.0, 2),          # tiny genome: heavy clustering
    (5000, 250, 31, 30000, 0.01, 1_000_000, 200_000, 2, 0.001, 2),    # long reads, j = 2
])
def test_random_inputs_vs_oracle(n_reads, L_, k, G, err, E, S, j, n_rate, repeats):
    bases, offs = _random_case(n_reads, L_, k, G, err, 1234 + n_reads, n_rate, repeats)
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, j, 100)
    ctx = api.Context(k, tai, nh, j=j)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, 3))
    assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits())
    assert np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits())
    assert st["kmers"] == lst.kmers and st["to_bloo2"] == lst.to_bloo2 and st["unambiguous_reads"] == lst.unambiguous_reads
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, 2))
    ost = osc.stats()
    for key in ("n_junctions", "nb_jcheck_kmer", "nb_no_juncs", "nb_processed", "nb_skipped", "reads_no_errors",
                "unambiguous_reads", "reads_processed"):
        assert sst[key] == ost[key], key
    keys, recs = sc.junctions()
    okeys, orecs = osc.junctions("creation")
    assert np.array_equal(keys, okeys)
    assert np.array_equal(recs["dist"], orecs["dist"]) and np.array_equal(recs["cov"], orecs["cov"])
    assert np.array_equal(recs["linked"], orecs["linked"])


def _scan_equals_oracle(sc, sst, osc):
    ost = osc.stats()
    for key in ("n_junctions", "nb_jcheck_kmer", "nb_no_juncs", "nb_processed", "nb_skipped", "reads_no_errors",
                "unambiguous_reads", "reads_processed"):
        assert sst[key] == ost[key], key
    keys, recs = sc.junctions()
    okeys, orecs = osc.junctions("creation")
    assert np.array_equal(keys, okeys)
    assert np.array_equal(recs["dist"], orecs["dist"]) and np.array_equal(recs["cov"], orecs["cov"])
    assert np.array_equal(recs["linked"], orecs["linked"])


@pytest.mark.parametrize("n_rate", [0.0, 0.004])
def test_scan_reuses_the_resident_load_planes_only_for_the_same_reads(n_rate):
    """Scanning the batches that were loaded takes getValidReads' answer for every occurrence the load routed to bloo2
    from the kept plane (no probe); other reads, another batching, a replaced filter or FGPU_FLAG_NO_RESIDENT probe as
    usual.  The results are the oracle's in every case."""
    k, E, S = 31, 2_000_000, 400_000
    bases, offs = _random_case(20000, 100, k, 40000, 0.01, 77, n_rate, 3)
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)

    ctx = api.Context(k, tai, nh)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, 3))
    assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits()) and st["to_bloo2"] == lst.to_bloo2
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, 3))
    assert sst["valid_reused"] == lst.to_bloo2 > 0          # same reads, same batches: every routed occurrence is reused
    _scan_equals_oracle(sc, sst, osc)
    sst = sc.scanReads(chunks(bases, offs, 2))              # other batch boundaries: nothing lines up, nothing is reused
    assert sst["valid_reused"] == 0
    _scan_equals_oracle(sc, sst, osc)

    # other reads of the same shape against the same filter: the stream comparison must refuse them
    bases2, offs2 = _random_case(20000, 100, k, 40000, 0.01, 78, n_rate, 3)
    if len(bases2) == len(bases):
        osc2 = po.Scanner(k, 1, 100, b2)
        osc2.scan_reads(bases2, offs2)
        sst = sc.scanReads(chunks(bases2, offs2, 3))
        assert sst["valid_reused"] == 0
        _scan_equals_oracle(sc, sst, osc2)

    ctx.bloom_upload(L.BLOO2, b2.bits())                    # a filter from outside: the kept planes are dropped
    sst = sc.scanReads(chunks(bases, offs, 3))
    assert sst["valid_reused"] == 0
    _scan_equals_oracle(sc, sst, osc)

    ctx2 = api.Context(k, tai, nh, keep_resident=False)
    api.load_two_filters(api.Bloom(ctx2, L.BLOO1), api.Bloom(ctx2, L.BLOO2), chunks(bases, offs, 3))
    sc2 = api.ReadScanner(ctx2)
    sst = sc2.scanReads(chunks(bases, offs, 3))
    assert sst["valid_reused"] == 0
    _scan_equals_oracle(sc2, sst, osc)


def test_empty_and_degenerate_batches():
    ctx = api.Context(21, 1 << 19, 3)
    ctx.load_begin()
    ctx.load_batch(api.ReadBatch.from_lines([]))
    ctx.load_batch(api.ReadBatch.from_lines([b"", b"", b"ACGT", b"NNNN"]))
    st = ctx.load_end()
    assert st["kmers"] == 0 and st["reads_processed"] == 4 and st["unambiguous_reads"] == 0
    assert not ctx.bloom_download(L.BLOO2).any() and not ctx.bloom_download(L.BLOO1).any()
    ctx.scan_begin()
    ctx.scan_batch(api.ReadBatch.from_lines([b"", b"ACGT"]))
    s = ctx.scan_end()
    assert s["n_junctions"] == 0 and s["reads_processed"] == 2
    keys, recs = ctx.junctions()
    assert len(keys) == 0


def test_state_machine_errors():
    ctx = api.Context(21, 1 << 19, 3)
    with pytest.raises(api.FaucetGpuError):
        ctx.load_batch(api.ReadBatch.from_lines([b"ACGT"]))
    ctx.load_begin()
    with pytest.raises(api.FaucetGpuError):
        ctx.scan_begin()
    # during a load pass both filters live interleaved: the raw bit arrays are neither readable nor writable
    with pytest.raises(api.FaucetGpuError):
        ctx.bloom_download(L.BLOO2)
    with pytest.raises(api.FaucetGpuError):
        ctx.bloom_upload(L.BLOO1, np.zeros((1 << 19) // 8, dtype=np.uint8))
    with pytest.raises(api.FaucetGpuError):
        ctx.bloom_weight(L.BLOO1)
    ctx.load_end()
    assert ctx.bloom_weight(L.BLOO1) == 0.0
    with pytest.raises(api.FaucetGpuError):
        api.Context(32, 1 << 19, 3)
    with pytest.raises(api.FaucetGpuError):
        api.Context(21, 1000, 3)
    # fail planes exist for at most four hash functions.  A pass begun with FGPU_LOAD_SHARD_PLANES on a five-function context is a
    # plain load (it ran into a copy from planes that were never made), gives the plain load's filters, and the fix-up says STATE
    lines = [b"ACGTTGCAAGGCTTAACCGGTTACGATCGATCGGATCGATTAGCTAGCTAGGCTAGCTAGGATCGATCGAT", b"TTGACCAGTAGGACCATTGACGATTAGGCAGATTACAGGATTTACAGGCATTACAGAC"] * 50
    five, plain = api.Context(21, 1 << 19, 5), api.Context(21, 1 << 19, 5)
    batch = api.ReadBatch.from_lines(lines)
    five.load_begin(shard_planes=True)
    five.load_batch(batch)
    five.load_end()
    plain.load_begin()
    plain.load_batch(batch)
    plain.load_end()
    for which in (L.BLOO1, L.BLOO2):
        assert np.array_equal(five.bloom_download(which), plain.bloom_download(which))
    prefix, _ = plain.bloom_devptr(L.BLOO1)
    with pytest.raises(api.FaucetGpuError):
        five.load_fixup(prefix)


def test_ceiling_diagnostics_run_and_reject_bad_arguments():
    ctx = api.Context(21, 1 << 19, 3)
    assert ctx.diag_stream_copy(1 << 24, 2) > 1.0                     # GB/s
    for mode in (0, 1, 2):
        assert ctx.diag_random_access(1 << 22, 1 << 20, mode, 2) > 1e6   # accesses/s
    with pytest.raises(api.FaucetGpuError):
        ctx.diag_random_access(3 << 20, 1 << 20, 0, 1)                # not a power of two
    with pytest.raises(api.FaucetGpuError):
        ctx.diag_random_access(1 << 22, 1 << 20, 7, 1)


def test_two_shard_load_prefix_or_is_exact():
    """Multi-GPU pass 1 emulated with two contexts on one device: presence bitmaps, exclusive
    prefix-OR as the carried-in state of the later shard, OR of the shards' bloo2."""
    c = Case("ragged_k31")
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    parts = chunks(bases, offs, 2)
    ctxs = [api.Context(c.k, tai, nh) for _ in parts]
    for ctx, part in zip(ctxs, parts):
        ctx.presence_batch(part)
    p0, nbytes = ctxs[0].bloom_devptr(L.BLOO1)
    p1, _ = ctxs[1].bloom_devptr(L.BLOO1)
    pres0 = ctxs[0].bloom_download(L.BLOO1)
    # rank 0 starts from nothing, rank 1 from rank 0's presence bitmap
    ctxs[0].bloom_upload(L.BLOO1, np.zeros_like(pres0))
    ctxs[1].bloom_upload(L.BLOO1, pres0)
    for ctx, part in zip(ctxs, parts):
        ctx.load_begin(keep_carry=True)
        ctx.load_batch(part)
        ctx.load_end()
    q0, _ = ctxs[0].bloom_devptr(L.BLOO2)
    q1, _ = ctxs[1].bloom_devptr(L.BLOO2)
    ctxs[0].synchronize(); ctxs[1].synchronize()
    ctxs[0].bitmap_or(q0, q1, nbytes)
    assert np.array_equal(ctxs[0].bloom_download(L.BLOO2), c.bloom())


def test_two_shard_scan_table_handover_is_exact():
    import torch
    c = Case("c1_k21")
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    parts = chunks(bases, offs, 2)
    a = api.Context(c.k, tai, nh)
    b = api.Context(c.k, tai, nh)
    for ctx in (a, b):
        ctx.bloom_upload(L.BLOO2, c.bloom())
    a.scan_begin()
    a.scan_batch(parts[0])
    st_a = a.scan_end()
    n = a.table_entries()
    buf = torch.empty(max(n, 1) * L.TABLE_ENTRY_BYTES, dtype=torch.uint8, device="cuda")
    assert a.export_table(buf.data_ptr(), buf.numel()) == n
    torch.cuda.synchronize()
    b.scan_begin()
    b.import_table(buf.data_ptr(), n, carried=st_a)
    b.scan_batch(parts[1])
    st = b.scan_end()
    cn = c.counters
    assert st["n_junctions"] == cn["distinct_junctions"] and st["nb_processed"] == cn["nb_processed"]
    assert st["nb_skipped"] == cn["nb_skipped"] and st["nb_no_juncs"] == cn["nb_no_juncs"]
    assert st["reads_no_errors"] == cn["reads_no_errors"] and st["nb_jcheck_kmer"] == cn["nb_jcheck_kmer"]
    keys, recs = b.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines())


@pytest.mark.parametrize("how", [["-batch_reads", "400"], [], ["-chunk_mb", "1"]])
@pytest.mark.parametrize("name", ["c1_k21", "ragged_k31", "j2_spacer20_k15", "mercy_k21"])
def test_cli_writes_the_reference_files(name, how, tmp_path):
    """The stand-alone host: same flags as the reference, byte-identical .bloom and .junctions (dump order included)."""
    import os
    import subprocess
    c = Case(name)
    reads = tmp_path / "reads.fa"
    reads.write_bytes(c.reads_text())
    args = [a if not a.endswith(".fa") else str(reads) for a in c.meta["args"]]
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "faucet_amd", "faucet")
    r = subprocess.run([exe, "-read_load_file", str(reads), "-read_scan_file", str(reads), "-file_prefix", str(tmp_path / "out")]
                       + how + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(tmp_path / "out.bloom", dtype=np.uint8), c.bloom())
    assert (tmp_path / "out.junctions").read_text().split("\n")[:-1] == c.junction_lines()
    cn = c.counters
    assert f"Distinct junctions: {cn['distinct_junctions']} " in r.stdout
    assert f"Number of processed kmers: {cn['nb_processed']} " in r.stdout
    assert f"Reads processed: {cn['load_reads_processed']}" in r.stdout
    assert "Weights after load: %s, %s" % tuple(cn["weights_after_load"]) in r.stdout


@pytest.mark.parametrize("name", ["restart_bloomfile_k21", "restart_bloomfile_twohash_k21", "restart_bloomfile_fp6_k21"])
def test_cli_restarts_from_a_bloom_file_like_the_reference(name, tmp_path):
    """-bloom_file (src/Faucet.cpp:97-100,185-195,257-258): pass 1 is skipped, the filter is loaded from a file into a Bloom sized with
    create_bloom_filter_optimal(estimated_kmers, fpRate) -- fpRate, NOT the p1 a load from reads is sized with -- or, with --two_hash,
    create_bloom_filter_2_hash.  Golden: the compiled reference restarted from the .bloom of a normal run (tests/golden/make_restart_golden.py).
    The plain case pins the reference's quirk: the file holds 3 bits per k-mer, the restarted run asks for 4, nearly nothing is "present"
    and the junction file comes out empty; the --two_hash case (2 of the 3 bits asked for) finds 158 junctions."""
    import gzip
    import json
    import os
    import subprocess
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)
    meta = json.load(open(os.path.join(d, "case.json")))
    reads, bloom = tmp_path / "reads.fa", tmp_path / "in.bloom"
    reads.write_bytes(gzip.open(os.path.join(d, "reads.fa.gz")).read())
    bloom.write_bytes(gzip.open(os.path.join(d, "in.bloom.gz")).read())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "faucet_amd", "faucet")
    r = subprocess.run([exe, "-read_load_file", str(reads), "-read_scan_file", str(reads), "-file_prefix", str(tmp_path / "out"), "-bloom_file", str(bloom)]
                       + meta["args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Starting from after bloom load based on bloom file." in r.stdout
    want = gzip.open(os.path.join(d, "out.junctions.gz")).read()
    assert (tmp_path / "out.junctions").read_bytes() == want                      # dump order included
    assert not (tmp_path / "out.bloom").exists()                                  # the reference dumps no .bloom on this path
    cn = meta["counters"]
    assert f"Bits per kmer: {cn['bits_per_kmer']} " in r.stdout
    for label, key in (("Distinct junctions: ", "distinct_junctions"), ("Number of kmers that we j-checked: ", "nb_jcheck_kmer"),
                       ("Number of processed kmers: ", "nb_processed"), ("Number of skipped kmers: ", "nb_skipped"), ("Reads without errors: ", "reads_no_errors")):
        assert f"{label}{cn[key]}" in r.stdout, label
    # a .bloom of another size is taken the way Bloom::load takes it (utils/Bloom.cpp:580-587: fread of what is there, the rest of the zeroed
    # filter stays empty) -- until round 4 it was refused; tests/test_gpu_vs_reference_fuzz.py runs such restarts against the compiled reference
    (tmp_path / "short.bloom").write_bytes(bloom.read_bytes()[:1000])
    r = subprocess.run([exe, "-read_load_file", str(reads), "-read_scan_file", str(reads), "-file_prefix", str(tmp_path / "out2"), "-bloom_file",
                        str(tmp_path / "short.bloom")] + meta["args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "holds 1000 of the" in r.stderr and (tmp_path / "out2.junctions").exists()


def test_cli_restarts_from_junction_files_like_the_reference(tmp_path):
    """-junctions_file <prefix> (needs -bloom_file; src/Faucet.cpp:104-109,130-134,289-293): both passes are skipped, <prefix>.junctions and the two
    pair filters are reloaded (JunctionMap::buildFromFile, utils/JunctionMap.cpp:619-639; Bloom::load).  The contig graph that follows in the
    reference is not part of this build: the CLI reloads and checks the files, prints what the reference prints after reloading them (pair
    filter weights, number of junctions: golden = the compiled reference's own lines) and stops with its "contig graph not built" code 3."""
    import gzip
    import json
    import os
    import subprocess
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "restart_junctions_k21")
    meta = json.load(open(os.path.join(d, "case.json")))
    for ext in ("bloom", "junctions", "short_pair_filter", "long_pair_filter"):
        (tmp_path / ("pe." + ext)).write_bytes(gzip.open(os.path.join(d, "in." + ext + ".gz")).read())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "faucet_amd", "faucet")
    base = [exe, "-read_load_file", "unused.fq", "-read_scan_file", "unused.fq", "-file_prefix", str(tmp_path / "again"), "-bloom_file", str(tmp_path / "pe.bloom")]
    r = subprocess.run(base + ["-junctions_file", str(tmp_path / "pe")] + meta["args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, r.stdout[-1500:] + r.stderr[-1500:]
    for line in meta["stdout_after_reload"]:
        if line.startswith("Size of junction"):        # sizeof(Junction), a debugging print of the reference
            continue
        assert line in r.stdout, line
    assert not (tmp_path / "again.junctions").exists()
    # without -bloom_file the reference refuses (exit code 1); a truncated pair filter is half-read as the reference half-reads it
    r = subprocess.run([exe, "-read_load_file", "u", "-read_scan_file", "u", "-file_prefix", "x", "-junctions_file", str(tmp_path / "pe")] + meta["args"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Cannot start from junctions without a bloom file." in r.stderr
    (tmp_path / "pe.long_pair_filter").write_bytes(b"\0" * 100)           # (taken the way Bloom::load takes it since round 4: what fits, the rest empty)
    r = subprocess.run(base + ["-junctions_file", str(tmp_path / "pe")] + meta["args"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "is not of the" in r.stderr


@pytest.mark.parametrize("force_lazy_fail", [False, True])
def test_cli_reads_both_passes_from_named_pipes(tmp_path, force_lazy_fail):
    """The reference's streaming scripts (src/stream_data_from_urls_list.sh) feed both passes through pipes: the host must read its
    inputs strictly sequentially, never seek or ask for a size -- and never need them twice: with FGPU_DEBUG_LAZY_FAIL=1 every lazy scan
    meets the failure that round 1 answered by opening the scan input again (on a pipe: a hang, or an empty second scan -- ADVICE r1);
    the library now scans its own copy of the batches again, so pipes are scanned lazily like files and nothing is read twice."""
    import os
    import subprocess
    import threading
    c = Case("ragged_k31")
    text = c.reads_text()
    pipes = [str(tmp_path / "load.fifo"), str(tmp_path / "scan.fifo")]
    for p in pipes:
        os.mkfifo(p)

    def feed(path):
        with open(path, "wb") as f:                      # blocks until the CLI opens its end
            for lo in range(0, len(text), 777):          # odd-sized writes: short reads on the other side
                f.write(text[lo:lo + 777])
                f.flush()

    feeders = [threading.Thread(target=feed, args=(p,), daemon=True) for p in pipes]
    for t in feeders:
        t.start()
    args = [a for a in c.meta["args"] if not a.endswith(".fa")]
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "faucet_amd", "faucet")
    env = dict(os.environ, FGPU_DEBUG_LAZY_FAIL="1") if force_lazy_fail else None
    r = subprocess.run([exe, "-read_load_file", pipes[0], "-read_scan_file", pipes[1], "-file_prefix", str(tmp_path / "out")] + args,
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    for t in feeders:
        t.join(timeout=10)
        assert not t.is_alive()
    assert np.array_equal(np.fromfile(tmp_path / "out.bloom", dtype=np.uint8), c.bloom())
    assert (tmp_path / "out.junctions").read_text().split("\n")[:-1] == c.junction_lines()


def _oracle_lists(bases, offs, k, j, spacer, bloom_bits, tai, nh):
    """scanInputRead's return value for every read, from the oracle driven read by read"""
    b2 = po.Bloom(tai, nh)
    b2.set_bits(bloom_bits)
    osc = po.Scanner(k, j, spacer, b2)
    lists = []
    for i in range(len(offs) - 1):
        lists.append([int(x) for x in osc.scan_input_read(bytes(bases[int(offs[i]):int(offs[i + 1])]))])
    return osc, lists


@pytest.mark.parametrize("n_batches,capacity", [(1, 0), (4, 0), (12, 1 << 10)])
@pytest.mark.parametrize("n_rate", [0.0, 0.004])
def test_scan_input_read_lists_match_the_oracle(n_batches, n_rate, capacity):
    """fgpu_scan_take_stops = the list scanInputRead returns per read (src/ReadScanner.cpp:260-282), batch by batch -- also
    when the junction table is rehashed into larger ones between the batches (capacity: its initial slots)."""
    k, E, S = 25, 1_000_000, 200_000
    bases, offs = _random_case(12000, 110, k, 30000, 0.012, 99, n_rate, 3)
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    _, want = _oracle_lists(bases, offs, k, 1, 100, b2.bits(), tai, nh)
    ctx = api.Context(k, tai, nh, record_stops=True, junction_capacity=capacity)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    parts = chunks(bases, offs, n_batches)
    got = []
    ctx.scan_begin()
    first_read = 0
    bounds = []
    for part in parts:
        ctx.scan_batch(part)
        bounds.append(first_read)
        first_read += part.n_reads
    sst = ctx.scan_end()
    seqs = []
    while True:
        t = ctx.take_stops()
        if t is None:
            break
        seq, st = t
        seqs.append(seq)
        lists = [[] for _ in range(parts[seq].n_reads)]
        assert np.all(np.diff(st["read"].astype(np.int64)) >= 0)          # reads in file order
        for e in st:
            lists[int(e["read"])].append(int(e["ext"]))
        got.extend(lists)
        # every piece contributes at least one element and starts with FIRST; a fake element is alone in its piece
        first = (st["info"] & L.STOP_FIRST) != 0
        fake = (st["info"] & L.STOP_FAKE) != 0
        assert first.sum() > 0 and np.all(first[fake])
    assert seqs == list(range(len(parts)))
    assert got == want
    _scan_equals_oracle(ctx, sst, osc)


@pytest.mark.parametrize("lists_to_host", [True, False])
def test_short_pair_filter_on_the_device_equals_the_oracles(lists_to_host):
    """fgpu_scan_short_pairs: scan_forward's addPair rules (src/ReadScanner.cpp:208-225) applied on the device to every piece's list; the filter
    that comes back equals the one the oracle's scan builds with cleaning on.  Without lists to the host nothing is handed out.  (A scan that
    replays itself repeats some adds, which are idempotent: the paired-end CLI test with FGPU_DEBUG_LAZY_FAIL covers that.)"""
    k, E, S = 25, 1_000_000, 200_000
    bases, offs = _random_case(12000, 110, k, 30000, 0.012, 99, 0.003, 3)
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, _ = oracle_run((bases, offs), k, tai, nh, 1, 100)
    _, ptai, pnh = api.size_optimal(E // 20, np.float32(0.01))      # the short filter of src/Faucet.cpp:266-283
    short = po.Bloom(ptai, pnh)
    osc = po.Scanner(k, 1, 100, b2, short_pf=short)
    osc.scan_reads(bases, offs, paired_ends=False, no_cleaning=False)
    ctx = api.Context(k, tai, nh, record_stops=True)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    ctx.scan_short_pairs(ptai, pnh, lists_to_host)
    for attempt in range(2):                 # the second scan starts from an empty filter again
        ctx.scan_begin()
        for part in chunks(bases, offs, 5):
            ctx.scan_batch(part)
        ctx.scan_end()
        taken = 0
        while ctx.take_stops() is not None:
            taken += 1
        assert taken == (5 if lists_to_host else 0)
        got = ctx.scan_short_pairs_download(ptai)
        assert got.any() and np.array_equal(got, short.bits())
    with pytest.raises(api.FaucetGpuError):
        api.Context(k, tai, nh).scan_short_pairs(ptai, pnh)              # needs FGPU_FLAG_RECORD_STOPS


def _paired_oracle(bases, offs, k, tai, nh, E, no_cleaning=False):
    """the oracle's scan with both pair filters: (bloo2, short filter, long filter, scanner)"""
    b1, b2, lst, _ = oracle_run((bases, offs), k, tai, nh, 1, 100)
    _, stai, snh = api.size_optimal(E // 20, np.float32(0.01))       # src/Faucet.cpp:266-283
    _, ltai, lnh = api.size_optimal(E // 10, np.float32(0.01))
    short, long_ = po.Bloom(stai, snh), po.Bloom(ltai, lnh)
    osc = po.Scanner(k, 1, 100, b2, short_pf=short, long_pf=long_)
    osc.scan_reads(bases, offs, paired_ends=True, no_cleaning=no_cleaning)
    return b2, short, long_, osc


def _pairs_in_repeats(n_pairs, seed):
    """read pairs of a small genome with planted repeats at very high coverage: both ends of a pair hold dozens of junctions, the same
    (k-mer, k-mer) pairs recur in many read pairs -- the lists on which the long-pair loop's check-then-insert order matters"""
    g = synth.make_genome(12_000, seed, repeats=8, repeat_len=400)
    r = synth.make_pairs(g, n_pairs, 100, 260, 20, 0.01, seed + 1)
    return po.reads_from_matrix(np.ascontiguousarray(r))


@pytest.mark.parametrize("n_chunks", [pytest.param(1, marks=pytest.mark.slow), 4, pytest.param(7, marks=pytest.mark.slow)])
def test_long_pair_filter_on_the_device_equals_the_oracles(n_chunks):
    """fgpu_scan_long_pairs: scanReads' paired-end loop (src/ReadScanner.cpp:317-343; check with Bloom::containsPair, insert with addPair, in
    file order) on the device.  Both pair filters and the two pair counts equal the oracle's whatever the batching -- 7 chunks of an odd
    number of reads each leave first ends waiting for the next batch -- and nothing is handed to the host."""
    k, E, S = 21, 400_000, 150_000
    bases, offs = _pairs_in_repeats(20_001, 5)            # an odd number of pairs and chunks that cut pairs in two
    tai, nh = api.load_filter_shape(E, S)
    b2, short, long_, osc = _paired_oracle(bases, offs, k, tai, nh, E)
    ost = osc.stats()
    ctx = api.Context(k, tai, nh, record_stops=True)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    ctx.scan_short_pairs(short.tai, short.n_hash, False)
    ctx.scan_long_pairs(long_.tai, long_.n_hash, 2)
    for attempt in range(2):                               # a second scan starts from empty filters and counts again
        ctx.scan_begin()
        for part in chunks(bases, offs, n_chunks):
            ctx.scan_batch(part)
        sst = ctx.scan_end()
        assert ctx.take_stops() is None
        bits, empty, not_empty = ctx.scan_long_pairs_download(long_.tai)
        assert (empty, not_empty) == (ost["empty_count"], ost["not_empty_count"])
        assert bits.any() and np.array_equal(bits, long_.bits())
        assert np.array_equal(ctx.scan_short_pairs_download(short.tai), short.bits())
        d = ctx.diag_long_pairs()
        assert d["items"] > 0 and 0 < d["inserts"] <= d["items"] - d["paired_by_carry"] and d["rounds"] >= d["batches"] - 1
    _scan_equals_oracle(ctx, sst, osc)


@pytest.mark.parametrize("cuts", [pytest.param((0, 6002, 24000, 40000), marks=pytest.mark.slow), (0, 0, 13000, 13000, 40000),
                                  pytest.param((0, 2, 4, 6, 39998, 40000), marks=pytest.mark.slow)])
def test_python_host_hands_both_pair_filters_from_shard_to_shard(cuts, monkeypatch):
    """faucet_amd/sharded.py (the host of `bench.py --gpus N`): the pair filters travel with the junction table as they do in the C++ host
    (shard_host.h): the short one collects adds, the long one is check-then-insert in file order, shards begin at even records, the pair
    counts of the shards add up.  Ranks in turn in one process (run_in_turn), every shard in batches that cut pairs in two; shards of a
    single pair and empty shards among them."""
    import torch
    from faucet_amd import sharded
    monkeypatch.setenv("FGPU_DEBUG_DELTA_CHECK", "1")      # (round 5: a shard's planes merged with the new keys; this data found what the first version missed)
    k, E, S = 21, 400_000, 150_000
    bases, offs = _pairs_in_repeats(20_000, 5)
    assert len(offs) - 1 == cuts[-1]
    tai, nh = api.load_filter_shape(E, S)
    b2, short, long_, osc = _paired_oracle(bases, offs, k, tai, nh, E)
    ost = osc.stats()
    dev = torch.device("cuda", 0)
    shards = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        inner = sorted({lo, hi, lo + (hi - lo) // 3 | 1 if hi - lo > 3 else hi, lo + 2 * (hi - lo) // 3 if hi - lo > 3 else hi})   # odd cuts inside
        inner = [x for x in inner if lo <= x <= hi]
        shards.append([api.ReadBatch(bases, offs[a:b + 1].copy()) for a, b in zip(inner[:-1], inner[1:]) if b > a])
    counts = []

    def make():
        g = sharded.GpuShard(api.Context(k, tai, nh, record_stops=True), dev)
        g.pairs_setup(short=(short.tai, short.n_hash), long=(long_.tai, long_.n_hash))
        return g

    def after_scan(r, stats, backend):
        counts.append(backend.pair_counts())
        assert backend.ctx.diag_prepared_refresh()["mismatching_words"] == 0

    for protocol in ("fixup", "presence"):
        counts.clear()
        lst, sst, last = sharded.run_in_turn(make, shards, protocol, None, after_scan)
        assert (sum(c[0] for c in counts), sum(c[1] for c in counts)) == (ost["empty_count"], ost["not_empty_count"])
        assert np.array_equal(last.ctx.scan_short_pairs_download(short.tai), short.bits())
        bits, _, _ = last.ctx.scan_long_pairs_download(long_.tai)
        assert bits.any() and np.array_equal(bits, long_.bits())
        _scan_equals_oracle(last.ctx, sst, osc)
        last.close()


def test_long_pair_filter_with_ragged_reads_and_empty_records():
    """reads with N (several pieces per read, lists spliced over the pieces), empty records between them (each still toggles firstEnd) and
    batches without a single valid piece"""
    k, E, S = 25, 1_000_000, 200_000
    bases, offs = _random_case(12001, 110, k, 30000, 0.012, 99, 0.003, 3)
    lines = [bytes(bases[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]
    for at in (5, 6, 400, 2001, 2002, 2003, 9000):         # empty records shift which reads are mates
        lines.insert(at, b"")
    junk = [b"NNNN", b"", b"ACGTN"] * 7                     # a batch of 21 reads without any valid piece, in the middle
    batches = [api.ReadBatch.from_lines(x) for x in (lines[:3001], junk, lines[3001:3002], lines[3002:])]
    whole = api.ReadBatch.from_lines(lines[:3001] + junk + lines[3001:])
    allb, allo = whole.bases, whole.offsets
    tai, nh = api.load_filter_shape(E, S)
    b2, short, long_, osc = _paired_oracle(allb, allo, k, tai, nh, E)
    ost = osc.stats()
    ctx = api.Context(k, tai, nh, record_stops=True)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    ctx.scan_short_pairs(short.tai, short.n_hash, False)
    ctx.scan_long_pairs(long_.tai, long_.n_hash, 2)
    ctx.scan_begin()
    for b in batches:
        ctx.scan_batch(b)
    ctx.scan_end()
    bits, empty, not_empty = ctx.scan_long_pairs_download(long_.tai)
    assert (empty, not_empty) == (ost["empty_count"], ost["not_empty_count"])
    assert np.array_equal(bits, long_.bits())


def test_long_pair_counts_only_and_argument_checks():
    """--no_cleaning leaves only the two counts of the loop (FGPU_LONG_PAIRS_COUNT); the filter mode needs a power-of-two size and recorded lists"""
    k, E, S = 21, 400_000, 150_000
    bases, offs = _pairs_in_repeats(3000, 9)
    tai, nh = api.load_filter_shape(E, S)
    b2, short, long_, osc = _paired_oracle(bases, offs, k, tai, nh, E, no_cleaning=True)
    ost = osc.stats()
    assert not long_.bits().any()
    ctx = api.Context(k, tai, nh, record_stops=True)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    ctx.scan_long_pairs(0, 0, 1)
    ctx.scan_begin()
    for part in chunks(bases, offs, 3):
        ctx.scan_batch(part)
    ctx.scan_end()
    assert ctx.take_stops() is None
    bits, empty, not_empty = ctx.scan_long_pairs_download()
    assert bits is None and (empty, not_empty) == (ost["empty_count"], ost["not_empty_count"]) and not_empty > 0
    with pytest.raises(api.FaucetGpuError):
        ctx.scan_long_pairs(1000, 6, 2)                                   # not a power of two
    with pytest.raises(api.FaucetGpuError):
        api.Context(k, tai, nh).scan_long_pairs(long_.tai, long_.n_hash, 2)   # needs FGPU_FLAG_RECORD_STOPS
    ctx.scan_long_pairs(0, 0, 0)                                           # off again: the lists come to the host as before
    ctx.scan_begin()
    ctx.scan_batch(api.ReadBatch(bases, offs))
    ctx.scan_end()
    assert ctx.take_stops() is not None


def test_empty_batch_between_full_ones_does_not_replay_recycled_buffers():
    k, E, S = 25, 1_000_000, 200_000
    bases, offs = _random_case(9000, 100, k, 30000, 0.01, 5, 0.0, 2)
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    ctx = api.Context(k, tai, nh)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    parts = chunks(bases, offs, 3)
    empty = api.ReadBatch.from_lines([])
    ctx.scan_begin()
    for part in (parts[0], parts[1], empty, empty, parts[2], empty):
        ctx.scan_batch(part)
    sst = ctx.scan_end()
    _scan_equals_oracle(ctx, sst, osc)


@pytest.mark.parametrize("case", ["pe_fastq_k21", "pe_repeats_k25", "pe_fasta_highcov_k31", "pe_mercy_k21", "pe_twohash_k27"])
@pytest.mark.parametrize("batch_reads", [400, 333, 100000, 0])
def test_cli_paired_end_run_writes_the_reference_pair_filters(batch_reads, case, tmp_path):
    """BASELINE config 3's shape: --fastq --paired_ends WITHOUT --no_cleaning.  All four files the reference writes before
    its contig-graph stage are byte-identical (the long pair filter is check-then-insert, i.e. order-dependent); the
    program then stops with exit code 3 because that stage is not part of this build."""
    import os
    import subprocess
    # (round 4: pe_repeats_k25 -- repeats at high coverage, reads with N, truncated reads, records with an empty sequence line, which shift
    # who is whose mate -- and pe_fasta_highcov_k31 -- FASTA, --high_cov filter sizes, an odd number of records: tests/golden/make_pairs_golden.py)
    c = Case(case)
    reads = tmp_path / ("reads.fq" if c.fastq else "reads.fa")
    reads.write_bytes(c.reads_text())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "faucet_amd", "faucet")
    how = ["-batch_reads", str(batch_reads)] if batch_reads else []      # 0: the default, records split on the device
    r = subprocess.run([exe, "-read_load_file", str(reads), "-read_scan_file", str(reads), "-file_prefix", str(tmp_path / "out")]
                       + how + c.meta["args"], capture_output=True, text=True)
    assert r.returncode == 3, r.stderr
    assert np.array_equal(np.fromfile(tmp_path / "out.bloom", dtype=np.uint8), c.bloom())
    assert (tmp_path / "out.junctions").read_text().split("\n")[:-1] == c.junction_lines()
    assert np.array_equal(np.fromfile(tmp_path / "out.short_pair_filter", dtype=np.uint8), c.pair_filter("short"))
    assert np.array_equal(np.fromfile(tmp_path / "out.long_pair_filter", dtype=np.uint8), c.pair_filter("long"))
    cn = c.counters
    assert f"Empty count: {cn['empty_count']}, not empty count: {cn['not_empty_count']}" in r.stdout
    assert f"Distinct junctions: {cn['distinct_junctions']} " in r.stdout
    # with --no_cleaning the pair filters stay empty and are not written, the pair counts are still reported
    r = subprocess.run([exe, "-read_load_file", str(reads), "-read_scan_file", str(reads), "-file_prefix", str(tmp_path / "nc"),
                        "--no_cleaning"] + how + c.meta["args"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not (tmp_path / "nc.short_pair_filter").exists()
    assert f"Empty count: {cn['empty_count']}, not empty count: {cn['not_empty_count']}" in r.stdout
    assert "Weight of short pair filter: 0.000000" in r.stdout


@pytest.mark.parametrize("how", [["-batch_reads", "400"], [], ["-chunk_mb", "1"]])
def test_cli_single_end_run_with_cleaning_writes_the_reference_short_pair_filter(how, tmp_path):
    """Single-end reads, cleaning on (neither --no_cleaning nor --paired_ends): the reference writes `.bloom`, `.junctions` and
    `.short_pair_filter` before its contig-graph stage (golden se_cleaning_k21, tests/golden/make_cleaning_golden.py).  Here the short pair
    filter is filled on the device and no list reaches the host (fgpu_scan_short_pairs with lists_to_host = 0); exit code 3 as for every run
    that would go on to the contig graph."""
    import os
    import subprocess
    c = Case("se_cleaning_k21")
    reads = tmp_path / "reads.fa"
    reads.write_bytes(c.reads_text())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "faucet_amd", "faucet")
    r = subprocess.run([exe, "-read_load_file", str(reads), "-read_scan_file", str(reads), "-file_prefix", str(tmp_path / "out")]
                       + how + c.meta["args"], capture_output=True, text=True)
    assert r.returncode == 3, r.stderr
    assert np.array_equal(np.fromfile(tmp_path / "out.bloom", dtype=np.uint8), c.bloom())
    assert (tmp_path / "out.junctions").read_text().split("\n")[:-1] == c.junction_lines()
    short = c.pair_filter("short")
    assert short.any() and np.array_equal(np.fromfile(tmp_path / "out.short_pair_filter", dtype=np.uint8), short)
    assert not (tmp_path / "out.long_pair_filter").exists()
    assert f"Distinct junctions: {c.counters['distinct_junctions']} " in r.stdout


@pytest.mark.parametrize("log_tai,nh", [(33, 3), (32, 2)])
def test_config4_sized_filters_index_past_32_bits(log_tai, nh):
    """BASELINE config 4's filter shape (2^33 bits = 1 GiB per filter, 32 GiB of first-set times): bit positions, the
    interleaved pair, the carry sweep and the junction scan must all be 64-bit clean.  Small read set, full-size filters."""
    k, tai = 31, 1 << log_tai
    bases, offs = _random_case(60000, 100, k, 120000, 0.01, 2024, 0.001, 3)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    ctx = api.Context(k, tai, nh)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, 3))
    assert st["kmers"] == lst.kmers and st["to_bloo2"] == lst.to_bloo2
    got2 = ctx.bloom_download(L.BLOO2)
    want2 = b2.bits()
    assert np.array_equal(got2, want2)
    set_bits = np.flatnonzero(want2)
    assert set_bits.size and set_bits.max() >= (tai // 8) * 3 // 4           # the data does reach the top quarter of the array
    assert np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits())
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, 3))
    assert sst["valid_reused"] == lst.to_bloo2
    _scan_equals_oracle(sc, sst, osc)
    ctx.close()


def _load_split(ctx, text, fastq, chunk):
    """stream `text` through fgpu_text_split in chunks of `chunk` bytes, carrying the unconsumed tail, into a load pass"""
    ctx.load_begin()
    ctx.text_reserve(min(chunk, 1 << 20) + 4096 if chunk % 2 else 0)      # (with and without the hint of the largest chunk: same results)
    carry, pos, n_reads = b"", 0, 0
    while True:
        nxt = text[pos:pos + chunk]
        pos += len(nxt)
        final = pos >= len(text)
        buf = carry + nxt
        rb, used = ctx.text_split(buf, fastq, final)
        if rb.n_reads:
            ctx.load_batch(rb)
            n_reads += rb.n_reads
        carry = buf[used:]
        if final:
            assert used == len(buf)
            break
    return ctx.load_end(), n_reads


@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21", "ragged_k31"])
@pytest.mark.parametrize("chunk", [1 << 30, 4099, 997])
def test_device_record_splitting_reproduces_the_reference_bloom(name, chunk):
    c = Case(name)
    text = c.reads_text()
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer)
    st, n_reads = _load_split(ctx, text, c.fastq, chunk)
    assert n_reads == len(c.lines()) == st["reads_processed"]
    assert np.array_equal(ctx.bloom_download(L.BLOO2), c.bloom())
    # and the scan of a split batch (whole text) gives the reference's junctions
    rb, used = ctx.text_split(text, c.fastq, True)
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads([rb])
    keys, recs = sc.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines())
    assert sst["valid_reused"] == 0 or chunk == 1 << 30        # same batch as the load only when the load was one chunk


@pytest.mark.parametrize("fastq", [False, True])
def test_device_record_splitting_edge_cases_follow_getline(fastq):
    k = 5
    seqs = [b"ACGTTGCATGCA", b"", b"ACGTNNACGTACGTAC", b"TTTTTTTTTT\r", b"acgtACGTACGTAA", b"GATTACAGATTACA"]
    def record(i, s):
        return (b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n") if fastq else (b">r%d\n" % i + s + b"\n")
    full = b"".join(record(i, s) for i, s in enumerate(seqs))
    texts = [full, full[:-1],                       # no final newline
             full + b"GATTACATTGCA\n",                   # header (any line: here one with k-mers of its own) without a sequence line: an empty read
             full + b"GATTACATTGCA",                     # ... unterminated: the reference's one string still holds it when the sequence's getline fails -- the read
             full + (b"@x\nACGTACGTAC" if fastq else b">x\nACGTACGTAC"),   # unterminated sequence line / missing FASTQ tail
             full + (b"@x\nACGTACGTAC\n+" if fastq else b">x\nACGTACGTAC\n>y"),
             b"\n\n" + full, b"", b"\n", b"ACGT", b"ACGTTGCATT"]       # (a single line without a newline: header and read at once)
    for text in texts:
        want = getline_ref.reads(text, fastq)      # (tests/getline_ref.py: the reading loop as a stream simulation, pinned to the compiled reference)
        for chunk in (1 << 20, 7, 23):
            ctx = api.Context(k, 1 << 12, 2)
            st, n_reads = _load_split(ctx, text, fastq, chunk)
            assert n_reads == len(want), (text, chunk)
            ref = api.Context(k, 1 << 12, 2)
            ref.load_begin()
            if want:
                ref.load_batch(api.ReadBatch.from_lines(want))
            rst = ref.load_end()
            assert st["kmers"] == rst["kmers"] and st["unambiguous_reads"] == rst["unambiguous_reads"], (text, chunk)
            assert np.array_equal(ctx.bloom_download(L.BLOO1), ref.bloom_download(L.BLOO1)), (text, chunk)
            assert np.array_equal(ctx.bloom_download(L.BLOO2), ref.bloom_download(L.BLOO2)), (text, chunk)


def _check_against_oracle(bases, offs, k, E, S, j, spacer=100, load_chunks=3, scan_chunks=2, **ctx_kw):
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, j, spacer)
    ctx = api.Context(k, tai, nh, j=j, max_spacer_dist=spacer, **ctx_kw)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, load_chunks))
    assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits()) and np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits())
    assert st["kmers"] == lst.kmers and st["to_bloo2"] == lst.to_bloo2
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, scan_chunks))
    _scan_equals_oracle(sc, sst, osc)
    return sst


def test_reads_of_two_thousand_bases():
    """pieces far beyond the 128 windows the walk keeps in registers"""
    bases, offs = _random_case(1500, 2000, 31, 60000, 0.01, 11, 0.0005, 4)
    _check_against_oracle(bases, offs, 31, 2_000_000, 400_000, 1)


@pytest.mark.parametrize("j", [3, 4])
def test_deeper_jcheck(j):
    bases, offs = _random_case(10000, 120, 23, 15000, 0.02, 70 + j, 0.0, 6)
    _check_against_oracle(bases, offs, 23, 800_000, 200_000, j)


@pytest.mark.parametrize("period,k", [(7, 15), (53, 21), (200, 31)])
def test_periodic_genome_tandem_repeats(period, k):
    """the same k-mer many times inside one piece and in every piece: created-key tracking inside clusters, giant clusters"""
    rng = np.random.default_rng(period)
    unit = synth._ACGT[rng.integers(0, 4, size=period)]
    genome = np.tile(unit, 40000 // period + 2)[:40000].copy()
    mut = rng.random(genome.shape) < 0.002                      # a few point differences between the copies
    genome[mut] = synth._ACGT[rng.integers(0, 4, size=int(mut.sum()))]
    r = synth.make_reads(genome, 6000, 150, 0.004, period + 1)
    bases, offs = po.reads_from_matrix(r)
    sst = _check_against_oracle(bases, offs, k, 500_000, 100_000, 1, scan_chunks=3)
    assert sst["walk_max_cluster"] >= 2


def test_many_tiny_reads_and_small_spacer():
    """reads shorter than a 64-position word (the pack kernel's slow path), shorter than k, empty; spacer rule firing often"""
    rng = np.random.default_rng(5)
    g = synth.make_genome(5000, 9)
    lines = []
    for _ in range(30000):
        ln = int(rng.integers(0, 70))
        s = int(rng.integers(0, 5000 - 70))
        lines.append(bytes(g[s:s + ln]))
    bases, offs = po.reads_from_lines(lines)
    _check_against_oracle(bases, offs, 11, 200_000, 50_000, 1, spacer=6, load_chunks=4, scan_chunks=5)


@pytest.mark.parametrize("max_len", [12, 26, 45])
def test_reads_shorter_than_a_code_word_contiguous_and_inside_raw_text(max_len):
    """64 consecutive reads that do not span the 2048 positions of one trip of the pack kernel (its bisection over the offsets in
    memory), several read boundaries inside the 32 positions of one lane, empty reads, bad characters -- as a contiguous batch and
    as reads lying inside raw FASTA text (fgpu_reads.starts)."""
    rng = np.random.default_rng(max_len)
    g = synth.make_genome(3000, 21)
    lines = []
    for _ in range(40000):
        ln = int(rng.integers(0, max_len + 1))
        s = int(rng.integers(0, 3000 - max_len))
        r = g[s:s + ln].copy()
        if ln and rng.random() < 0.05:
            r[int(rng.integers(0, ln))] = ord("N")
        lines.append(bytes(r))
    bases, offs = po.reads_from_lines(lines)
    k = 7
    _check_against_oracle(bases, offs, k, 100_000, 20_000, 1, spacer=5, load_chunks=3, scan_chunks=2)
    tai, nh = api.load_filter_shape(100_000, 20_000)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 5)
    text = b"".join(b">r%d\n" % i + ln + b"\n" for i, ln in enumerate(lines))
    ctx = api.Context(k, tai, nh, j=1, max_spacer_dist=5)
    st, n_reads = _load_split(ctx, text, False, 50_000)
    assert n_reads == len(lines) and st["kmers"] == lst.kmers
    assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits()) and np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits())
    rb, used = ctx.text_split(text, False, True)
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads([rb])
    _scan_equals_oracle(sc, sst, osc)


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_small_inputs_against_the_oracle(seed):
    """random k, j, spacer, read lengths, alphabets and batchings on small inputs (where corner cases live)"""
    rng = np.random.default_rng(1000 + seed)
    k = int(rng.integers(3, 32))
    j = int(rng.integers(0, 4))
    spacer = int(rng.choice([2, 5, 20, 100]))
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
        if rng.random() < 0.5:
            r = synth._COMP[r[::-1]]
            r[r == 0] = ord("N")
        lines.append(bytes(r))
    bases, offs = po.reads_from_lines(lines)
    tai = 1 << int(rng.integers(10, 20))
    nh = int(rng.integers(1, 5))
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, j, spacer)
    ctx = api.Context(k, tai, nh, j=j, max_spacer_dist=spacer, walk_window_span=int(rng.choice([0, 64, 1000, 1 << 16])),
                      record_stops=bool(rng.integers(0, 2)))
    nlb, nsb = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, nlb))
    assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits()) and np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits())
    assert st["kmers"] == lst.kmers and st["to_bloo2"] == lst.to_bloo2 and st["unambiguous_reads"] == lst.unambiguous_reads
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, nsb))
    _scan_equals_oracle(sc, sst, osc)


def test_the_library_absorbs_a_failed_lazy_check(tmp_path, monkeypatch):
    """FGPU_DEBUG_LAZY_FAIL=1 makes every lazy scan meet the one failure its self-check cannot repair.  The library keeps the packed
    batches of a lazy scan in HBM and scans them again by itself with every junction test evaluated (fgpu_diag_scan_replays counts it):
    the callers see an ordinary scan -- same files through the CLI (paired-end lists included: none handed out twice), same records
    through the Python mirror, streaming and prepared, and also when the journal is too small to hold the scan (FGPU_JOURNAL_MB=0: the
    scan is checked, then goes on eagerly)."""
    import os
    import subprocess
    c = Case("pe_fastq_k21")
    reads = tmp_path / "reads.fq"
    reads.write_bytes(c.reads_text())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "faucet_amd", "faucet")
    for extra in ({}, {"FGPU_JOURNAL_MB": "0"}):
        env = dict(os.environ, FGPU_DEBUG_LAZY_FAIL="1", **extra)
        r = subprocess.run([exe, "-read_load_file", str(reads), "-read_scan_file", str(reads), "-file_prefix", str(tmp_path / "out"),
                            "-batch_reads", "300"] + c.meta["args"], capture_output=True, text=True, env=env)
        assert r.returncode == 3, r.stderr
        assert (tmp_path / "out.junctions").read_text().split("\n")[:-1] == c.junction_lines()
        assert np.array_equal(np.fromfile(tmp_path / "out.short_pair_filter", dtype=np.uint8), c.pair_filter("short"))
        assert np.array_equal(np.fromfile(tmp_path / "out.long_pair_filter", dtype=np.uint8), c.pair_filter("long"))
    # the same through the Python mirror, in a child process (the knob is read once per process)
    code = (
        "import numpy as np\n"
        "from faucet_amd import _lib as L, api\n"
        "from oracle import pyoracle as po\n"
        "from tests.golden_util import Case\n"
        "from tests.test_gpu_parity import chunks\n"
        "c = Case('ragged_k31')\n"
        "bases, offs = po.reads_from_lines(c.lines())\n"
        "tai, nh = api.load_filter_shape(c.E, c.S, c.fp)\n"
        "want = sorted(c.junction_lines())\n"
        "for mode in ('stream', 'prepared'):\n"
        "    ctx = api.Context(c.k, tai, nh, walk_window_span=512)\n"
        "    ctx.bloom_upload(L.BLOO2, c.bloom())\n"
        "    ctx.scan_begin()\n"
        "    for b in chunks(bases, offs, 5):\n"
        "        ctx.scan_batch(b) if mode == 'stream' else ctx.scan_prepare(b)\n"
        "    if mode == 'prepared':\n"
        "        ctx.scan_walk_prepared()\n"
        "    st = ctx.scan_end()\n"
        "    keys, recs = ctx.junctions()\n"
        "    assert ctx.diag_scan_replays() == 1, (mode, ctx.diag_scan_replays())\n"
        "    assert st['reads_processed'] == len(offs) - 1\n"
        "    assert sorted(api.junction_lines(keys, recs, c.k)) == want, mode\n"
        "    for key, val in (('nb_processed', c.counters['nb_processed']), ('nb_skipped', c.counters['nb_skipped']), ('nb_jcheck_kmer', c.counters['nb_jcheck_kmer'])):\n"
        "        assert st[key] == val, (mode, key)\n"
        "print('absorbed ok')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FGPU_DEBUG_LAZY_FAIL="1")
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=root)
    assert r.returncode == 0 and "absorbed ok" in r.stdout, r.stdout + r.stderr


def test_a_replay_applies_the_long_pair_loop_to_every_batch_once():
    """with the lists ALSO handed to the host (fgpu_scan_short_pairs(..., lists_to_host = 1)) a replay harvests every batch the caller
    has not taken yet a second time; the device's check-then-insert loop (fgpu_scan_long_pairs) must see each batch once all the same.
    FGPU_DEBUG_LAZY_FAIL=4 forces the replay once four batches have been prepared -- lists of earlier batches are harvested by then."""
    import os
    import subprocess
    code = (
        "import numpy as np\n"
        "from faucet_amd import _lib as L, api\n"
        "from tests.test_gpu_parity import chunks, _paired_oracle, _pairs_in_repeats\n"
        "k, E, S = 21, 400_000, 150_000\n"
        "bases, offs = _pairs_in_repeats(20_001, 5)\n"
        "tai, nh = api.load_filter_shape(E, S)\n"
        "b2, short, long_, osc = _paired_oracle(bases, offs, k, tai, nh, E)\n"
        "ost = osc.stats()\n"
        "for take_during in (False, True):\n"
        "    ctx = api.Context(k, tai, nh, record_stops=True)\n"
        "    ctx.bloom_upload(L.BLOO2, b2.bits())\n"
        "    ctx.scan_short_pairs(short.tai, short.n_hash, True)\n"
        "    ctx.scan_long_pairs(long_.tai, long_.n_hash, 2)\n"
        "    ctx.scan_begin()\n"
        "    seqs = []\n"
        "    for i, part in enumerate(chunks(bases, offs, 7)):\n"
        "        ctx.scan_batch(part)\n"
        "        if take_during and i in (1, 2):\n"
        "            t = ctx.take_stops()\n"
        "            if t is not None: seqs.append(t[0])\n"
        "    ctx.scan_end()\n"
        "    while True:\n"
        "        t = ctx.take_stops()\n"
        "        if t is None: break\n"
        "        seqs.append(t[0])\n"
        "    assert seqs == list(range(7)), seqs\n"
        "    assert ctx.diag_scan_replays() == 1, ctx.diag_scan_replays()\n"
        "    bits, empty, not_empty = ctx.scan_long_pairs_download(long_.tai)\n"
        "    assert (empty, not_empty) == (ost['empty_count'], ost['not_empty_count']), (empty, not_empty)\n"
        "    assert np.array_equal(bits, long_.bits())\n"
        "    assert np.array_equal(ctx.scan_short_pairs_download(short.tai), short.bits())\n"
        "print('once each ok')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FGPU_DEBUG_LAZY_FAIL="4")
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=root)
    assert r.returncode == 0 and "once each ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("case", ["c1_k21", "ragged_k31", "mercy_k21", "twohash_k31_L150", "pe_repeats_k25"])
def test_load_pass_with_256_byte_records_gives_the_reference_filter(case, tmp_path):
    """FGPU_LOAD_LAYOUT=records (load_common.h, Filt<1>; round 5, measured and not the default): the pass keeps {bloo1 word, bloo2 word, 32 first-set
    times} in one aligned 256-byte record per 32 filter bits instead of the interleaved pair + first[] -- same algorithm, other addresses; the
    reference's files come out, --mercy (times of every bit) and several batches with their sweeps included, and with -gpus 2 the fix-up
    protocol reads its times from the records"""
    import os
    import subprocess
    c = Case(case)
    reads = tmp_path / ("reads.fq" if c.fastq else "reads.fa")
    reads.write_bytes(c.reads_text())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "faucet_amd", "faucet")
    for extra in (["-batch_reads", "97"], ["-gpus", "2"]):
        prefix = tmp_path / ("out" + extra[0])
        r = subprocess.run([exe, "-read_load_file", str(reads), "-read_scan_file", str(reads), "-file_prefix", str(prefix)] + extra + c.meta["args"],
                           capture_output=True, text=True, env=dict(os.environ, FGPU_LOAD_LAYOUT="records"), timeout=600)
        assert r.returncode == (0 if c.no_cleaning else 3), r.stderr[-2000:]
        assert np.array_equal(np.fromfile(str(prefix) + ".bloom", dtype=np.uint8), c.bloom())
        assert open(str(prefix) + ".junctions").read().split("\n")[:-1] == c.junction_lines()
        w = c.counters["weights_after_load"]
        assert f"Weights after load: {w[0]}, {w[1]}" in r.stdout.replace("\r", "\n")


@pytest.mark.parametrize("n_batches", [1, 5])
def test_mercy_load_matches_the_reference(n_batches):
    """load_two_filters(..., mercy = true) (utils/Bloom.cpp:300-333): the reference's --mercy .bloom, byte for byte, and it does
    differ from the plain load on this low-coverage fixture"""
    c = Case("mercy_k21")
    assert c.mercy and not np.array_equal(c.bloom(), Case("nomercy_k21").bloom())
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    ctx = api.Context(c.k, tai, nh, mercy=True)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, n_batches))
    assert np.array_equal(ctx.bloom_download(L.BLOO2), c.bloom())
    w = c.counters["weights_after_load"]
    assert f"{ctx.bloom_weight(L.BLOO1):f}" == w[0] and f"{ctx.bloom_weight(L.BLOO2):f}" == w[1]
    # the scan over that filter (resident planes in use) gives the reference's junctions
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, n_batches))
    keys, recs = sc.junctions()
    assert sorted(api.junction_lines(keys, recs, c.k)) == sorted(c.junction_lines())
    assert sst["n_junctions"] == c.counters["distinct_junctions"]


@pytest.mark.parametrize("seed", range(6))
def test_mercy_random_inputs_vs_oracle(seed):
    rng = np.random.default_rng(300 + seed)
    k = int(rng.choice([11, 21, 31]))
    G = int(rng.integers(3000, 30000))
    cov = float(rng.choice([2.0, 5.0, 12.0]))
    n = int(G * cov / 100)
    bases, offs = _random_case(n, 100, k, G, float(rng.choice([0.0, 0.01, 0.03])), 900 + seed, float(rng.choice([0.0, 0.003])), int(rng.integers(0, 4)))
    tai, nh = 1 << int(rng.integers(14, 20)), int(rng.integers(1, 5))
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    olst = po.load_two_filters(b1, b2, bases, offs, k, mercy=True)
    ctx = api.Context(k, tai, nh, mercy=True)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, int(rng.integers(1, 6))))
    assert np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits())
    assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits())
    assert st["to_bloo2"] == olst.to_bloo2 and st["kmers"] == olst.kmers


@pytest.mark.parametrize("d", kat("stage3"), ids=lambda d: d["case"])
def test_stage3_probes_on_device_match_the_reference(d):
    """the contig-graph stage's filter work (oldContains, jcheck, getValidJExtension, isBloomJunction), batched on the
    device, against the reference's own functions on the golden filters"""
    c = Case(d["case"])
    ctx = api.Context(d["k"], d["tai"], d["n_hash"], j=d["j"])
    ctx.bloom_upload(L.BLOO2, c.bloom())
    kmers = np.array([int(p[0], 16) for p in d["probes"]], dtype=np.uint64)
    canon = np.array([po.lib().fo_canon(int(x), d["k"]) for x in kmers], dtype=np.uint64)
    assert list(ctx.probe_contains(L.BLOO2, canon)) == [p[1] for p in d["probes"]]
    assert list(ctx.probe_jcheck(kmers)) == [p[2] for p in d["probes"]]
    assert list(ctx.probe_valid_extension(kmers)) == [p[3] for p in d["probes"]]
    assert list(ctx.probe_bloom_junction(kmers)) == [p[4] for p in d["probes"]]


def test_walk_evaluates_the_junction_tests_the_preview_left_out():
    """The need plane is only a preview: where the walk scans a window outside it, it runs testForJunction itself (and gives up
    loudly only if such a test comes out true, because the dependency clusters did not know that candidate).  With
    FGPU_DEBUG_NEED_DROP=1 (read once per process: child pytest) the evaluation of about half of the windows whose tests are false
    is thrown away after the flags kernel, so the walk re-evaluates them wherever it scans them -- long reads beyond the 128
    windows held in registers included -- and every scan test still has to agree with the oracle and the goldens."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FGPU_DEBUG_NEED_DROP="1")
    sel = ("test_scan_matches_reference_junctions or test_random_inputs_vs_oracle or test_reads_of_two_thousand_bases or "
           "test_periodic_genome or test_deeper_jcheck or test_scan_input_read_lists or test_many_tiny_reads")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-m", "gpu", "-q", "-x", "-k", sel],
                       capture_output=True, text=True, env=env, cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    # and the path was really taken: a scan in such a process reports the windows it tested itself
    code = ("import numpy as np\n"
            "from faucet_amd import _lib as L, api\n"
            "from oracle import pyoracle as po\n"
            "from tests.golden_util import Case\n"
            "c = Case('c1_k21')\n"
            "bases, offs = po.reads_from_lines(c.lines())\n"
            "tai, nh = api.load_filter_shape(c.E, c.S, c.fp)\n"
            "ctx = api.Context(c.k, tai, nh)\n"
            "ctx.bloom_upload(L.BLOO2, c.bloom())\n"
            "st = api.ReadScanner(ctx).scanReads([api.ReadBatch(bases, offs)])\n"
            "assert st['flags_filled'] > 1000 and st['nb_jcheck_kmer'] == c.counters['nb_jcheck_kmer'], st\n"
            "print('filled', st['flags_filled'])\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=root)
    assert r.returncode == 0 and "filled" in r.stdout, r.stdout + r.stderr


def test_a_late_junction_test_that_comes_out_true_voids_the_scan_only_if_its_kmer_is_shared():
    """A junction test the walk has to run itself (the preview left the position out) may come out TRUE at a k-mer no piece of the window
    registered: the walk goes on, and the window is checked afterwards -- only if that k-mer occurs on another piece of the same window
    is the scan void (and scanned again from the journal, eagerly).  Config 4's 2*10^10 positions meet the case about once per run.
    FGPU_DEBUG_NEED_DROP=2 (child processes: the variable is read once) throws away the evaluation of every position of one k-mer in 16 whatever the
    answer.  (a) reads that cover their genome 0.025x in one window: late tests noted, no second occurrence, NO replay, results the
    oracle's; (b) 50x: second occurrences, replay, results the oracle's; (c) the scan tests of this file under the same switch."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FGPU_DEBUG_NEED_DROP="2")
    code = ("import numpy as np\n"
            "from faucet_amd import _lib as L, api\n"
            "from oracle import pyoracle as po\n"
            "from tests.test_gpu_parity import _random_case, chunks\n"
            "k, E, S = 31, 20_000_000, 4_000_000\n"
            "tai, nh = api.load_filter_shape(E, S)\n"
            "seen = []\n"
            "for G, n_load, n_scan, seed, span in ((2_000_000, 200_000, 500, 5, 0), (2_000_000, 200_000, 500, 6, 0), (2_000_000, 200_000, 4_000, 5, 0),\n"
            "                                      (2_000_000, 200_000, 4_000, 6, 1 << 13), (40_000, 20_000, 20_000, 7, 0)):\n"
            "    bases, offs = _random_case(n_load, 100, k, G, 0.01, seed, 0.0, 0)\n"
            "    ctx = api.Context(k, tai, nh, walk_window_span=span)     # (span 2^13: the noted positions spread over ~50 windows, each swept by its own)\n"
            "    api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, 2))\n"
            "    b2 = po.Bloom(tai, nh)\n"
            "    b2.set_bits(ctx.bloom_download(L.BLOO2))\n"
            "    sb, so = bases[: offs[n_scan]], offs[: n_scan + 1]\n"
            "    osc = po.Scanner(k, 1, 100, b2)\n"
            "    osc.scan_reads(sb, so)\n"
            "    sc = api.ReadScanner(ctx)\n"
            "    sst = sc.scanReads([api.ReadBatch(sb, so)])\n"
            "    ost = osc.stats()\n"
            "    for key in ('n_junctions', 'nb_jcheck_kmer', 'nb_no_juncs', 'nb_processed', 'nb_skipped', 'reads_no_errors'):\n"
            "        assert sst[key] == ost[key], (key, sst[key], ost[key])\n"
            "    keys, recs = sc.junctions()\n"
            "    okeys, orecs = osc.junctions('creation')\n"
            "    assert np.array_equal(keys, okeys)\n"
            "    assert np.array_equal(recs['dist'], orecs['dist']) and np.array_equal(recs['cov'], orecs['cov']) and np.array_equal(recs['linked'], orecs['linked'])\n"
            "    late = ctx.diag_late_flags()\n"
            "    seen.append((late['noted'], late['conflicts'], ctx.diag_scan_replays()))\n"
            "    assert late['swept'] == late['noted'] or late['noted'] > 256, late   # the check passed over every noted position (a run-time guard too: pull_counters)\n"
            "    if span: assert sst['walk_windows'] > 20 and late['noted'] > 0, (sst['walk_windows'], late)\n"
            "    print('case', G, n_scan, span, seen[-1], 'junctions', len(keys))\n"
            "    ctx.close()\n"
            "assert any(n > 0 and c == 0 and r == 0 for n, c, r in seen), seen      # noted, checked, kept\n"
            "assert any(c > 0 and r == 1 for n, c, r in seen), seen                # found on another piece: scanned again\n"
            "assert all(r == 1 for n, c, r in seen if c > 0 or n > 256), seen\n"
            "print('LATE OK')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=root)
    assert r.returncode == 0 and "LATE OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    sel = ("test_scan_matches_reference_junctions or test_random_inputs_vs_oracle or test_reads_of_two_thousand_bases or "
           "test_periodic_genome or test_deeper_jcheck or test_scan_input_read_lists or test_many_tiny_reads")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-m", "gpu", "-q", "-x", "-k", sel],
                       capture_output=True, text=True, env=env, cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("mercy", [False, True])
@pytest.mark.parametrize("ratio", ["0/1", "1/1", "1/4", "1000000/1"])
def test_load_with_a_lagging_carry_is_exact(ratio, mercy, monkeypatch):
    """The carry is brought up to date (a sweep of first[]) only when an epoch has grown to FGPU_SWEEP_RATIO of what the carry
    covers; in between, first-set times run on across batches.  Every policy -- after every batch, doubling, never before
    load_end -- gives the oracle's two filters and counters on 13 uneven batches, with and without --mercy, and so does a second
    load pass on the same context (first[] and the epoch are reset by load_begin)."""
    monkeypatch.setenv("FGPU_SWEEP_RATIO", ratio)
    k, tai, nh = 21, 1 << 18, 3
    bases, offs = _random_case(1500, 100, k, 9000, 0.02, 4242, 0.003, 2)
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    olst = po.load_two_filters(b1, b2, bases, offs, k, mercy=mercy)
    ctx = api.Context(k, tai, nh, mercy=mercy)
    n = len(offs) - 1
    cuts = [0, 1, 3, 40, 41, 200, 420, 421, 700, 900, 1100, 1101, 1400, n]
    batches = [api.ReadBatch(bases, offs[a:b + 1].copy()) for a, b in zip(cuts[:-1], cuts[1:])]
    for _ in range(2):
        st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), batches)
        assert np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits())
        assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits())
        assert st["to_bloo2"] == olst.to_bloo2 and st["kmers"] == olst.kmers


def test_page_locked_and_overlapped_downloads_equal_the_plain_ones():
    """fgpu_bloom_download_begin / _wait (copy stream, page-locked destination, the scan submitted in between) and the junction
    download into page-locked buffers return what the blocking calls return; a load_begin issued while a download is in flight
    waits for it instead of rewriting the filter under the copy."""
    c = Case("ragged_k31")
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer)
    batches = chunks(bases, offs, 3)
    api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), batches)
    buf = api.HostBuffer(tai // 8)
    early = ctx.bloom_download_begin(L.BLOO2, buf)
    sc = api.ReadScanner(ctx)
    sc.scanReads(batches)
    keys_p, recs_p = ctx.junctions(pinned=True)
    ctx.bloom_download_wait()
    assert np.array_equal(early, c.bloom()) and np.array_equal(early, ctx.bloom_download(L.BLOO2))
    keys, recs = ctx.junctions()
    assert np.array_equal(keys, keys_p) and recs.tobytes() == recs_p.tobytes()
    assert sorted(api.junction_lines(keys_p, recs_p, c.k)) == sorted(c.junction_lines())
    # a download in flight when the next load pass starts
    first = ctx.bloom_download_begin(L.BLOO2, buf).copy
    ctx.load_begin()
    snapshot = first()
    ctx.load_end()
    assert np.array_equal(snapshot, c.bloom())
    with pytest.raises(ValueError):
        ctx.bloom_download_begin(L.BLOO2, api.HostBuffer(16))
    ctx.close()


def _saturated_filter_case(n_reads, seed):
    """10x reads over a genome whose k-mers overfill the filter they are given: bloo2 ends up ~40 % full, its false positives
    make every few positions look like a junction, and the scan creates several junction records PER READ (the data set on
    which a fixed-size table crawled: 34 M records from 10 M reads)"""
    k, G = 31, n_reads * 10
    bases, offs = _random_case(n_reads, 100, k, G, 0.01, seed)
    tai, nh = api.load_filter_shape(10 * n_reads, 2 * n_reads)
    return k, bases, offs, tai, nh


def test_junction_table_grows_between_batches():
    k, bases, offs, tai, nh = _saturated_filter_case(60_000, 77)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh)
    n_ref = osc.stats()["n_junctions"]
    assert n_ref > 40_000                                   # the better part of a record per read
    ctx = api.Context(k, tai, nh, junction_capacity=1 << 14)   # a quarter of it is passed with the first of 12 batches
    batches = chunks(bases, offs, 12)
    api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), batches)
    sc = api.ReadScanner(ctx)
    for _ in range(2):                                      # the second scan starts on the grown table
        sst = sc.scanReads(batches)
        _scan_equals_oracle(sc, sst, osc)
        assert sst["n_junctions"] == n_ref
    # the same through prepare-all + ordered walk (the multi-GPU ranks' path) on a fresh, small table
    ctx2 = api.Context(k, tai, nh, junction_capacity=1 << 14)
    api.load_two_filters(api.Bloom(ctx2, L.BLOO1), api.Bloom(ctx2, L.BLOO2), batches)
    ctx2.scan_begin()
    for b in batches:
        ctx2.scan_prepare(b)
    ctx2.scan_walk_prepared()
    sst2 = ctx2.scan_end()
    keys, recs = ctx2.junctions()
    k1, r1 = sc.junctions()
    assert sst2["n_junctions"] == n_ref and np.array_equal(keys, k1) and recs.tobytes() == r1.tobytes()


def test_a_batch_that_outgrows_the_junction_table_is_absorbed():
    """VERDICT r5 item 6a.  One batch, far more records than slots (utils/JunctionMap.h:61: the reference's unordered_map just grows): the library
    scans its journal again on a larger table -- twice here, 2^12 -> 2^14 -> 2^16 slots for ~10^4 records -- and the caller sees an ordinary scan with the
    oracle's map.  Also with the overflow in a LATER batch (the batches before it are replayed with it), with lists recorded (the oracle's
    lists, also when taken after every batch: none from a walk that overflowed), and -- no journal:
    eager flags -- still the prompt FGPU_ERR_CAPACITY with the advice, not a crawl through a saturated table."""
    k, bases, offs, tai, nh = _saturated_filter_case(30_000, 78)
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    po.load_two_filters(b1, b2, bases, offs, k)
    osc = po.Scanner(k, 1, 100, b2)
    osc.scan_reads(bases, offs)
    okeys, orecs = osc.junctions("creation")
    ost = osc.stats()
    assert len(okeys) > 4 * (1 << 12)
    _, want = _oracle_lists(bases, offs, k, 1, 100, b2.bits(), tai, nh)
    # (3, True, True): lists taken after every batch -- the first batch's walk overflows, and its lists are asked for while its flag is up
    for n_batches, record_stops, take_during in ((1, False, False), (3, False, False), (2, True, False), (3, True, True)):
        ctx = api.Context(k, tai, nh, junction_capacity=1 << 12, record_stops=record_stops)
        batches = chunks(bases, offs, n_batches)
        api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), batches)
        ctx.scan_begin()
        taken = []
        for b in batches:
            ctx.scan_batch(b)
            if take_during:
                t = ctx.take_stops()
                if t is not None:
                    taken.append(t)
        sst = ctx.scan_end()
        keys, recs = ctx.junctions()
        assert np.array_equal(keys, okeys) and np.array_equal(recs["dist"], orecs["dist"]) and np.array_equal(recs["cov"], orecs["cov"]) and \
            np.array_equal(recs["linked"], orecs["linked"]), (n_batches, record_stops)
        for key in ("n_junctions", "nb_jcheck_kmer", "nb_no_juncs", "nb_processed", "nb_skipped", "reads_no_errors", "reads_processed"):
            assert int(sst[key]) == int(ost[key]), (key, n_batches)
        assert ctx.diag_scan_replays() >= 1
        if record_stops:      # every batch's lists exactly once, whatever was scanned twice -- and the oracle's lists
            while True:
                t = ctx.take_stops()
                if t is None:
                    break
                taken.append(t)
            seen = [seq for seq, _ in taken]
            assert seen == list(range(n_batches))
            got = []
            for seq, st in taken:
                lists = [[] for _ in range(batches[seq].n_reads)]
                for e in st:
                    lists[int(e["read"])].append(int(e["ext"]))
                got.extend(lists)
            assert got == want, (n_batches, take_during)
        ctx.close()
    ctx = api.Context(k, tai, nh, junction_capacity=1 << 12, eager_flags=True)
    batch = chunks(bases, offs, 1)
    api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), batch)
    ctx.scan_begin()
    with pytest.raises(api.FaucetGpuError, match="junction table full"):
        ctx.scan_batch(batch[0])
        ctx.scan_end()
    try:
        ctx.scan_end()
    except api.FaucetGpuError:
        pass
    ctx.close()


@pytest.mark.parametrize("mode", ["shard_times", "shard_planes"])
@pytest.mark.parametrize("n_shards,batches_per_shard,ratio", [(2, 1, None), (3, 4, None), (4, 3, "0/1"), (3, 5, "1000000/1")])
def test_shard_fixup_protocol_is_exact(n_shards, batches_per_shard, ratio, mode, monkeypatch):
    """Multi-GPU pass 1 without the presence pass (fgpu_load_fixup), emulated with one context per shard on this device: every shard
    loads its reads alone -- with first-set times that count through the shard (FGPU_LOAD_SHARD_TIMES: shards below 2^32 positions), or writing
    down which bits of an occurrence were not set before it (FGPU_LOAD_SHARD_PLANES, round 5: any shard size) -- then re-evaluates what it kept
    out of bloo2 against the OR of the lower shards' bloo1.  The OR of the shards' bloo2 is the oracle's bloo2, the last shard's bloo1 the oracle's bloo1, the
    to_bloo2 counts add up, and the scan of every shard reuses the fixed-up planes (valid_reused == to_bloo2 of the shard)."""
    import torch
    if ratio:
        monkeypatch.setenv("FGPU_SWEEP_RATIO", ratio)
    k, tai, nh = 21, 1 << 18, 3
    bases, offs = _random_case(2400, 100, k, 9000, 0.02, 99, 0.003, 2)
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    olst = po.load_two_filters(b1, b2, bases, offs, k)
    n = len(offs) - 1
    cuts = np.linspace(0, n, n_shards + 1).astype(int)
    ctxs, shards, stats = [], [], []
    for a, z in zip(cuts[:-1], cuts[1:]):
        sub = np.linspace(a, z, batches_per_shard + 1).astype(int)
        shards.append([api.ReadBatch(bases, offs[x:y + 1].copy()) for x, y in zip(sub[:-1], sub[1:])])
        ctxs.append(api.Context(k, tai, nh))
    for ctx, sh in zip(ctxs, shards):
        ctx.load_begin(**{mode: True})
        for b in sh:
            ctx.load_batch(b)
        stats.append(ctx.load_end())
    local_b1 = [torch.from_numpy(ctx.bloom_download(L.BLOO1)).cuda() for ctx in ctxs]
    prefix = torch.zeros(tai // 8, dtype=torch.uint8, device="cuda")
    total = stats[0]["to_bloo2"]
    for r in range(1, n_shards):
        prefix |= local_b1[r - 1]
        torch.cuda.synchronize()
        st = ctxs[r].load_fixup(prefix.data_ptr())
        assert st["to_bloo2"] >= stats[r]["to_bloo2"]
        stats[r] = st
        total += st["to_bloo2"]
        with pytest.raises(api.FaucetGpuError):      # once per pass
            ctxs[r].load_fixup(prefix.data_ptr())
    assert total == olst.to_bloo2
    merged = np.zeros(tai // 8, dtype=np.uint8)
    for ctx in ctxs:
        merged |= ctx.bloom_download(L.BLOO2)
    assert np.array_equal(merged, b2.bits())
    assert np.array_equal(ctxs[-1].bloom_download(L.BLOO1), b1.bits())
    # every shard scans with the global filter; its validity answers come from the fixed-up planes
    for ctx, sh, st in zip(ctxs, shards, stats):
        ctx.bloom_upload(L.BLOO2, merged)                       # (an upload forgets the planes ...
    ctx = ctxs[-1]
    ctx.load_begin(**{mode: True})                              # ... so load the last shard again and fix it up: the planes are kept)
    for b in shards[-1]:
        ctx.load_batch(b)
    ctx.load_end()
    st = ctx.load_fixup(prefix.data_ptr())
    q, nbytes = ctx.bloom_devptr(L.BLOO2)
    m = torch.from_numpy(merged).cuda()
    torch.cuda.synchronize()
    ctx.bitmap_or(q, m.data_ptr(), nbytes)
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(shards[-1])
    assert sst["valid_reused"] == st["to_bloo2"]
    osc = po.Scanner(k, 1, 100, b2)
    for b in shards[-1]:
        osc.scan_reads(b.bases, b.offsets)
    _scan_equals_oracle(sc, sst, osc)


def test_load_fixup_refuses_passes_it_cannot_speak_for():
    k, tai, nh = 21, 1 << 16, 3
    bases, offs = _random_case(300, 100, k, 3000, 0.01, 5)
    import torch
    prefix = torch.zeros(tai // 8, dtype=torch.uint8, device="cuda")
    for kw, begin in (({}, {}), ({"keep_resident": False}, {"shard_times": True}), ({"mercy": True}, {"shard_times": True}),
                      ({}, {"shard_times": True, "keep_carry": True}), ({"keep_resident": False}, {"shard_planes": True}),
                      ({"mercy": True}, {"shard_planes": True}), ({}, {"shard_planes": True, "keep_carry": True})):
        ctx = api.Context(k, tai, nh, **kw)
        ctx.load_begin(**begin)
        ctx.load_batch(api.ReadBatch(bases, offs))
        ctx.load_end()
        with pytest.raises(api.FaucetGpuError, match="load_fixup needs"):
            ctx.load_fixup(prefix.data_ptr())
        ctx.close()


def test_a_fresher_preview_lets_the_walk_look_only_for_the_keys_created_since(monkeypatch):
    """fgpu_scan_import_hint a second time + fgpu_scan_refresh_prepared (round 5): shard C prepares against an early preview, is then shown the table
    shard B was HANDED (= A's final table) and makes its planes again against it, and when B's final table arrives its walk merges the keys B
    created into the planes through a filter of just those keys (fgpu_diag_prepared_refresh says so).  Records, creation order and counters are
    the oracle's -- also when the "fresher preview" is NOT an earlier state of the table that arrives (the count of newer entries does not fit:
    the planes are made again in full), when nothing was refreshed, and with the short cut switched off."""
    import torch
    monkeypatch.setenv("FGPU_DEBUG_DELTA_CHECK", "1")      # the merged planes are compared with planes made again in full, batch by batch
    k, G = 21, 30_000
    bases, offs = _random_case(15_000, 100, k, G, 0.012, 911, 0.002, 3)
    tai, nh = api.load_filter_shape(20 * G, 4 * G)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh)
    n = len(offs) - 1
    cut = [0, n // 3, 2 * n // 3, n]
    parts = [[api.ReadBatch(bases, offs[x:y + 1].copy()) for x, y in ((lo, (lo + hi) // 2), ((lo + hi) // 2, hi))] for lo, hi in zip(cut[:-1], cut[1:])]
    ctxs = [api.Context(k, tai, nh) for _ in range(3)]
    for ctx in ctxs:
        ctx.bloom_upload(L.BLOO2, b2.bits())

    def export(ctx):
        m = ctx.table_entries()
        buf = torch.empty(max(m, 1) * L.TABLE_ENTRY_BYTES, dtype=torch.uint8, device="cuda")
        assert ctx.export_table(buf.data_ptr(), buf.numel()) == m
        torch.cuda.synchronize()
        return m, buf

    a, b, c = ctxs
    a.scan_begin()
    a.scan_batch(parts[0][0])
    n_early, early = export(a)
    a.scan_batch(parts[0][1])
    st_a = a.scan_end()
    n_a, t_a = export(a)
    b.scan_begin()
    b.import_table(t_a.data_ptr(), n_a, carried=st_a)
    for p in parts[1]:
        b.scan_batch(p)
    st_b = b.scan_end()
    n_b, t_b = export(b)
    assert 0 < n_early < n_a < n_b
    okeys, orecs = osc.junctions("creation")
    ost = osc.stats()

    def run_c(late, refresh=True):
        c.scan_begin()
        c.import_hint(early.data_ptr(), n_early)
        for p in parts[2]:
            c.scan_prepare(p)
        if late is not None:
            c.import_hint(late[1].data_ptr(), late[0])
            if refresh:
                c.scan_refresh_prepared()
        c.import_table(t_b.data_ptr(), n_b, carried=st_b)
        c.scan_walk_prepared()
        st = c.scan_end()
        keys, recs = c.junctions()
        for key in ("n_junctions", "nb_jcheck_kmer", "nb_no_juncs", "nb_processed", "nb_skipped", "reads_no_errors"):
            assert st[key] == ost[key], key
        assert np.array_equal(keys, okeys) and np.array_equal(recs["dist"], orecs["dist"]) and np.array_equal(recs["cov"], orecs["cov"])
        return c.diag_prepared_refresh()

    d = run_c((n_a, t_a))
    assert d == {"batches_in_full": 0, "batches_merged": 2, "new_keys": n_b - n_a, "mismatching_words": 0}, d
    # round 6: the refresh also made the batches' candidate planes, and the walk linked every first window of a batch by them (the debug knob
    # above ran the full link pass behind each and compared the lk planes: "mismatching_words")
    sl = c.diag_sparse_link()
    assert sl["windows_sparse"] >= 2, sl
    d = run_c(None)                                         # no fresher preview: the planes speak of the early one, the surplus is A's rest + B's
    assert d["batches_merged"] == 2 and d["new_keys"] == n_b - n_early and d["mismatching_words"] == 0, d
    assert c.diag_sparse_link()["windows_sparse"] == 0      # (no refresh call, no candidate planes: every window linked in full)
    d = run_c((n_a, t_a), refresh=False)                    # shown but not refreshed: the planes do not speak of the newest preview
    assert d["batches_in_full"] == 2 and d["batches_merged"] == 0, d
    assert c.diag_sparse_link()["windows_sparse"] == 0
    monkeypatch.setenv("FGPU_NO_SPARSE_LINK", "1")          # the short cut off: same records
    d = run_c((n_a, t_a))
    assert d["batches_merged"] == 2 and d["mismatching_words"] == 0 and c.diag_sparse_link()["windows_sparse"] == 0, d
    monkeypatch.delenv("FGPU_NO_SPARSE_LINK")
    # a "preview" that is not an earlier state of the table that arrives: B's own final table with half of its entries dropped from the FRONT
    # (old entries missing, all the new ones there) -- as many entries as A's table, but the newer-than-the-preview count does not fit
    bogus = t_b[(n_b - n_a) * L.TABLE_ENTRY_BYTES:].clone()
    d = run_c((n_a, bogus))
    assert d["batches_in_full"] == 2 and d["batches_merged"] == 0, d
    # ... and one where the COUNT fits by coincidence -- A's table with one key exchanged for another, stamps as they were: as many
    # entries newer than the preview as the surplus, but the older entries are not the preview's keys (their digest differs)
    near = t_a.clone()
    near[8 * 0] ^= 1                                        # (the last base of the first entry's k-mer)
    d = run_c((n_a, near))
    assert d["batches_in_full"] == 2 and d["batches_merged"] == 0, d


def test_table_hint_lets_a_later_shard_prepare_lazily_and_never_enters_the_result():
    """fgpu_scan_import_hint: shard B prepares against the table shard A had after a third of its reads (a preview), is then handed A's
    final table and walks.  Records, order and counters are the oracle's; fewer junction tests were evaluated than without the hint;
    walking on the hint itself is refused."""
    import torch
    k, G = 21, 30_000
    bases, offs = _random_case(12_000, 100, k, G, 0.01, 4711, 0.002, 3)     # 40x
    tai, nh = api.load_filter_shape(20 * G, 4 * G)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh)
    n = len(offs) - 1
    half = n // 2
    part_a = [api.ReadBatch(bases, offs[x:y + 1].copy()) for x, y in ((0, half // 3), (half // 3, half))]
    part_b = [api.ReadBatch(bases, offs[x:y + 1].copy()) for x, y in ((half, half + half // 2), (half + half // 2, n))]
    a, b = api.Context(k, tai, nh), api.Context(k, tai, nh)
    for ctx in (a, b):
        ctx.bloom_upload(L.BLOO2, b2.bits())

    def export(ctx):
        m = ctx.table_entries()
        buf = torch.empty(max(m, 1) * L.TABLE_ENTRY_BYTES, dtype=torch.uint8, device="cuda")
        assert ctx.export_table(buf.data_ptr(), buf.numel()) == m
        torch.cuda.synchronize()
        return m, buf

    a.scan_begin()
    a.scan_batch(part_a[0])
    n_hint, hint = export(a)                                   # mid-scan: an earlier state of A's table
    a.scan_batch(part_a[1])
    st_a = a.scan_end()
    n_real, real = export(a)
    assert 0 < n_hint < n_real

    def run_b(with_hint):
        b.scan_begin()
        if with_hint:
            b.import_hint(hint.data_ptr(), n_hint)
        for p in part_b:
            b.scan_prepare(p)
        if with_hint:
            with pytest.raises(api.FaucetGpuError, match="preview"):
                b.scan_walk_prepared()
        b.import_table(real.data_ptr(), n_real, carried=st_a)
        b.scan_walk_prepared()
        st = b.scan_end()
        return st, b.junctions()

    st_plain, (k_plain, r_plain) = run_b(False)
    st_hint, (k_hint, r_hint) = run_b(True)
    assert st_hint["flag_positions"] < 0.8 * st_plain["flag_positions"]
    for st, keys, recs in ((st_plain, k_plain, r_plain), (st_hint, k_hint, r_hint)):
        ost = osc.stats()
        for key in ("n_junctions", "nb_jcheck_kmer", "nb_no_juncs", "nb_processed", "nb_skipped", "reads_no_errors"):
            assert st[key] == ost[key], key
        okeys, orecs = osc.junctions("creation")
        assert np.array_equal(keys, okeys) and np.array_equal(recs["dist"], orecs["dist"]) and np.array_equal(recs["cov"], orecs["cov"])
    # the hint may land between two prepares (the batches before it have seen an empty table) but not once a walk has been issued
    b.scan_begin()
    b.scan_prepare(part_b[0])
    b.import_hint(hint.data_ptr(), n_hint)
    b.scan_prepare(part_b[1])
    b.import_table(real.data_ptr(), n_real, carried=st_a)
    b.scan_walk_prepared()
    st_mid = b.scan_end()
    k_mid, r_mid = b.junctions()
    assert np.array_equal(k_mid, k_plain) and r_mid.tobytes() == r_plain.tobytes()
    assert st_hint["flag_positions"] <= st_mid["flag_positions"] <= st_plain["flag_positions"]
    b.scan_begin()
    b.scan_batch(part_b[0])
    with pytest.raises(api.FaucetGpuError, match="before any walk"):
        b.import_hint(hint.data_ptr(), n_hint)
    b.scan_end()


@pytest.mark.parametrize("table_mib,slice_mib,n_hash,fill", [(64, 4, 3, 0x29), (8, 1, 2, 0x5A), (64, 8, 2, 0x11), (512, 4, 4, 0x7B)])
def test_binned_probe_chains_answer_like_direct_ones(table_mib, slice_mib, n_hash, fill):
    """NS1 (north_star's query-side blocking) as built for measurement in csrc/diag.hip: Bloom::contains chains whose FIRST level is binned by filter
    slice and probed from the XCD that holds the slice, survivors handed back as a dense list, must give the answers of the direct chains bit
    for bit (the diagnostic had no correctness test)."""
    ctx = api.Context(31, 1 << 29, 3)
    r = ctx.diag_binned_chain(table_mib << 20, 1 << 24, slice_mib << 20, n_hash, fill, 1)
    assert r["equal"], r
    want = bin(fill).count("1") / 8
    assert abs(r["survivors_share"] - want) < 0.01, r      # the first level lets through exactly the items whose first bit is set
    ctx.close()


def test_key_ordered_walk_under_contention_is_repeatable(monkeypatch):
    """ADVICE r2 (the hand-over's release order): many waves on the turn counters of a few hot k-mers -- twenty copies of a 300-base repeat at
    high coverage, one large cluster per window -- walked in k-mer order from the first window on, five times over: every run must give the
    oracle's junction map record for record (a turn that moved before a record's store had landed would show as a lost coverage count or link)."""
    monkeypatch.setenv("FGPU_WALK_KO", "16")
    monkeypatch.setenv("FGPU_WALK_KO_ALWAYS", "1")
    g = synth.make_genome(300_000, 91, repeats=20, repeat_len=300)
    r = synth.make_reads(g, 120_000, 100, 0.01, 92)           # 40x: every wrong base of the repeat recurs often enough to be in bloo2
    bases, offs = po.reads_from_matrix(r)
    k, E, S = 31, 4_000_000, 1_000_000
    tai, nh = api.load_filter_shape(E, S)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    okeys, orecs = osc.junctions("creation")
    biggest = 0
    for rep in range(5):
        ctx = api.Context(k, tai, nh, walk_window_span=1 << (20 + rep % 3))
        api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, 3))
        sc = api.ReadScanner(ctx)
        sst = sc.scanReads(chunks(bases, offs, 2))
        keys, recs = sc.junctions()
        assert np.array_equal(keys, okeys), rep
        for f in ("dist", "cov", "linked"):
            assert np.array_equal(recs[f], orecs[f]), (rep, f)
        biggest = max(biggest, sst["walk_max_cluster"])
        assert sst["walk_parallel"] > 1000
        ctx.close()
    assert biggest >= 64


def test_device_batches_with_the_callers_total_equal_the_ones_without_and_a_wrong_total_is_refused():
    """fgpu_reads.total_bases (include/faucet_gpu.h): a device batch whose caller says how many bases it holds is packed without the
    read-back of two offsets; the results are the same three ways (host batches, device batches without and with the total), ragged reads and
    an offsets[0] that is not 0 included, and a total that does not match the offsets fails the pass instead of packing something else."""
    import torch
    bases, offs = _random_case(6000, 100, 21, 9000, 0.01, 77, n_rate=0.002, repeats=2)
    bases, offs = bases[37:], (offs - 37)[1:]                      # drop the first read's head: offsets[0] = 63
    k, (tai, nh) = 21, api.load_filter_shape(600_000, 150_000)
    b1, b2, lst, osc = oracle_run((bases[offs[0]:], offs - offs[0]), k, tai, nh, 1, 100)
    d_bases = torch.from_numpy(np.ascontiguousarray(bases)).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    cuts = [0, 1500, 1501, 4000, len(offs) - 1]

    def batches(with_total, lie=0):
        out = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            n_pos = int(offs[hi] - offs[lo]) + (hi - lo) + lie if with_total else None
            out.append(api.ReadBatch(d_bases.data_ptr(), d_offs[lo:].data_ptr(), n_reads=hi - lo, on_device=True, keepalive=(d_bases, d_offs), n_positions=n_pos))
        return out

    for with_total in (False, True):
        assert (batches(with_total)[0].c_struct().total_bases != 0) == with_total
        ctx = api.Context(k, tai, nh)
        st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), batches(with_total))
        assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits()) and st["to_bloo2"] == lst.to_bloo2
        sc = api.ReadScanner(ctx)
        sst = sc.scanReads(batches(with_total))
        _scan_equals_oracle(sc, sst, osc)
        ctx.close()
    for lie in (-1, 64):
        ctx = api.Context(k, tai, nh)
        with pytest.raises(api.FaucetGpuError, match="total_bases"):
            api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), batches(True, lie))
        ctx.close()
