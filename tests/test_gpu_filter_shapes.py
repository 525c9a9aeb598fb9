"""Filter shapes the rest of the suite never runs, against the oracle and the compiled reference: one hash function (S/E near 1), five to ten
(a small -fp), 2^31 bits (the one size whose load keeps its carry by re-hashing, k_carry_set) and -j 5..8.  Code that only these shapes reach:
the generic resolve kernel k_load_resolve (more than MISS_PLANES = 4 hash functions: bits past the planes are re-tested against the carry),
the early return of a one-function filter, the 4-bit hash index of k_scan_flags_sm, the 8-deep stacks of jcheck_dfs, the shard hosts'
choice of protocol by hash count, and first-set times that restart at 0 in every batch.  Every test asserts the hash count it reached."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api, synth
from oracle import pyoracle as po
from tests import golden_util
from tests.test_gpu_parity import _check_against_oracle, _oracle_lists, _random_case, _scan_equals_oracle, chunks, oracle_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "faucet_ref")
need_ref = pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/faucet_ref was not built (make -C oracle ref)")


def fp_for(E, S, nh):
    """an -fp at which the product's sizing from reads (fgpu_solve_p1 + fgpu_size_optimal) gives `nh` hash functions"""
    fp = golden_util.fp_for(E, S, nh, lambda e, s, f: api.load_filter_shape(e, s, f)[1])
    assert fp is not None, (E, S, nh)
    return fp


def shape(nh, E=1_000_000):
    """(tai, n_hash) as the product sizes a filter from reads for `nh` hash functions: S = 0.95 E at the default fp for one, S = E / 5 and a
    smaller fp for the others"""
    if nh == 1:
        tai, got = api.load_filter_shape(E, E * 95 // 100)
    else:
        tai, got = api.load_filter_shape(E, E // 5, fp_for(E, E // 5, nh))
    assert got == nh
    return tai, got


@functools.lru_cache(maxsize=None)
def _case(nh, mercy=False):
    """40x random reads of a 20 kb genome with planted repeats and N, and the oracle's filters and scan on them"""
    bases, offs = _random_case(8000, 100, 25, 20000, 0.012, 500 + nh, 0.002, 3)
    tai, nh = shape(nh)
    b1, b2, lst, osc = oracle_run((bases, offs), 25, tai, nh, 1, 100, mercy=mercy)
    return bases, offs, tai, nh, b1, b2, lst, osc


def _load_equals_oracle(ctx, st, b1, b2, lst):
    assert np.array_equal(ctx.bloom_download(L.BLOO1), b1.bits()), "bloo1 differs from the oracle"
    assert np.array_equal(ctx.bloom_download(L.BLOO2), b2.bits()), "bloo2 differs from the oracle"
    assert st["kmers"] == lst.kmers and st["to_bloo2"] == lst.to_bloo2 and st["unambiguous_reads"] == lst.unambiguous_reads


NH = [1, 3, 5, 6, 7, 10]      # 3: the shapes of the rest of the suite, as a control


@pytest.mark.parametrize("n_batches,ratio", [(1, None), (4, None), (4, "0/1"), (4, "1000000/1")], ids=["1", "4", "4-sweep-every", "4-sweep-never"])
@pytest.mark.parametrize("nh", NH, ids=lambda n: f"nh{n}")
def test_load_and_scan_equal_the_oracle(nh, n_batches, ratio, monkeypatch):
    """both filters bit for bit, kmers / to_bloo2, every scan counter, junction keys in creation order and their records -- with the carry
    brought up to date after every batch or never before load_end (FGPU_SWEEP_RATIO), so the generic resolve meets a lagging carry"""
    if ratio:
        monkeypatch.setenv("FGPU_SWEEP_RATIO", ratio)
    bases, offs, tai, nh_, b1, b2, lst, osc = _case(nh)
    assert nh_ == nh
    ctx = api.Context(25, tai, nh)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, n_batches))
    _load_equals_oracle(ctx, st, b1, b2, lst)
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, n_batches))
    assert sst["n_junctions"] > 100
    _scan_equals_oracle(sc, sst, osc)
    ctx.close()


@pytest.mark.parametrize("n_batches", [1, 4])
@pytest.mark.parametrize("nh", [1, 7], ids=lambda n: f"nh{n}")
def test_mercy_load_and_scan_equal_the_oracle(nh, n_batches):
    bases, offs, tai, nh_, b1, b2, lst, osc = _case(nh, mercy=True)
    assert nh_ == nh
    plain = _case(nh)[5]
    assert not np.array_equal(b2.bits(), plain.bits())          # --mercy does change bloo2 here
    ctx = api.Context(25, tai, nh, mercy=True)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, n_batches))
    _load_equals_oracle(ctx, st, b1, b2, lst)
    sc = api.ReadScanner(ctx)
    _scan_equals_oracle(sc, sc.scanReads(chunks(bases, offs, n_batches)), osc)
    ctx.close()


def _dense(bits, fill, seed):
    """the filter with random bits set on top until about `fill` of it is 1: a k-mer that is not in the data passes 4 of 7 bits often
    enough (fill^4) for a scan that tests fewer bits than it should to find junctions the oracle does not"""
    rng = np.random.default_rng(seed)
    have = np.unpackbits(bits).mean()
    p = max(0.0, (fill - have) / (1.0 - have))
    return bits | np.packbits(rng.random(bits.size * 8) < p)


@pytest.mark.parametrize("n_batches", [1, 4])
@pytest.mark.parametrize("nh", [3, 5, 7, 10], ids=lambda n: f"nh{n}")
def test_scan_on_a_dense_filter_equals_the_oracle(nh, n_batches):
    """the scan (flags kernels, walk, junction records) over a bloo2 about 35 % full -- the load's own filters are about 1 % full, where any
    four bits of a k-mer not in the data are all set with a chance of about 1e-8 and a hash count the scan cuts short goes unseen"""
    bases, offs, tai, nh_, _, b2, _, _ = _case(nh)
    assert nh_ == nh
    dense = _dense(b2.bits(), 0.35, 70 + nh)
    assert 0.3 < np.unpackbits(dense).mean() < 0.4
    ob = po.Bloom(tai, nh)
    ob.set_bits(dense)
    osc = po.Scanner(25, 1, 100, ob)
    osc.scan_reads(bases, offs)
    ctx = api.Context(25, tai, nh)
    ctx.bloom_upload(L.BLOO2, dense)
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, n_batches))
    _scan_equals_oracle(sc, sst, osc)
    ctx.close()


def test_stop_lists_and_both_pair_filters_at_seven_hash_functions():
    """scanInputRead's lists per read, the short pair filter (single ends with cleaning) and both pair filters of paired ends, on a bloo2 of
    seven hash functions"""
    k, E, S = 25, 1_000_000, 200_000
    tai, nh = shape(7, E)
    bases, offs = _random_case(12000, 110, k, 30000, 0.012, 99, 0.003, 3)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100)
    _, want = _oracle_lists(bases, offs, k, 1, 100, b2.bits(), tai, nh)
    _, stai, snh = api.size_optimal(E // 20, np.float32(0.01))       # src/Faucet.cpp:266-283
    _, ltai, lnh = api.size_optimal(E // 10, np.float32(0.01))
    ctx = api.Context(k, tai, nh, record_stops=True)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    ctx.scan_short_pairs(stai, snh, True)
    parts = chunks(bases, offs, 4)
    ctx.scan_begin()
    for part in parts:
        ctx.scan_batch(part)
    sst = ctx.scan_end()
    got = []
    while (t := ctx.take_stops()) is not None:
        seq, st = t
        lists = [[] for _ in range(parts[seq].n_reads)]
        for e in st:
            lists[int(e["read"])].append(int(e["ext"]))
        got.extend(lists)
    assert got == want
    _scan_equals_oracle(ctx, sst, osc)
    short = po.Bloom(stai, snh)
    osc2 = po.Scanner(k, 1, 100, b2, short_pf=short)
    osc2.scan_reads(bases, offs, paired_ends=False, no_cleaning=False)
    got = ctx.scan_short_pairs_download(stai)
    assert got.any() and np.array_equal(got, short.bits())
    ctx.close()
    # paired ends: the long filter is check-then-insert in file order
    short, long_ = po.Bloom(stai, snh), po.Bloom(ltai, lnh)
    osc3 = po.Scanner(k, 1, 100, b2, short_pf=short, long_pf=long_)
    osc3.scan_reads(bases, offs, paired_ends=True, no_cleaning=False)
    ost = osc3.stats()
    ctx = api.Context(k, tai, nh, record_stops=True)
    ctx.bloom_upload(L.BLOO2, b2.bits())
    ctx.scan_short_pairs(stai, snh, False)
    ctx.scan_long_pairs(ltai, lnh, 2)
    ctx.scan_begin()
    for part in chunks(bases, offs, 5):
        ctx.scan_batch(part)
    ctx.scan_end()
    bits, empty, not_empty = ctx.scan_long_pairs_download(ltai)
    assert (empty, not_empty) == (ost["empty_count"], ost["not_empty_count"])
    assert bits.any() and np.array_equal(bits, long_.bits())
    assert np.array_equal(ctx.scan_short_pairs_download(stai), short.bits())
    ctx.close()


def test_walk_evaluates_the_junction_tests_the_preview_left_out_at_one_and_seven_hash_functions():
    """FGPU_DEBUG_NEED_DROP=1 (read once per process: child pytest) throws away about half of the flags kernel's false junction tests, so the
    walk runs testForJunction itself (fgpu_flags.h) on filters of one and seven hash functions; the results must still be the oracle's"""
    env = dict(os.environ, FGPU_DEBUG_NEED_DROP="1")
    sel = "test_load_and_scan_equal_the_oracle and (nh1- or nh7-) or test_scan_on_a_dense_filter or test_deep_jcheck"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", sel],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert "19 passed" in r.stdout, r.stdout[-500:]


def _segments(rng, k, n, max_extra):
    """random sequences of k .. k + max_extra bases: their k-mers lie at every distance from a dead end"""
    return [synth._ACGT[rng.integers(0, 4, size=k + int(rng.integers(0, max_extra + 1)))].tobytes() for _ in range(n)]


@pytest.mark.parametrize("nh", range(1, 11), ids=lambda n: f"nh{n}")
def test_device_probes_equal_the_reference_functions(nh):
    """fgpu_probe_contains and Stage 3's batched probes (JChecker::jcheck, getValidJExtension, isBloomJunction) against the oracle's
    restatement of the reference's functions, on a filter of the k-mers of short sequences (dead ends at every depth up to 12) and noise"""
    k, tai = 21, 1 << 20
    rng = np.random.default_rng(40 + nh)
    segs = _segments(rng, k, 3000, 12)
    b = po.Bloom(tai, nh)
    kmers = []
    for s in segs:
        for i in range(len(s) - k + 1):
            x = po.lib().fo_encode(s[i:i + k], k)
            kmers.append(x)
            b.add(po.lib().fo_canon(x, k))
    for x in rng.integers(0, 1 << (2 * k), size=20000 // nh, dtype=np.uint64):
        b.add(po.lib().fo_canon(int(x), k))
    probes = np.array(kmers[::3] + [int(x) for x in rng.integers(0, 1 << (2 * k), size=500, dtype=np.uint64)], dtype=np.uint64)
    canon = np.array([po.lib().fo_canon(int(x), k) for x in probes], dtype=np.uint64)
    want_in = [b.contains(int(c)) for c in canon]
    assert any(want_in) and not all(want_in)
    for j in (0, 1, 3, 5, 8):
        ctx = api.Context(k, tai, nh, j=j)
        assert ctx.n_hash == nh
        ctx.bloom_upload(L.BLOO2, b.bits())
        assert list(ctx.probe_contains(L.BLOO2, canon)) == want_in
        want = [po.lib().fo_stage3_jcheck(b.h, int(x), k, j) for x in probes]
        assert list(ctx.probe_jcheck(probes)) == want, j
        if j >= 5:          # the clear answers, both ways: some k-mers of the filter fail only at depth > 4
            assert 0 < sum(want) < len(want)
        assert list(ctx.probe_valid_extension(probes)) == [po.lib().fo_stage3_valid_extension(b.h, int(x), k, j) for x in probes], j
        assert list(ctx.probe_bloom_junction(probes)) == [po.lib().fo_stage3_bloom_junction(b.h, int(x), k, j) for x in probes], j
        ctx.close()


def _shards_of(bases, offs, n_shards, batches_per_shard):
    n = len(offs) - 1
    cuts = np.linspace(0, n, n_shards + 1).astype(int)
    out = []
    for a, z in zip(cuts[:-1], cuts[1:]):
        sub = np.linspace(a, z, batches_per_shard + 1).astype(int)
        out.append([api.ReadBatch(bases, offs[x:y + 1].copy()) for x, y in zip(sub[:-1], sub[1:])])
    return out


def _fixup_run(k, tai, nh, shards, mode="shard_times"):
    """test_shard_fixup_protocol_is_exact's scheme: every shard loads alone, then re-evaluates what it kept out of bloo2 against the OR of the
    lower shards' bloo1.  Returns (contexts, the OR of their bloo2, the sum of to_bloo2, the last prefix)."""
    import torch
    ctxs, stats = [], []
    for sh in shards:
        ctx = api.Context(k, tai, nh)
        ctx.load_begin(**{mode: True})
        for b in sh:
            ctx.load_batch(b)
        stats.append(ctx.load_end())
        ctxs.append(ctx)
    prefix = torch.zeros(tai // 8, dtype=torch.uint8, device="cuda")
    total = stats[0]["to_bloo2"]
    for r in range(1, len(shards)):
        prefix |= torch.from_numpy(ctxs[r - 1].bloom_download(L.BLOO1)).cuda()
        torch.cuda.synchronize()
        st = ctxs[r].load_fixup(prefix.data_ptr())
        assert st["to_bloo2"] >= stats[r]["to_bloo2"]
        total += st["to_bloo2"]
    merged = np.zeros(tai // 8, dtype=np.uint8)
    for ctx in ctxs:
        merged |= ctx.bloom_download(L.BLOO2)
    return ctxs, merged, total, prefix


@pytest.mark.parametrize("n_shards,batches_per_shard", [(2, 1), (3, 4)])
@pytest.mark.parametrize("nh", [1, 7], ids=lambda n: f"nh{n}")
def test_shard_fixup_on_one_clock(nh, n_shards, batches_per_shard):
    """the fix-up protocol's own pass on one clock through the shard (FGPU_LOAD_SHARD_TIMES), which has no limit on hash functions: the OR
    of the shards' bloo2 is the oracle's, the last shard's bloo1 too, the to_bloo2 counts add up, and the last shard's scan is the oracle's"""
    k = 21
    tai, nh_ = shape(nh, 300_000)
    assert nh_ == nh
    bases, offs = _random_case(2400, 100, k, 9000, 0.02, 99 + nh, 0.003, 2)
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    olst = po.load_two_filters(b1, b2, bases, offs, k)
    shards = _shards_of(bases, offs, n_shards, batches_per_shard)
    ctxs, merged, total, prefix = _fixup_run(k, tai, nh, shards)
    assert total == olst.to_bloo2
    assert np.array_equal(merged, b2.bits())
    assert np.array_equal(ctxs[-1].bloom_download(L.BLOO1), b1.bits())
    ctx = ctxs[-1]
    ctx.bloom_upload(L.BLOO2, merged)
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(shards[-1])
    osc = po.Scanner(k, 1, 100, b2)
    for b in shards[-1]:
        osc.scan_reads(b.bases, b.offsets)
    _scan_equals_oracle(sc, sst, osc)
    for c in ctxs:
        c.close()


def test_shard_planes_past_four_hash_functions_are_a_plain_load_and_the_python_host_takes_one_clock(monkeypatch):
    """fail planes exist for four hash functions: a FGPU_LOAD_SHARD_PLANES pass at seven is a plain load and fgpu_load_fixup answers STATE;
    the Python host (sharded.GpuShard) with FAUCET_SHARD_PLANES=1 must therefore stay on one clock, and its fix-up run gives the oracle's filters"""
    import torch
    from faucet_amd import sharded
    k = 21
    tai, nh = shape(7, 300_000)
    bases, offs = _random_case(2400, 100, k, 9000, 0.02, 199, 0.003, 2)
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    olst = po.load_two_filters(b1, b2, bases, offs, k)
    shards = _shards_of(bases, offs, 3, 2)
    planes, plain = api.Context(k, tai, nh), api.Context(k, tai, nh)
    planes.load_begin(shard_planes=True)
    plain.load_begin()
    for b in shards[1]:
        planes.load_batch(b)
        plain.load_batch(b)
    planes.load_end()
    plain.load_end()
    for which in (L.BLOO1, L.BLOO2):
        assert np.array_equal(planes.bloom_download(which), plain.bloom_download(which))
    prefix = torch.from_numpy(plain.bloom_download(L.BLOO1)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(api.FaucetGpuError):
        planes.load_fixup(prefix.data_ptr())
    planes.close()
    plain.close()

    monkeypatch.setenv("FAUCET_SHARD_PLANES", "1")
    dev = torch.device("cuda", 0)
    probe = sharded.GpuShard(api.Context(k, tai, nh), dev)
    assert probe._one_clock(shards[0]) and probe.fixup_possible(shards[0])
    probe.close()
    lst, sst, last = sharded.run_in_turn(lambda: sharded.GpuShard(api.Context(k, tai, nh), dev), shards, "fixup")
    assert sum(s["to_bloo2"] for s in lst) == olst.to_bloo2
    assert np.array_equal(last.ctx.bloom_download(L.BLOO2), b2.bits())
    osc = po.Scanner(k, 1, 100, b2)
    osc.scan_reads(bases, offs)
    _scan_equals_oracle(last.ctx, sst, osc)
    last.close()


@functools.lru_cache(maxsize=None)
def _case_2g(nh, mercy):
    k, tai = 31, 1 << 31
    bases, offs = _random_case(30000, 100, k, 60000, 0.01, 2031 + nh, 0.001, 3)
    b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, 1, 100, mercy=mercy)
    return k, tai, bases, offs, b1, b2, lst, osc


@pytest.mark.parametrize("nh,mercy", [(3, False), (7, True)])
def test_filters_of_two_to_the_31_bits(nh, mercy):
    """2^31 bits, the one size at which the load keeps its carry by re-hashing every batch's new k-mers (k_carry_set) and restarts its
    first-set times at 0 in every batch (--mercy reads them against tb = 0): five batches against the oracle, set bits in the top quarter"""
    k, tai, bases, offs, b1, b2, lst, osc = _case_2g(nh, mercy)
    set_bits = np.flatnonzero(b2.bits())
    assert set_bits.size and set_bits.max() >= (tai // 8) * 3 // 4
    ctx = api.Context(k, tai, nh, mercy=mercy)
    st = api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), chunks(bases, offs, 5))
    _load_equals_oracle(ctx, st, b1, b2, lst)
    sc = api.ReadScanner(ctx)
    sst = sc.scanReads(chunks(bases, offs, 3))
    _scan_equals_oracle(sc, sst, osc)
    ctx.close()


def test_shard_fixup_at_two_to_the_31_bits():
    """two shards on one clock each at 2^31 bits: the clock runs through the whole shard while the carry is kept by re-hashing"""
    k, tai, bases, offs, b1, b2, lst, osc = _case_2g(3, False)
    ctxs, merged, total, _ = _fixup_run(k, tai, 3, _shards_of(bases, offs, 2, 3))
    assert total == lst.to_bloo2
    assert np.array_equal(merged, b2.bits())
    assert np.array_equal(ctxs[-1].bloom_download(L.BLOO1), b1.bits())
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("j", [5, 6, 8])
def test_deep_jcheck(j):
    """-j 5..8 on a sparse filter of three hash functions: the generic flags kernel and jcheck_dfs' 8-deep stacks"""
    tai, nh = api.load_filter_shape(800_000, 200_000)
    assert nh == 3
    bases, offs = _random_case(10000, 120, 23, 15000, 0.02, 80 + j, 0.001, 6)
    sst = _check_against_oracle(bases, offs, 23, 800_000, 200_000, j)
    assert sst["n_junctions"] > 100


# ---- the command line against the compiled reference ----------------------------------------------------------------------------------

def _reads(tmp_path, paired, fastq, seed, n=1200):
    from tests.test_oracle_vs_reference_fuzz import _write
    g = synth.make_genome(6000, seed, repeats=3, repeat_len=90)
    r = synth.make_pairs(g, n // 2, 100, 250, 20, 0.01, seed + 1) if paired else synth.make_reads(g, n, 100, 0.01, seed + 1)
    path = str(tmp_path / ("in.fq" if fastq else "in.fa"))
    _write(path, [bytes(x) for x in np.ascontiguousarray(r)], fastq)
    return path


def _hash_lines(stdout):
    return [ln.split(":")[1].strip() for ln in stdout.splitlines() if ln.startswith("Number of hash functions:")]


def _args(E, S, fp=None, paired=False, fastq=False, cleaning=False, extra=()):
    a = ["-size_kmer", "21", "-max_read_length", "100", "-estimated_kmers", str(E), "-singletons", str(S)]
    a += ["-fp", str(fp)] if fp is not None else []
    a += ["--fastq"] if fastq else []
    a += ["--paired_ends"] if paired else []
    a += [] if cleaning else ["--no_cleaning"]
    return a + list(extra)


@need_ref
@pytest.mark.parametrize("nh,paired,cleaning", [(1, False, True), (6, True, True), (7, False, True), (9, False, False), (7, True, False)])
def test_cli_from_reads_equals_the_compiled_reference(nh, paired, cleaning, tmp_path):
    from tests.test_gpu_vs_reference_fuzz import cli_against_reference
    E = 200_000
    S = E * 95 // 100 if nh == 1 else E // 5
    fp = None if nh == 1 else fp_for(E, S, nh)
    assert api.load_filter_shape(E, S, 0.04 if fp is None else fp)[1] == nh
    path = _reads(tmp_path, paired, paired, 60 + nh)
    ref_out, gpu_out = cli_against_reference(path, _args(E, S, fp, paired, paired, cleaning), tmp_path)
    assert _hash_lines(ref_out)[:1] == _hash_lines(gpu_out)[:1] == [str(nh)]


@need_ref
def test_cli_restart_from_a_bloom_file_with_six_hash_functions(tmp_path):
    """-bloom_file sizes the restarted filter from -fp alone (create_bloom_filter_optimal(E, fp)): 0.01, the value the reference's usage
    prints, gives six hash functions"""
    from tests.test_gpu_vs_reference_fuzz import cli_against_reference
    E, S = 200_000, 40_000
    assert api.size_optimal(E, np.float32(0.01))[2] == 6
    path = _reads(tmp_path, False, False, 71)
    d = tmp_path / "load"
    d.mkdir()
    r = subprocess.run([REF_BIN, "-read_load_file", path, "-read_scan_file", path, "-file_prefix", str(d / "out"), "--just_load_bloom"] +
                       _args(E, S), capture_output=True, text=True, timeout=600)
    assert os.path.getsize(d / "out.bloom") > 0, r.stderr[-2000:]
    ref_out, gpu_out = cli_against_reference(path, _args(E, S, 0.01, extra=["-bloom_file", str(d / "out.bloom")]), tmp_path, writes=(".junctions",))
    assert _hash_lines(ref_out) == _hash_lines(gpu_out) and set(_hash_lines(gpu_out)) == {"6"}


@need_ref
def test_cli_with_j_8_equals_the_compiled_reference(tmp_path):
    """-j 8 on a sparse three-function filter: no jcheck level comes near the reference's 1000 k-mers (utils/JChecker.cpp)"""
    from tests.test_gpu_vs_reference_fuzz import cli_against_reference
    E, S = 600_000, 120_000
    assert api.load_filter_shape(E, S)[1] == 3
    path = _reads(tmp_path, False, True, 81)
    ref_out, gpu_out = cli_against_reference(path, _args(E, S, fastq=True, cleaning=True, extra=["-j", "8"]), tmp_path)
    assert _hash_lines(ref_out)[:1] == _hash_lines(gpu_out)[:1] == ["3"]


@need_ref
@pytest.mark.parametrize("gpus", [2, 3])
@pytest.mark.parametrize("how", ["auto", "planes", "presence"])
def test_cli_over_read_shards_at_seven_hash_functions(gpus, how, tmp_path):
    """-gpus N at seven hash functions: the default fix-up protocol on one clock, FAUCET_SHARD_PLANES=1 (planes cover four functions: one
    clock all the same) and the presence protocol -- the reference's files and log every time"""
    from tests.test_gpu_vs_reference_fuzz import cli_against_reference
    E, S = 200_000, 40_000
    fp = fp_for(E, S, 7)
    path = _reads(tmp_path, True, True, 90 + gpus)
    env = {"FGPU_CLI_TIMES": "1"}
    env.update({"planes": {"FAUCET_SHARD_PLANES": "1"}, "presence": {"FAUCET_SHARD_PROTOCOL": "presence"}}.get(how, {}))
    ref_out, gpu_out = cli_against_reference(path, _args(E, S, fp, True, True, True), tmp_path, ["-gpus", str(gpus)], env)
    assert _hash_lines(ref_out)[:1] == _hash_lines(gpu_out)[:1] == ["7"]


def test_cli_refuses_the_fixup_protocol_with_mercy(tmp_path):
    E, S = 200_000, 40_000
    path = _reads(tmp_path, False, False, 95)
    exe = os.path.join(ROOT, "faucet_amd", "faucet")
    r = subprocess.run([exe, "-read_load_file", path, "-read_scan_file", path, "-file_prefix", str(tmp_path / "out"), "-gpus", "2", "--mercy"] +
                       _args(E, S, fp_for(E, S, 7)), capture_output=True, text=True, timeout=600, env=dict(os.environ, FAUCET_SHARD_PROTOCOL="fixup"))
    assert r.returncode != 0 and "FAUCET_SHARD_PROTOCOL=fixup" in r.stderr, r.stderr[-2000:]


@need_ref
@pytest.mark.parametrize("E", [200_000, pytest.param(300_000_000, marks=pytest.mark.slow)])
def test_cli_at_two_to_the_31_bits(E, tmp_path):
    """-estimated_kmers 3e8 at S = E / 5 sizes both filters at 2^31 bits (carry by re-hashing); 2e5 is its small sibling"""
    from tests.test_gpu_vs_reference_fuzz import cli_against_reference
    tai, nh = api.load_filter_shape(E, E // 5)
    assert nh == 3 and (tai == 1 << 31) == (E > 1e8)
    path = _reads(tmp_path, False, False, 97, n=4000)
    ref_out, gpu_out = cli_against_reference(path, _args(E, E // 5, cleaning=True), tmp_path, ["-batch_reads", "700"])
    assert _hash_lines(ref_out)[:1] == _hash_lines(gpu_out)[:1] == ["3"]


@need_ref
def test_cli_load_pass_with_256_byte_records_at_seven_hash_functions(tmp_path):
    """FGPU_LOAD_LAYOUT=records (the other filter layout of the load) with the generic resolve kernel"""
    from tests.test_gpu_vs_reference_fuzz import cli_against_reference
    E, S = 200_000, 40_000
    path = _reads(tmp_path, True, False, 99)
    ref_out, gpu_out = cli_against_reference(path, _args(E, S, fp_for(E, S, 7), True, False, True), tmp_path, ["-batch_reads", "97"],
                                             env={"FGPU_LOAD_LAYOUT": "records"})
    assert _hash_lines(ref_out)[:1] == _hash_lines(gpu_out)[:1] == ["7"]


@need_ref
@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "faucet_ref_gpu")), reason="oracle/_ref/faucet_ref_gpu was not built")
def test_linked_binding_at_seven_hash_functions_ends_like_the_pure_reference(tmp_path):
    """Stage 3's device walks and the reference's contig graph on a filter of seven hash functions"""
    from tests.test_gpu_vs_reference_fuzz import binding_differences
    from tests.test_oracle_vs_reference_fuzz import random_run
    seed = 7000
    _, _, args = random_run(seed, tmp_path)
    E, S = int(args[args.index("-estimated_kmers") + 1]), int(args[args.index("-singletons") + 1])
    fp = fp_for(E, S, 7)
    outs = {}
    notes, _ = binding_differences(seed, tmp_path, ["-fp", str(fp)], outs)
    assert notes == []
    assert _hash_lines(outs["ref"])[:1] == _hash_lines(outs["bound"])[:1] == ["7"]
