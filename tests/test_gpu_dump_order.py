"""fgpu_scan_dump_order (k_dump_first, k_dump_key and one rocPRIM radix sort per stretch between rehashes, faucet_amd/csrc/scan_table.hip)
against an independent reference: the container's node list replayed link by link (tests/dump_order_ref.py, pinned to a real
std::unordered_map by tests/test_dump_order_ref_cpu.py).  Every comparison is exact equality of the uint32 orders.

The keys are the test's own: a hand-made table (FGPU_TABLE_ENTRY_BYTES per entry: key, creation stamp, 16 record bytes) goes in through
fgpu_scan_import_table in a shuffled order and must come back from the creation-ordered download in stamp order with its records intact --
which also covers k_import, the table's growth in fgpu_scan_reserve and the download for tables no scan has made.  The command line hides
a wrong device order behind its host replay (faucet_main.cpp); the last two tests make it say which of the two wrote the file.
Needs an MI355X."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api, synth
from oracle import pyoracle as po
from tests import dump_order_ref as ref
from tests.golden_util import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "faucet_amd", "faucet")
# ExportEntry (faucet_amd/csrc/walk_tables.h): the record bytes are dist[5] cov[4] linked (bit c = link c) and six bytes of padding
ENTRY = np.dtype([("key", "<u8"), ("stamp", "<u8"), ("dist", np.uint8, 5), ("cov", np.uint8, 4), ("linked", np.uint8), ("pad", np.uint8, 6)])
assert ENTRY.itemsize == L.TABLE_ENTRY_BYTES


def small_table_context(k):
    """2^10 slots: fgpu_scan_reserve keeps the table below a quarter full, so an import of more than 256 entries grows it first"""
    return api.Context(k, 1 << 19, 3, junction_capacity=1 << 10)


def random_keys(n, seed, bits=62):
    """n distinct oriented k-mers below 2^bits in a random order (k odd: a k-mer and its reverse complement are two legal keys)"""
    rng = np.random.default_rng(seed)
    keys = np.unique(rng.integers(0, 1 << bits, size=n + 64, dtype=np.uint64))
    assert len(keys) >= n
    return rng.permutation(keys)[:n]


def hand_made_table(keys, seed):
    """(entries in creation order, the same entries shuffled): distinct creation stamps that ascend with the index and are never 0 (k_import
    and k_export give no stamp a meaning; the walk's own are piece << 20 | half-step, and piece 0, half-step 0 is one of them), random records"""
    rng = np.random.default_rng(seed)
    n = len(keys)
    e = np.zeros(n, dtype=ENTRY)
    e["key"] = keys
    stamps = np.unique(rng.integers(1, 1 << 60, size=n + 64, dtype=np.uint64))[:n]
    assert len(stamps) == n
    e["stamp"] = stamps
    e["dist"] = rng.integers(0, 256, size=(n, 5))
    e["cov"] = rng.integers(0, 256, size=(n, 4))
    e["linked"] = rng.integers(0, 32, size=n)
    return e, e[rng.permutation(n)]


def import_keys(ctx, keys, seed=0):
    """a scan of its own that only imports the hand-made table; the precondition of every test here: the download gives the keys in
    ascending stamp order and the records unchanged"""
    import torch
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    assert len(np.unique(keys)) == n > 0 and int(keys.max()) < 1 << (2 * ctx.k)
    created, shuffled = hand_made_table(keys, seed)
    dev = torch.from_numpy(shuffled.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    ctx.scan_begin()
    ctx.import_table(dev.data_ptr(), n)
    st = ctx.scan_end()
    assert st["n_junctions"] == n
    got_keys, got_recs = ctx.junctions()
    assert np.array_equal(got_keys, created["key"])
    assert np.array_equal(got_recs["dist"], created["dist"]) and np.array_equal(got_recs["cov"], created["cov"])
    assert np.array_equal(got_recs["linked"], (created["linked"][:, None] >> np.arange(5, dtype=np.uint8)[None, :]) & 1)
    return got_keys


def assert_order(ctx, keys, counts, buckets, n=None):
    m = len(keys) if n is None else n
    got = ctx.scan_dump_order(counts, buckets, n)
    assert got.dtype == np.uint32 and got.shape == (m,)
    want = ref.replay(keys, counts, buckets, m)
    assert np.array_equal(got, want), (m, list(counts), list(buckets), np.flatnonzero(got != want)[:5])


@pytest.fixture(scope="module")
def ctx31():
    ctx = small_table_context(31)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ctx5():
    ctx = small_table_context(5)
    yield ctx
    ctx.close()


# ---- a. sizes, the library's own schedule -----------------------------------------------------------------------------------------------
# around the first rehashes (13, 29), around one thread block (256) and sixteen (4096), past the command line's 50 000-key prefix (70 001),
# and one size past the rehash at 172 933, past the kernels' grid stride and past rocPRIM's single-block and small-size sorts (180 000)
@pytest.mark.parametrize("n", [1, 2, 13, 14, 29, 30, 255, 256, 257, 4095, 4096, 4097, 70001, 180000])
def test_sizes_with_the_librarys_schedule(n, ctx31):
    keys = import_keys(ctx31, random_keys(n, 1000 + n), seed=n)
    assert_order(ctx31, keys, *ref.libstdcxx_schedule(n))


# ---- b. key families ---------------------------------------------------------------------------------------------------------------------
def _family(name):
    """(k, keys)"""
    rng = np.random.default_rng(5)
    i = np.arange(1 << 15, dtype=np.uint64)
    if name in ref.crowded_k5_sets():                      # k = 5: every key below 1024, crowded whatever the bucket count
        return 5, ref.crowded_k5_sets()[name]
    if name == "one_bucket":                               # B * i + r for the last bucket count (1109 from 541 keys on): one bucket holds every node
        return 31, rng.permutation(np.uint64(1109) * i[:1000] + np.uint64(7))
    if name == "one_per_bucket":                           # 0 .. n-1 and more buckets than keys in the end
        return 31, i[:1000].copy()
    if name == "two_buckets":
        return 31, rng.permutation(np.concatenate([np.uint64(1109) * i[:500] + np.uint64(3), np.uint64(1109) * i[:500] + np.uint64(1000)]))
    if name == "one_bucket_20000":                         # (20753 buckets from 10273 keys on)
        return 31, rng.permutation(np.uint64(20753) * i[:20000] + np.uint64(5))
    if name == "two_buckets_20000":
        return 31, rng.permutation(np.concatenate([np.uint64(20753) * i[:10000], np.uint64(20753) * i[:10000] + np.uint64(20752)]))
    raise KeyError(name)


@pytest.mark.parametrize("name", sorted(ref.crowded_k5_sets()) + ["one_bucket", "one_per_bucket", "two_buckets", "one_bucket_20000", "two_buckets_20000"])
def test_key_families(name, ctx31, ctx5):
    k, keys = _family(name)
    ctx = ctx5 if k == 5 else ctx31
    keys = import_keys(ctx, keys, seed=len(keys))
    counts, buckets = ref.libstdcxx_schedule(len(keys))
    if name.startswith(("one_bucket", "two_buckets")):     # what the family's name says, of the last stretch
        assert len(np.unique(keys % np.uint64(buckets[-1]))) == int(name[:3] == "two") + 1
    if name == "one_per_bucket":
        assert buckets[-1] > len(keys)
    assert_order(ctx, keys, counts, buckets)


# ---- c. artificial schedules on one key set (sound input: the replay equals the closed form on such schedules, test_dump_order_ref_cpu.py) ---
@pytest.fixture(scope="module")
def fixed_3000():
    ctx = small_table_context(31)
    keys = import_keys(ctx, random_keys(3000, 31), seed=3)
    yield ctx, keys
    ctx.close()


SCHEDULES = {
    "one_stretch_B1": ([0], [1]),
    "one_stretch_B2": ([0], [2]),
    "one_stretch_B3": ([0], [3]),
    "one_stretch_B_4294967295": ([0], [(1 << 32) - 1]),        # the largest bucket count there is: 16 GiB of first-position words
    "one_stretch_largest_prime_below_2p28": ([0], [268435399]),
    "two_rehashes_at_one_count": ([0, 1000, 1000], [13, 101, 57]),
    "three_rehashes_at_one_count": ([0, 0, 1500, 1500, 1500], [1, 13, 541, 29, 1109]),
    "rehash_at_count_n": ([0, 1500, 3000], [13, 541, 1109]),
    "rehashes_at_count_n_twice": ([0, 3000, 3000], [7, 5087, 3]),
    "shrinking_buckets": ([0, 1000, 2000], [5087, 541, 13]),
    "first_real_rehash_at_count_0": ([0, 0, 100], [1, 13, 29]),
    "every_node_its_own_stretch_at_first": ([0, 1, 2, 3, 4, 5, 2999], [2, 3, 2, 5, 1, 4, 6]),
}


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_artificial_schedules(name, fixed_3000):
    ctx, keys = fixed_3000
    assert_order(ctx, keys, *SCHEDULES[name])


# ---- d. prefixes and reuse -----------------------------------------------------------------------------------------------------------------
def test_prefixes_schedules_back_to_back_and_a_second_import_on_one_context():
    ctx = small_table_context(31)
    keys = import_keys(ctx, random_keys(4097, 4), seed=4)
    sizes = [1, 13, 14, 4096, 4097]
    for n in sizes + sizes[::-1]:                                   # every answer speaks of the first n keys only
        assert_order(ctx, keys, *ref.libstdcxx_schedule(n), n=n)
    # two schedules back to back: the first positions and both lists are made again by every call (many buckets, then few; long list, then short)
    assert_order(ctx, keys, [0], [1000003])
    assert_order(ctx, keys, [0, 2000], [7, 5])
    assert_order(ctx, keys, [0, 50], [3, 1000003], n=100)
    assert_order(ctx, keys, *ref.libstdcxx_schedule(4097))
    # other keys, fewer of them, in a new scan on the same context
    other = import_keys(ctx, random_keys(1000, 44), seed=44)
    assert not np.intersect1d(other, keys).size
    assert_order(ctx, other, *ref.libstdcxx_schedule(1000))
    with pytest.raises(api.FaucetGpuError, match=f"error {L.ERR_STATE}:"):
        ctx.scan_dump_order(*ref.libstdcxx_schedule(4097), n=4097)  # the keys of the LAST download, at most that many
    assert_order(ctx, other, *ref.libstdcxx_schedule(1000))
    ctx.close()


# ---- e. keys of real scans -----------------------------------------------------------------------------------------------------------------
def test_a_goldens_scan_is_dumped_in_the_reference_files_order():
    c = Case("pe_repeats_k25")
    bases, offs = po.reads_from_lines(c.lines())
    tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
    ctx = api.Context(c.k, tai, nh, j=c.j, max_spacer_dist=c.spacer)
    ctx.bloom_upload(L.BLOO2, c.bloom())
    sc = api.ReadScanner(ctx)
    sc.scanReads([api.ReadBatch(bases, offs)])
    keys, recs = sc.junctions()
    assert len(keys) == c.counters["distinct_junctions"] == 377
    counts, buckets = ref.libstdcxx_schedule(len(keys))
    assert_order(ctx, keys, counts, buckets)
    order = ctx.scan_dump_order(counts, buckets)
    assert api.junction_lines(keys[order], recs[order], c.k) == c.junction_lines()      # (the reference's own file: its container's order)
    ctx.close()


def test_a_generated_inputs_scan():
    """30 000 reads of 100 bases with 2 % errors over a 60 000-base genome: 3203 junctions (the oracle's count)"""
    k = 31
    bases, offs = po.reads_from_matrix(synth.make_reads(synth.make_genome(60000, 4321), 30000, 100, 0.02, 4322))
    tai, nh = api.load_filter_shape(4_000_000, 2_000_000)
    ctx = api.Context(k, tai, nh)
    batch = api.ReadBatch(bases, offs)
    api.load_two_filters(api.Bloom(ctx, L.BLOO1), api.Bloom(ctx, L.BLOO2), [batch])
    sc = api.ReadScanner(ctx)
    sc.scanReads([batch])
    keys, _ = sc.junctions()
    assert len(keys) > 3000
    assert_order(ctx, keys, *ref.libstdcxx_schedule(len(keys)))
    assert_order(ctx, keys, *ref.libstdcxx_schedule(1500), n=1500)
    ctx.close()


# ---- f. refusals: each leaves the context usable ----------------------------------------------------------------------------------------------
def _call(ctx, counts, buckets, n, n_rehashes=None, null=()):
    """the C entry point itself: (status, order)"""
    c = (C.c_uint64 * max(len(counts), 1))(*counts)
    b = (C.c_uint64 * max(len(buckets), 1))(*buckets)
    out = (C.c_uint32 * max(n, 1))()
    rc = ctx.lib.fgpu_scan_dump_order(ctx.h, None if "counts" in null else c, None if "buckets" in null else b,
                                      len(counts) if n_rehashes is None else n_rehashes, n, None if "order" in null else out)
    return rc, np.frombuffer(out, dtype=np.uint32)[:n].copy()


def test_refusals_leave_the_context_usable():
    """No kernel runs on a schedule that is refused: fgpu_scan_dump_order_impl checks the whole schedule on the host before it allocates, sets or
    launches anything (read there, not tried out)."""
    import torch
    ctx = small_table_context(31)
    n = 500
    good = ref.libstdcxx_schedule(n)
    assert _call(ctx, *good, n)[0] == L.ERR_STATE                     # before any download
    created, shuffled = hand_made_table(random_keys(n, 6), 6)
    dev = torch.from_numpy(shuffled.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    ctx.scan_begin()
    ctx.import_table(dev.data_ptr(), n)
    assert _call(ctx, *good, n)[0] == L.ERR_STATE                     # inside an open scan
    ctx.scan_end()
    assert _call(ctx, *good, n)[0] == L.ERR_STATE                     # the scan is over, nothing downloaded yet
    keys, _ = ctx.junctions()
    assert np.array_equal(keys, created["key"])
    want = ref.replay(keys, *good, n)

    def still_works():
        rc, order = _call(ctx, *good, n)
        assert rc == L.OK and np.array_equal(order, want)

    still_works()
    ctx.load_begin()
    assert _call(ctx, *good, n)[0] == L.ERR_STATE                     # inside an open load pass
    ctx.load_batch(api.ReadBatch.from_lines([b"", b"ACGT"]))
    ctx.load_end()
    still_works()
    ctx.estimate_begin(10)
    assert _call(ctx, *good, n)[0] == L.ERR_STATE                     # inside an open estimate pass
    ctx.estimate_end()
    still_works()
    assert _call(ctx, *ref.libstdcxx_schedule(n + 1), n + 1)[0] == L.ERR_STATE      # more keys than were downloaded
    still_works()
    for kw in (dict(n_rehashes=0), dict(null=("counts",)), dict(null=("buckets",)), dict(null=("order",))):
        assert _call(ctx, *good, n, **kw)[0] == L.ERR_ARG, kw
        still_works()
    assert _call(ctx, [], [], n)[0] == L.ERR_ARG
    bad = {"counts[0] != 0": ([3], [13]),
           "counts[0] != 0, more stretches": ([5, 13, 29], [13, 29, 59]),
           "descending counts": ([0, 100, 50], [13, 127, 59]),
           "descending counts, at the end": ([0, 0, 13, 12], [1, 13, 29, 59]),
           "a count above n": ([0, n + 1], [13, 1109]),
           "a count above n, in the middle": ([0, 0, 13, n + 1, n + 2], [1, 13, 29, 59, 127]),
           "a zero bucket count": ([0, 13], [13, 0]),
           "a zero bucket count for the empty container": ([0, 0], [0, 13]),
           "2^32 buckets": ([0, 13], [13, 1 << 32]),
           "2^32 buckets for the empty container": ([0, 0], [1 << 32, 13]),
           "2^63 buckets": ([0], [1 << 63])}
    for what, (counts, buckets) in bad.items():
        rc, _ = _call(ctx, counts, buckets, n)
        assert rc == L.ERR_ARG, what
        assert b"fgpu_scan_dump_order" in ctx.lib.fgpu_last_error(ctx.h), what
        still_works()
    rc, _ = _call(ctx, [0, 200], [13, 29], 100)                        # a prefix: the counts are held against n, not against the download
    assert rc == L.ERR_ARG
    still_works()
    with pytest.raises(api.FaucetGpuError, match=f"error {L.ERR_ARG}:"):
        ctx.scan_dump_order([3], [13])
    with pytest.raises(ValueError):
        ctx.scan_dump_order([0, 13], [13])
    assert np.array_equal(ctx.scan_dump_order(*good), want)          # n defaults to what was downloaded last
    ctx.close()


# ---- the command line takes the device's order, and says so ---------------------------------------------------------------------------------
def _faucet_checked(reads, prefix, args):
    """`faucet` with its timing lines and the whole-order check on: the order must have come from the device, and equal the host replay's"""
    env = dict(os.environ, FGPU_CLI_TIMES="1", FAUCET_DEBUG_DUMP_ORDER_CHECK="1")
    r = subprocess.run([CLI, "-read_load_file", str(reads), "-read_scan_file", str(reads), "-file_prefix", str(prefix)] + args,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "dump order on the device (fgpu_scan_dump_order)" in r.stderr, r.stderr[-3000:]
    assert "on the device equals the host replay's" in r.stderr, r.stderr[-3000:]
    return r


def test_cli_takes_the_devices_dump_order_on_a_golden(tmp_path):
    c = Case("c1_k21")
    reads = tmp_path / "reads.fa"
    reads.write_bytes(c.reads_text())
    r = _faucet_checked(reads, tmp_path / "out", c.meta["args"])
    assert f"Distinct junctions: {c.counters['distinct_junctions']} " in r.stdout
    assert (tmp_path / "out.junctions").read_text().split("\n")[:-1] == c.junction_lines()


def test_cli_takes_the_devices_dump_order_past_its_checked_prefix(tmp_path):
    """64 000 reads of 100 bases (1 % errors, a 640 000-base genome) into filters sized for 640 000 k-mers, 128 000 of them singletons:
    bloo2 is overfilled, its false positives make junctions of every few positions -- 77 336 junctions by the oracle, past the 50 000 keys on
    which the command line compares the device's order with its own replay before it trusts the device with the rest."""
    n_reads = 64000
    reads = tmp_path / "reads.fa"
    synth.write_fasta(str(reads), synth.make_reads(synth.make_genome(10 * n_reads, 4321), n_reads, 100, 0.01, 4322))
    r = _faucet_checked(reads, tmp_path / "out", ["-size_kmer", "31", "-max_read_length", "100", "-estimated_kmers", str(10 * n_reads),
                                                  "-singletons", str(2 * n_reads), "--no_cleaning"])
    n_junctions = int(re.search(r"Distinct junctions: (\d+) ", r.stdout).group(1))
    assert n_junctions >= 60000
    assert f"dump order of {n_junctions} junctions on the device equals the host replay's" in r.stderr
    assert len((tmp_path / "out.junctions").read_text().split("\n")) - 1 == n_junctions
