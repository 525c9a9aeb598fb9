"""tests/dump_order_ref.py, the reference the device's dump order is compared with (tests/test_gpu_dump_order.py), pinned to the standard
library: a small stand-alone program (tests/host/dump_order_dump.cpp, built here with the address and undefined-behaviour sanitizers: host
code only) prints the library's rehash schedule and the iteration order of a real std::unordered_map; the linked-list replay must give that
order, and LIBSTDCXX_SCHEDULE must be that schedule.  The replay is also compared with the closed form (one sort per stretch, what the
device computes) on random ARTIFICIAL schedules, which is what makes such schedules a sound input to the device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dump_order_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("dump_order") / "dump_order_dump")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++11", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I",
                        os.path.join(ROOT, "faucet_amd", "host"), os.path.join(ROOT, "tests", "host", "dump_order_dump.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _library(exe, keys, tmp_path, schedule_n=None):
    """(schedule as a list of (count, buckets), the real container's order) for these keys"""
    path = tmp_path / "keys.bin"
    np.ascontiguousarray(keys, dtype="<u8").tofile(path)
    r = subprocess.run([exe, str(path)] + ([str(schedule_n)] if schedule_n is not None else []), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-500:] + r.stderr[-3000:]
    sch_line, order_line = r.stdout.split("\n")[:2]
    assert sch_line.startswith("schedule") and order_line.startswith("order")
    sch = [tuple(int(x) for x in w.split(":")) for w in sch_line.split()[1:]]
    return sch, np.array(order_line.split()[1:], dtype=np.uint32)


def test_the_schedule_constant_is_the_librarys(dump_exe, tmp_path):
    sch, _ = _library(dump_exe, np.zeros(0, np.uint64), tmp_path, schedule_n=300000)
    assert tuple(sch) == ref.LIBSTDCXX_SCHEDULE
    for n in (1, 2, 13, 14, 29, 30, 257, 258, 4097, 70001, 172933, 172934, 180000, 300000):
        sch, _ = _library(dump_exe, np.zeros(0, np.uint64), tmp_path, schedule_n=n)
        counts, buckets = ref.libstdcxx_schedule(n)
        assert sch == list(zip(counts, buckets)), n
    sch, _ = _library(dump_exe, np.zeros(0, np.uint64), tmp_path, schedule_n=0)      # (no insertion: the library has not left its one bucket yet)
    assert sch == [(0, 1)] and ref.libstdcxx_schedule(0) == ([0, 0], [1, 13])
    with pytest.raises(ValueError):
        ref.libstdcxx_schedule(351062)


@pytest.mark.parametrize("n", [0, 1, 13, 14, 1000, 54321])
def test_replay_equals_the_real_container_on_random_62_bit_keys(n, dump_exe, tmp_path):
    keys = np.unique(np.random.default_rng(100 + n).integers(0, 1 << 62, size=n + 16, dtype=np.uint64))
    keys = np.random.default_rng(n).permutation(keys)[:n]
    _, order = _library(dump_exe, keys, tmp_path)
    counts, buckets = ref.libstdcxx_schedule(n)
    got = ref.replay(keys, counts, buckets, n)
    assert got.dtype == np.uint32 and np.array_equal(got, order)
    if n:
        assert np.array_equal(np.sort(got), np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("name", sorted(ref.crowded_k5_sets()))
def test_replay_equals_the_real_container_on_crowded_small_keys(name, dump_exe, tmp_path):
    keys = ref.crowded_k5_sets()[name]
    assert len(np.unique(keys)) == len(keys) and int(keys.max()) < 1024
    sch, order = _library(dump_exe, keys, tmp_path)
    counts, buckets = ref.libstdcxx_schedule(len(keys))
    assert sch == list(zip(counts, buckets))
    assert np.array_equal(ref.replay(keys, counts, buckets), order)
    for m in (1, 13, 14, 300):       # prefixes: replay(keys, ..., m) speaks of keys[:m]
        _, order = _library(dump_exe, keys[:m], tmp_path)
        assert np.array_equal(ref.replay(keys, *ref.libstdcxx_schedule(m), m), order)


def _closed_form(keys, counts, buckets, n):
    """the closed form of faucet_amd/host/junction_order.h (DumpOrder::of_sorted) for an arbitrary schedule: per stretch, the list as it
    stands followed by the nodes inserted until the next rehash, sorted by (first position of the node's bucket, own position), latest first"""
    lst = []
    for j, (c, b) in enumerate(zip(counts, buckets)):
        m = counts[j + 1] if j + 1 < len(counts) else n
        if m == 0:
            continue
        seq = lst[:c] + list(range(c, m))
        first = {}
        for t, node in enumerate(seq):
            first.setdefault(int(keys[node]) % b, t)
        lst = [seq[t] for t in sorted(range(m), key=lambda t: (-first[int(keys[seq[t]]) % b], -t))]
    return np.array(lst, dtype=np.uint32)


def test_replay_equals_the_closed_form_on_artificial_schedules():
    """random schedules -- 1 to 6 rehashes, repeated counts, a rehash at count n, bucket counts from 1 to 1 000 003 that may shrink,
    crowded and sparse key spaces: the two rules and the sorts agree, so the device may be asked for schedules no library produces"""
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(1, 400))
        space = int(rng.choice([n, 2 * n + 3, 1 << 20, 1 << 62]))
        keys = rng.permutation(n).astype(np.uint64) if space == n else np.unique(rng.integers(0, space, size=4 * n, dtype=np.uint64))
        keys = rng.permutation(keys)[:n]
        n = len(keys)
        phases = int(rng.integers(1, 7))
        counts = [0] + sorted(int(x) for x in rng.integers(0, n + 1, size=phases - 1))
        buckets = [int(rng.choice([1, 2, 3, 7, 13, int(rng.integers(1, 2 * n + 2)), 1000003])) for _ in range(phases)]
        assert np.array_equal(ref.replay(keys, counts, buckets, n), _closed_form(keys, counts, buckets, n)), (trial, counts, buckets)


def test_replay_refuses_what_is_no_schedule():
    keys = np.arange(10, dtype=np.uint64)
    for counts, buckets in (([1], [3]), ([0, 5, 4], [1, 2, 3]), ([0, 11], [1, 2]), ([0], [0]), ([], []), ([0, 1], [1])):
        with pytest.raises(ValueError):
            ref.replay(keys, counts, buckets, 10)
