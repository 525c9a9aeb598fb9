"""Merging the sketches of pass 0, without a GPU: the numpy restatement of the planes (tests/estimate_planes_ref.py) that the GPU tests
(tests/test_gpu_estimate_merge.py) compare the device with is pinned here -- the planes of the two parts of a read set, merged by the rule of
include/faucet_gpu.h, are the planes of the whole, word for word, and their counts are tests/estimate_ref.py's, which counts cells another way
(np.unique on the keys, no planes) -- and the command line linked against the CPU stand-in of the ABI, which has no estimate pass, refuses
`-gpus 2 --estimate` as it refuses `--estimate`."""
import os
import subprocess

import numpy as np
import pytest

from tests import estimate_planes_ref as P
from tests import estimate_ref as R
from tests.golden_util import CASES, Case
from tests.test_estimate_cpu import _args, _reads, cli  # noqa: F401  (the fixture: the command line built against tests/stub)

BITS = [8, 12]


@pytest.mark.parametrize("name", CASES)
def test_merged_planes_of_two_parts_are_the_planes_of_the_whole(name):
    """every golden's reads cut at three record boundaries (a pair's two records stay together), 2^8 cells per level -- crowded: every level
    has cells hit twice on both sides -- and 2^12"""
    c = Case(name)
    lines = c.lines()
    unit = 2 if c.paired else 1
    n = len(lines) // unit
    whole = R.golden_canon(name)
    for r_bits in BITS:
        want = P.planes(whole, r_bits)
        empty, once, kmers = R.golden_counts(name, r_bits)
        assert P.counts(want, r_bits) == (empty, once)
        for cut in (unit * (n // 7), unit * (n // 2), unit * (n - 1)):
            a, b = R.canon_kmers(lines[:cut], c.k), R.canon_kmers(lines[cut:], c.k)
            assert len(a) + len(b) == kmers and (cut != unit * (n // 2) or min(len(a), len(b)) > 0)      # (a last record may be shorter than k)
            pa, pb = P.planes(a, r_bits), P.planes(b, r_bits)
            got = P.merge(pa, pb)
            assert np.array_equal(got, want), (r_bits, cut)
            assert np.array_equal(P.merge(pb, pa), want)
            assert P.counts(got, r_bits) == (empty, once)
            if r_bits == 8 and cut == unit * (n // 2):      # the merge is more than an OR here: cells seen once on each side
                assert not np.array_equal(pa | pb, want)


def test_the_rule_on_every_pair_of_cell_states():
    """0, 1 and 2 (= at least twice) add and saturate at 2; merging is associative and commutative, so any reduction order gives the same planes"""
    word = {0: 0x00000000, 1: 0x00000001, 2: 0x00010001}
    for x in range(3):
        for y in range(3):
            got = int(P.merge(np.array([word[x] << 3], np.uint32), np.array([word[y] << 3], np.uint32))[0])
            assert got == word[min(x + y, 2)] << 3, (x, y)
    rng = np.random.default_rng(3)

    def random_planes():
        seen = rng.integers(0, 1 << 16, 64, dtype=np.uint32)
        return seen | ((rng.integers(0, 1 << 16, 64, dtype=np.uint32) & seen) << np.uint32(16))

    a, b, c = random_planes(), random_planes(), random_planes()
    assert np.array_equal(P.merge(P.merge(a, b), c), P.merge(a, P.merge(b, c)))
    assert np.array_equal(P.merge(a, b), P.merge(b, a))
    assert np.array_equal(P.merge(a, np.zeros(64, np.uint32)), a)
    states = P.cell_states(P.merge(a, b), 8)
    assert np.array_equal(states, np.minimum(P.cell_states(a, 8) + P.cell_states(b, 8), 2))


def test_estimate_over_read_shards_is_refused_where_the_library_lacks_the_entry_points(cli, tmp_path):  # noqa: F811
    c = Case("c1_k21")
    inp, prefix = _reads(c, tmp_path), str(tmp_path / "out")
    r = subprocess.run([cli, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", prefix, "--estimate", "-gpus", "2"] + _args(c),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "--estimate" in r.stderr and "lacks the entry points" in r.stderr
    for name in ("fgpu_estimate_begin", "fgpu_estimate_batch", "fgpu_estimate_end"):
        assert name in r.stderr
    assert r.stdout == "" and not os.path.exists(prefix + ".bloom")      # before anything is read, sized or printed
