"""The planes of pass 0's sketch (faucet_amd/csrc/estimate.hip) restated in numpy, word for word, and the rule by which two sketches merge --
for tests/test_estimate_merge_cpu.py, which pins this restatement against tests/estimate_ref.py's counts, and tests/test_gpu_estimate_merge.py,
which compares the device's planes with it.

The planes are 2^r_bits bytes = 2^(r_bits - 2) 32-bit words: level l in words [l << (r_bits - 4), (l + 1) << (r_bits - 4)), cell c of a level
in word c >> 4, `seen` (hit at least once) in bit c & 15, `twice` (hit at least twice) in bit 16 + (c & 15).  Dense arrays: for small r_bits."""
import numpy as np

from tests import estimate_ref as R

_U = np.uint64
LOW = np.uint32(0xFFFF)


def planes(canon, r_bits):
    """the word image a pass over these occurrences (canonical k-mers, one entry each) ends with"""
    m = 1 << r_bits
    h = R.mix(canon)
    key = R.level_of(h).astype(_U) * _U(m) + (h & _U(m - 1))          # level * m + cell: 16 consecutive keys share a word
    cells, hits = np.unique(key, return_counts=True)
    out = np.zeros(m // 4, np.uint32)
    word, bit = (cells >> _U(4)).astype(np.int64), (cells & _U(15)).astype(np.uint32)
    np.bitwise_or.at(out, word, np.uint32(1) << bit)
    np.bitwise_or.at(out, word[hits >= 2], np.uint32(1) << (bit[hits >= 2] + np.uint32(16)))
    return out


def merge(a, b):
    """saturating addition of two-bit counters: out = a | b | ((a & b & 0xFFFF) << 16)"""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    return a | b | ((a & b & LOW) << np.uint32(16))


def cell_states(words, r_bits, level=None):
    """the counter of every cell (0, 1 or 2 = at least twice), in cell order; one level's cells, or all four levels'"""
    words = np.asarray(words, np.uint32)
    if level is not None:
        per = 1 << (r_bits - 4)
        words = words[level * per:(level + 1) * per]
    shifts = np.arange(16, dtype=np.uint32)
    seen = (words[:, None] >> shifts) & np.uint32(1)
    twice = (words[:, None] >> (shifts + np.uint32(16))) & np.uint32(1)
    assert not (twice & ~seen).any(), "`twice` without `seen`: no sketch gives such a cell"
    return (seen + twice).astype(np.int64).reshape(-1)


def counts(words, r_bits):
    """(empty[4], once[4]) of a word image"""
    empty, once = [], []
    for l in range(R.LEVELS):
        s = cell_states(words, r_bits, l)
        empty.append(int((s == 0).sum()))
        once.append(int((s == 1).sum()))
    return empty, once
