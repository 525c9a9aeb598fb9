"""The estimator of pass 0 (include/faucet_gpu.h, fgpu_estimate_*) restated in numpy, for tests/test_estimate_cpu.py and tests/test_gpu_estimate.py.

Canonical k-mers of sequence lines with A0 C1 T2 G3, split at everything but upper-case ACGT; h = the murmur3 finaliser; level
min(clz64(h) / 4, 3); cell h & (m - 1); cells counted with np.unique, so r_bits = 30 needs no dense array."""
import functools
import math

import numpy as np

from tests.golden_util import Case

LEVELS, SHIFT = 4, 4
_U = np.uint64


def canon_kmers(lines, k):
    """the canonical k-mer of every valid window of every line, one entry per occurrence (uint64)"""
    if not lines:
        return np.zeros(0, _U)
    text = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    n = len(text) - k + 1
    if n <= 0:
        return np.zeros(0, _U)
    ok = (text == ord("A")) | (text == ord("C")) | (text == ord("G")) | (text == ord("T"))
    code = ((text >> 1) & 3).astype(_U)
    bad = np.concatenate([[0], np.cumsum(~ok)])
    valid = (bad[k:k + n] - bad[:n]) == 0
    fwd, rc = np.zeros(n, _U), np.zeros(n, _U)
    for j in range(k):
        c = code[j:j + n]
        fwd = (fwd << _U(2)) | c
        rc |= (c ^ _U(2)) << _U(2 * j)
    return np.minimum(fwd, rc)[valid]


def mix(x):
    """fd_mix: the 64-bit finaliser of murmur3, a bijection"""
    x = np.asarray(x, dtype=_U).copy()
    x ^= x >> _U(33)
    x *= _U(0xff51afd7ed558ccd)
    x ^= x >> _U(33)
    x *= _U(0xc4ceb9fe1a85ec53)
    x ^= x >> _U(33)
    return x


def level_of(h):
    """min(clz64(h) / 4, 3): at least 4, 8, 12 leading zeros"""
    return (h < _U(1 << 60)).astype(np.int64) + (h < _U(1 << 56)) + (h < _U(1 << 52))


def counts(canon, r_bits):
    """(empty[4], once[4], kmers) of the sketch of these occurrences with 2^r_bits cells per level"""
    m = 1 << r_bits
    h = mix(canon)
    key = level_of(h).astype(_U) * _U(m) + (h & _U(m - 1))
    cells, hits = np.unique(key, return_counts=True)
    lv = (cells >> _U(r_bits)).astype(np.int64)
    empty = [m - int((lv == l).sum()) for l in range(LEVELS)]
    once = [int(((lv == l) & (hits == 1)).sum()) for l in range(LEVELS)]
    return empty, once, len(canon)


def solve(empty, once, r_bits):
    """(level, F0, f1), or None where level 3 is not usable"""
    m = 1 << r_bits
    usable = [8 * e >= m for e in empty]
    if not usable[LEVELS - 1]:
        return None
    level = LEVELS - 1
    while level > 0 and usable[level - 1]:
        level -= 1
    f0 = sum(float(m) * math.log(float(m) / float(empty[l])) for l in range(level, LEVELS))
    f1 = sum(float(m) * float(once[l]) / float(empty[l]) for l in range(level, LEVELS))
    return level, 16.0 ** level * f0, 16.0 ** level * f1


def exact(canon):
    """(distinct canonical k-mers, those seen exactly once)"""
    _, n = np.unique(canon, return_counts=True)
    return len(n), int((n == 1).sum())


@functools.lru_cache(maxsize=None)
def golden_canon(name):
    """the occurrences of a golden's reads (computed once per process, shared, never written to)"""
    c = Case(name)
    out = canon_kmers(c.lines(), c.k)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def golden_counts(name, r_bits):
    return counts(golden_canon(name), r_bits)
