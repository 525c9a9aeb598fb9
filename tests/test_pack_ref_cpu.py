"""tests/pack_ref.py pinned before it judges a kernel (tests/test_gpu_pack_layout.py): the k-mers it decodes from its own blocks, fed through the
two-filter rule in stream order, give the oracle's filters -- on inputs where the order of a read's tokens changes the outcome --; blocks small
enough to check by eye; the digest against a second, scalar implementation.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import pack_ref as P
from tests.golden_util import Case

ONES = 0xFFFFFFFFFFFFFFFF
M64 = (1 << 64) - 1


def generated_lines(seed=7, n=120):
    """reads of 30 to 90 bytes over a genome of 4000, so that some k-mers repeat and most do not; two in three carry one to three Ns, some at
    either end, one is shorter than k, one is empty, one is all N"""
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 4000)
    out = []
    for i in range(n):
        ln = int(rng.integers(30, 91))
        at = int(rng.integers(0, len(genome) - ln))
        r = genome[at:at + ln].copy()
        if i % 3:
            r[rng.integers(0, ln, int(rng.integers(1, 4)))] = ord("N")
        if i % 10 == 4:
            r[0] = ord("N")
        if i % 10 == 7:
            r[-1] = ord("N")
        out.append(r.tobytes())
    out[2] = b""
    out[13] = b"NNNN"
    out[25] = b"ACGTACG"
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(lines, k, tai, n_hash): the filters are sized so that bloo1 ends between a quarter and a half full -- false positives occur, and which
    k-mer meets one depends on what was added before it"""
    if name == "generated":
        return generated_lines(), 15, 1 << 13, 2
    c = Case(name)
    return c.lines(), c.k, 1 << 17, 2


def two_filter_rule(kmers, tai, nh):
    """load_two_filters over a sequence of canonical k-mers: a k-mer bloo1 holds (or seems to) goes to bloo2, any other into bloo1"""
    b1, b2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    for km in kmers:
        km = int(km)
        if b1.contains(km):
            b2.add(km)
        else:
            b1.add(km)
    return b1.bits().copy(), b2.bits().copy()


@pytest.mark.parametrize("name", ["generated", "ragged_k31", "c1_k21"])
def test_decoded_kmers_in_stream_order_load_as_the_oracle_loads_the_reads(name):
    lines, k, tai, nh = case(name)
    kmers = P.decode_kmers(P.pack(lines), k)
    o1, o2 = po.Bloom(tai, nh), po.Bloom(tai, nh)
    bases, offs = po.reads_from_lines(lines)
    lst = po.load_two_filters(o1, o2, bases, offs, k)
    assert len(kmers) == lst.kmers > 0
    b1, b2 = two_filter_rule(kmers, tai, nh)
    weight = o1.weight()
    assert 0.2 < weight < 0.6, weight                       # neither empty of false positives nor saturated
    assert np.array_equal(b1, o1.bits()) and np.array_equal(b2, o2.bits())
    # the pin is order-sensitive: the same k-mers with every read's tokens in the line's own order load to another bloo2
    forward = P.decode_kmers(P.pack(lines, reverse_tokens=False), k)
    assert np.array_equal(np.sort(forward), np.sort(kmers))
    if name == "c1_k21":                                    # no read of this golden has a bad byte: nothing to reverse
        assert np.array_equal(forward, kmers)
        return
    assert not np.array_equal(forward, kmers)
    if name == "generated":
        assert not np.array_equal(two_filter_rule(forward, tai, nh)[1], o2.bits()), "this input cannot tell the token orders apart"
    # ragged_k31 cannot tell them apart through its filters.  bloo1 ends as the same bits in any order, and bloo2 differs only where a k-mer that
    # occurs once finds all its bits set by the first occurrences in the OTHER piece of its own read: 86 of its 1201 reads have two pieces, at
    # threefold coverage.  On this golden the comparison above pins the k-mers and their count; the generated reads pin the order.


# ---- blocks to check by eye -----------------------------------------------------------------------------------------------------------------
def block_of(codes0, bad0, T):
    """a block of one stream word: word 0 of either plane as given, every other code word 0, the 8 padding words of the bad plane all ones"""
    body = [codes0] + [0] * 17 + [bad0] + [ONES] * 8
    return body, T


HAND = {
    # A0 C1 G3 T2 and the separator: 00 01 11 10 00 from the top; positions 0-3 good, 4 the separator, 5-63 behind T
    "ACGT": ([b"ACGT"], block_of(0x1E00000000000000, 0xFFFFFFFFFFFFFFF0, 5)),
    # runs AC | N | GT laid out GT N AC: 11 10 00 00 01 00; bad at 2 (N), 5 (separator) and from 6 on: ~0b011011
    "ACNGT": ([b"ACNGT"], block_of(0xE040000000000000, 0xFFFFFFFFFFFFFFE4, 6)),
    "an empty read": ([b""], block_of(0, ONES, 1)),
    "a read of only N": ([b"N"], block_of(0, ONES, 2)),
    # two reads share word 0: GT N AC | sep | C N -> N C | sep: 11 10 00 00 01 00 00 01 00; bad at 2, 5, 6, 8 and from 9 on
    "ACNGT, CN": ([b"ACNGT", b"CN"], block_of(0xE041000000000000, 0xFFFFFFFFFFFFFF64, 9)),
}


@pytest.mark.parametrize("name", list(HAND))
def test_blocks_small_enough_to_check_by_eye(name):
    lines, (body, T) = HAND[name]
    got = P.pack(lines)
    assert got.dtype == np.uint64 and got.nbytes == P.nbytes_of(T) == 24 * 9 + 16 == 232
    assert [int(w) for w in got[:-2]] == body
    assert int(got[-1]) == T
    assert int(got[-2]) == scalar_digest(body)


def test_a_stream_of_exactly_one_word_and_one_position_more():
    """T = 64: no tail bits, the padding starts at bad word 1; T = 65: a second stream word whose bad bits 1-63 are the tail"""
    line = b"ACGT" * 15 + b"ACG"                            # 63 bytes + separator
    got = P.pack([line])
    assert int(got[-1]) == 64 and len(got) == 3 * 9 + 2
    assert int(got[18]) == 1 << 63 and [int(w) for w in got[19:27]] == [ONES] * 8
    assert int(got[0]) == 0x1E1E1E1E1E1E1E1E and int(got[1]) == 0x1E1E1E1E1E1E1E1C and not got[2:18].any()
    got = P.pack([line + b"T"])
    assert int(got[-1]) == 65 and len(got) == 3 * 10 + 2
    assert int(got[1]) == 0x1E1E1E1E1E1E1E1E and int(got[2]) == 0 and int(got[20]) == 0 and int(got[21]) == ONES
    assert [int(w) for w in got[22:30]] == [ONES] * 8


def test_every_byte_value_is_good_or_bad_exactly_as_the_rule_says():
    line = bytes(range(256))
    code, bad = P.stream([line], reverse_tokens=False)
    assert [i for i in range(256) if not bad[i]] == [65, 67, 71, 84]
    assert [code[i] for i in (65, 67, 71, 84)] == [0, 1, 3, 2] and sum(code) == 6


def test_unpack_and_decode_read_what_pack_wrote():
    lines = generated_lines(seed=3, n=40)
    block = P.pack(lines)
    code, bad, T = P.unpack(block)
    want_code, want_bad = P.stream(lines)
    assert T == len(want_code) and code.tolist() == want_code and bad.tolist() == [bool(b) for b in want_bad]
    # the k-mers of one read, by hand: pieces last first, windows of a piece ascending
    km = P.decode_kmers(P.pack([b"ACGTNTTGCA"]), 4)
    enc = {"A": 0, "C": 1, "T": 2, "G": 3}

    def canon(s):
        f = functools.reduce(lambda x, ch: x * 4 + enc[ch], s, 0)
        r = functools.reduce(lambda x, ch: x * 4 + (enc[ch] ^ 2), reversed(s), 0)
        return min(f, r)

    assert km.tolist() == [canon("TTGC"), canon("TGCA"), canon("ACGT")]


# ---- the digest ---------------------------------------------------------------------------------------------------------------------------
def scalar_digest(words):
    total = 0
    for index, w in enumerate(words):
        x = (w ^ ((index + 1) * 0x9E3779B97F4A7C15)) & M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
        total += x ^ (x >> 31)
    return total & M64


def test_the_digest_against_a_scalar_implementation():
    # splitmix64 seeded with 0 returns mix(GOLDEN) first: 0xE220A8397B1DCDAF (the published first output) -- a zero word at index 0
    assert scalar_digest([0]) == 0xE220A8397B1DCDAF == P.digest(np.zeros(1, np.uint64))
    zeros = np.zeros(3 * 9, np.uint64)
    assert P.digest(zeros) == scalar_digest([0] * 27)
    one = zeros.copy()
    one[13] = 1
    assert P.digest(one) == scalar_digest([0] * 13 + [1] + [0] * 13) != P.digest(zeros)
    moved = zeros.copy()
    moved[14] = 1                                            # the same word elsewhere: the digest knows the place
    assert P.digest(moved) not in (P.digest(one), P.digest(zeros))
    rng = np.random.default_rng(5)
    words = rng.integers(0, 1 << 64, 1000, dtype=np.uint64)
    assert P.digest(words) == scalar_digest([int(w) for w in words])
    block = P.pack(generated_lines(seed=9, n=30))
    assert int(block[-2]) == scalar_digest([int(w) for w in block[:-2]])
