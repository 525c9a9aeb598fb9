"""The packed stream block (include/faucet_gpu.h, fgpu_packed) restated in plain numpy / Python, for tests/test_pack_ref_cpu.py and
tests/test_gpu_pack_layout.py.  Imports no project code: it is written from the description below, one stream position at a time.

The stream of a batch of n sequence lines
    T = total bytes + n: every read is followed by ONE separator position; read i starts at S_i = (bytes before it) + i.
    n_words = ceil(T / 64).
Token order
    A read is cut into its maximal runs of good bytes (upper-case A C G T, nothing else) and of other bytes.  The runs are laid out in REVERSE
    run order, the bytes inside a run in their own order -- so ascending stream position is the order in which the reference works through a
    read's pieces (getUnambiguousReads hands them out last first).
The block: 3 * (n_words + 8) + 2 little-endian 64-bit words
    codes plane   2 * (n_words + 8) words.  Position p: word p // 32, bits 62 - 2 * (p % 32) and the one above -- the first position of a
                  word in its two most significant bits.  A good byte c has code (c >> 1) & 3 (A0 C1 T2 G3), every other position code 0.
    bad plane     n_words + 8 words.  Position p: bit p % 64 of word p // 64.  1 for separators, for bytes that are not good, for every
                  position from T to the end of word n_words - 1, and for all of the 8 padding words (whose code words are 0).
    trailer       {digest, T}.  digest = sum mod 2^64, over the 3 * (n_words + 8) words before it, of mix(word ^ ((index + 1) * GOLDEN)),
                  mix = the finaliser of splitmix64, index = the word's place in the block.
    nbytes = 24 * (n_words + 8) + 16."""
import numpy as np

PADW = 8
GOLDEN = 0x9E3779B97F4A7C15
GOOD = frozenset(b"ACGT")
_U = np.uint64


def runs(line):
    """the maximal runs of good / other bytes of one line, in the line's order: [(is_good, bytes), ...]"""
    out, s = [], 0
    while s < len(line):
        good = line[s] in GOOD
        e = s + 1
        while e < len(line) and (line[e] in GOOD) == good:
            e += 1
        out.append((good, line[s:e]))
        s = e
    return out


def stream(lines, reverse_tokens=True):
    """(code[T], bad[T]) of the batch, one entry per stream position.  reverse_tokens=False lays every read's runs out in the line's own order:
    NOT the format, only what a test needs to show that it can tell the two apart."""
    code, bad = [], []
    for line in lines:
        tokens = runs(line)
        for good, run in (reversed(tokens) if reverse_tokens else tokens):
            for c in run:
                code.append((c >> 1) & 3 if good else 0)
                bad.append(0 if good else 1)
        code.append(0)                    # the separator behind the read
        bad.append(1)
    return code, bad


def n_words_of(T):
    return (T + 63) // 64


def nbytes_of(T):
    return 24 * (n_words_of(T) + PADW) + 16


def digest(words):
    """sum over the words of the splitmix64 finaliser of word ^ ((index + 1) * GOLDEN), mod 2^64 (uint64 arithmetic wraps)"""
    w = np.asarray(words, dtype=_U)
    with np.errstate(over="ignore"):
        x = w ^ ((np.arange(len(w), dtype=_U) + _U(1)) * _U(GOLDEN))
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        x ^= x >> _U(31)
        return int(np.add.reduce(x, dtype=_U)) if len(x) else 0


def pack(lines, reverse_tokens=True):
    """the block of a batch of at least one line, as uint64 words (block.tobytes() is the device buffer, block.nbytes its nbytes)"""
    assert len(lines) > 0, "a batch without reads has no block"
    code, bad = stream(lines, reverse_tokens)
    T = len(code)
    assert T == sum(len(x) for x in lines) + len(lines)
    plane = n_words_of(T) + PADW
    codes_w = [0] * (2 * plane)
    bad_w = [0] * plane
    for p in range(T):
        codes_w[p // 32] |= code[p] << (62 - 2 * (p % 32))
        bad_w[p // 64] |= bad[p] << (p % 64)
    for p in range(T, 64 * plane):        # the tail of the last word and the padding words
        bad_w[p // 64] |= 1 << (p % 64)
    body = np.array(codes_w + bad_w, dtype=_U)
    return np.concatenate([body, np.array([digest(body), T], dtype=_U)])


def unpack(block):
    """(code[T], bad[T], T) of a block, one entry per stream position"""
    block = np.asarray(block, dtype=_U)
    T = int(block[-1])
    plane = n_words_of(T) + PADW
    assert len(block) == 3 * plane + 2
    p = np.arange(T, dtype=np.int64)
    code = (block[p // 32] >> (62 - 2 * (p % 32)).astype(_U)) & _U(3)
    bad = (block[2 * plane + p // 64] >> (p % 64).astype(_U)) & _U(1)
    return code, bad.astype(bool), T


def decode_kmers(block, k):
    """the canonical k-mers (A0 C1 T2 G3, the smaller of a window and its reverse complement) of all windows of k good positions, in ascending
    stream position: what the passes work through, in their order"""
    code, bad, T = unpack(block)
    n = T - k + 1
    if n <= 0:
        return np.zeros(0, _U)
    seen = np.concatenate([[0], np.cumsum(bad)])
    valid = (seen[k:k + n] - seen[:n]) == 0
    fwd, rc = np.zeros(n, _U), np.zeros(n, _U)
    for j in range(k):
        c = code[j:j + n]
        fwd = (fwd << _U(2)) | c
        rc |= (c ^ _U(2)) << _U(2 * j)
    return np.minimum(fwd, rc)[valid]
