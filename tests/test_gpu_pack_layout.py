"""k_pack / k_pack_fix (faucet_amd/csrc/pack.hip) against the restatement of the packed stream block (tests/pack_ref.py): every block byte for
byte -- codes, bad plane, padding words, digest and T -- at the smallest shapes that take each branch of the two kernels, from host, device
and fgpu_text_split batches, through fgpu_load_slice_pack and through fgpu_estimate_keep; and the consumers (fgpu_load_slice_batch_packed,
fgpu_load_batch_packed) fed blocks that the restatement built on the host: the oracle's filters, stats and junctions.  Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from oracle import pyoracle as po
from tests import pack_ref as P
from tests.golden_util import Case
from tests.test_gpu_parity import oracle_run
from tests.test_gpu_slices_packed import Reader

gpu = pytest.mark.gpu          # the tests that pack or load on the device; the checks of the shapes themselves run anywhere

ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---- the launch rule of k_pack, restated to say where a shape's wave boundaries fall ------------------------------------------------------------
def wave_starts(T):
    """first stream position of every wave of k_pack that has work.  One lane per half-word (32 positions) of the padded planes, hw = 2 *
    (n_words + 8) of them; the grid is ceil((hw / 4 + 1) / 256) blocks of 4 waves (four trips to a wave), capped at 4096 blocks; a wave takes
    `per` = ceil(hw / waves) rounded up to a multiple of 64 consecutive half-words, in trips of 64 (2048 positions)"""
    hw = 2 * (P.n_words_of(T) + P.PADW)
    blocks = min(4096, max(1, (hw // 4 + 1 + 255) // 256))
    waves = 4 * blocks
    per = ((hw + waves - 1) // waves + 63) // 64 * 64
    return blocks, [w * per * 32 for w in range(waves) if w * per < hw]


def where(lines, pos):
    """what lies at stream position `pos`: ("in", length) inside a read, ("sep", length) on the separator of a read of that length, with
    length 0 also saying whether both neighbours are empty ("empties"), or ("tail", 0) at or behind T"""
    s = 0
    for i, ln in enumerate(lines):
        if pos < s + len(ln):
            return "in", len(ln)
        if pos == s + len(ln):
            if len(ln) == 0 and 0 < i < len(lines) - 1 and not lines[i - 1] and not lines[i + 1]:
                return "empties", 0
            return "sep", len(ln)
        s += len(ln) + 1
    return "tail", 0


class Build:
    """lines appended while the stream position they reach is tracked; the good bytes come from a genome of 3000, so that k-mers repeat"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.genome = self.rng.choice(ACGT, 3000)
        self.lines, self.pos = [], 0

    def add(self, line):
        self.lines.append(bytes(line))
        self.pos += len(line) + 1

    def good(self, n):
        at = int(self.rng.integers(0, 3000))
        self.add(np.resize(np.roll(self.genome, -at), n).tobytes())

    def good_with_separator_at(self, pos):
        assert pos > self.pos
        self.good(pos - self.pos)
        assert self.pos == pos + 1

    def empties(self, n):
        for _ in range(n):
            self.add(b"")

    def shorts(self, n):
        """reads of 1 to 31 bytes, 64 of them span far fewer than the 2048 positions of a trip; every fifth has a bad byte"""
        for i in range(n):
            r = self.rng.choice(ACGT, 1 + (i * 7) % 31)
            if i % 5 == 2:
                r[int(self.rng.integers(0, len(r)))] = (ord("N"), ord("a"), ord("n"))[i % 3]
            self.add(r.tobytes())


@functools.lru_cache(maxsize=None)
def mixed(size):
    """The batch that makes k_pack change between its two look-ups of the read that holds a position -- bisection over 64 read starts held one
    per lane while they reach past the trip's last half-word (long reads), bisection over the offsets in memory while they do not (reads of 0 to
    31 bytes) -- within one wave's run and from wave to wave, with the register window started again in the middle of a run.

    size 12: about 100 empty reads, one read to position 5400, 200 reads of 1 to 31, one read that ends at 12250, 70 empty reads: T = 12321.
        193 + 8 plane words, 402 half-words, 101 lanes asked for = 1 block, 4 waves of ceil(402 / 4) = 101 -> 128 half-words = 4096 positions: wave 1 starts inside the first long read and
        meets the short reads in its second trip, wave 2 starts among the short reads and meets the second long read, wave 3 starts among the
        empty reads at the end (12288) and holds the last 33 positions, the tail of the last word and the padding.
    size 40 (T = 41431: 656 plane words, 1312 half-words, 329 lanes asked for = 2 blocks) and 70 (T = 69901: 1101 plane words, 2202
        half-words, 551 lanes = 3 blocks): the same pieces again and again; 8 and 12 waves of 192 half-words = 6144 positions, so a wave starts
        at every multiple of 6144 below T (7 and 12 of them have work).  6144 lies inside a long read, 12288 on the separator behind one,
        18432 in a run of 100 empty reads, 24576 and 36864 among short reads, 30720 inside a long read; from 43008 on size 70 repeats the
        pattern and ends inside a long read (67584).  tests below assert all of this from wave_starts()."""
    b = Build(size)
    b.empties(100)
    if size == 12:
        b.good_with_separator_at(5400)
        b.shorts(200)
        b.good_with_separator_at(12250)
        b.empties(70)
        return b.lines
    rounds = {40: 1, 70: 2}[size]
    for r in range(rounds):
        base = r * 36864
        b.good_with_separator_at(base + 7000)
        b.shorts(200)
        b.good_with_separator_at(base + 12288)
        b.empties(70)
        b.shorts(200)
        b.good_with_separator_at(base + 18400)
        b.empties(100)
        b.good(5000)
        b.shorts(200)
        b.good(3000)
        b.empties(70)
        if size == 70 and r == 1:                # (the third block's per-wave share grows beyond 192 half-words above 73216 positions)
            break
        b.good(5000)
        b.shorts(200)
    b.good(3000)
    b.empties(70)
    return b.lines


def stream_T(lines):
    return sum(len(x) for x in lines) + len(lines)


# ---- packing and comparing ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reader():
    rd = Reader()
    yield rd
    rd.close()


@pytest.fixture()
def packer():
    """a context in a sliced pass that owns no bit: it only packs"""
    ctx = api.Context(21, 1 << 12, 2)
    ctx.load_slice_begin(0, 0)
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=64)
def _want(lines):
    return P.pack(list(lines))


def want_block(lines):
    return _want(tuple(lines))


def assert_block(got_bytes, lines, what=""):
    """the device block's bytes are the restatement's; on a difference, say which plane and word"""
    want = want_block(lines)
    assert len(got_bytes) == want.nbytes == P.nbytes_of(stream_T(lines)), what
    got = np.frombuffer(got_bytes.tobytes(), np.uint64)
    if np.array_equal(got, want):
        return
    plane = P.n_words_of(stream_T(lines)) + P.PADW
    at = int(np.flatnonzero(got != want)[0])
    part = "codes" if at < 2 * plane else "bad plane" if at < 3 * plane else "trailer"
    word = at if at < 2 * plane else at - 2 * plane if at < 3 * plane else at - 3 * plane
    raise AssertionError(f"{what}: {int((got != want).sum())} words differ, the first is {part} word {word} of {plane} in the plane "
                         f"(first position {word * (32 if part == 'codes' else 64)}, T = {stream_T(lines)}): got {int(got[at]):#018x}, want {int(want[at]):#018x}")


def pack_and_check(reader, packer, batch, lines, what=""):
    pk = packer.load_slice_pack(batch)
    assert (pk.T, pk.n_reads, pk.nbytes) == (stream_T(lines), len(lines), P.nbytes_of(stream_T(lines))), what
    assert_block(reader.read(packer, pk.block_dev, pk.nbytes), lines, what)


def host_batch(lines, first_offset=0):
    """a host batch whose offsets[0] is `first_offset`: that many bytes of another batch lie in front of it"""
    b = api.ReadBatch.from_lines(lines)
    if not first_offset:
        return b
    bases = np.concatenate([np.full(first_offset, ord("C"), np.uint8), b.bases])
    return api.ReadBatch(bases, b.offsets + np.uint64(first_offset))


def device_batch(lines, lead=0, with_n_positions=True, first_offset=0):
    """a device batch whose bases begin `lead` bytes into an allocation (and whose offsets[0] is `first_offset`)"""
    import torch
    data = b"".join(lines)
    buf = torch.zeros(lead + first_offset + len(data) + 64, dtype=torch.uint8, device="cuda")
    if data:
        buf[lead + first_offset:lead + first_offset + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(x) for x in lines])
    d_offs = torch.from_numpy(offs + first_offset).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 256 == 0
    return api.ReadBatch(buf.data_ptr() + lead, d_offs.data_ptr(), n_reads=len(lines), on_device=True, keepalive=(buf, d_offs),
                         n_positions=stream_T(lines) if with_n_positions else None)


def as_text(lines, fastq, seed):
    """the lines as the sequence lines of FASTA / FASTQ records whose header lengths vary from 1 to 40 bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for ln in lines:
        assert b"\n" not in ln
        head = (b"@" if fastq else b">") + b"r" * int(rng.integers(0, 40))
        out.append(head + b"\n" + ln + b"\n" + (b"+\n" + b"I" * len(ln) + b"\n" if fastq else b""))
    return b"".join(out)


def text_batch(packer, lines, fastq, seed=1):
    text = as_text(lines, fastq, seed)
    rb, used = packer.text_split(text, fastq, True)
    assert used == len(text) and rb.n_reads == len(lines)
    return rb


# ---- 1. read lengths and the two look-up paths ------------------------------------------------------------------------------------------------
def test_the_mixed_batches_are_the_shapes_they_claim_to_be():
    """no device work: the wave boundaries of the launch rule fall where the comments of mixed() say"""
    for size, blocks, n_waves in ((12, 1, 4), (40, 2, 7), (70, 3, 12)):
        lines = mixed(size)
        T = stream_T(lines)
        got_blocks, starts = wave_starts(T)
        assert got_blocks == blocks and len(starts) == n_waves and abs(T - size * 1000) < 3500, (size, T, got_blocks, len(starts))
        at = [where(lines, s) for s in starts]
        if size == 12:
            assert starts == [0, 4096, 8192, 12288] and T > 12288                 # all four waves of the block have work
            assert at[1][0] == "in" and at[1][1] > 5000 and at[2][0] in ("in", "sep") and at[2][1] < 32 and at[3] == ("empties", 0)
        else:
            assert starts[:7] == [6144 * w for w in range(7)]
            assert at[1][0] == "in" and at[1][1] > 5000                           # inside a long read
            assert at[2][0] == "sep" and at[2][1] > 1000                          # on the separator behind a long read
            assert at[3] == ("empties", 0)                                        # inside a run of empty reads
            assert at[4][1] < 32 and at[6][1] < 32 and at[5] == ("in", 5000)      # among short reads; inside a long read
        assert sum(1 for x in lines if not x) >= 170 and sum(1 for x in lines if 0 < len(x) < 32) >= 200


@gpu
@pytest.mark.parametrize("size", [12, 40, 70])
def test_mixed_read_lengths_over_one_two_and_three_blocks(reader, packer, size):
    lines = mixed(size)
    pack_and_check(reader, packer, host_batch(lines), lines, f"mixed batch of {stream_T(lines)} positions")


# ---- 2. word edges ------------------------------------------------------------------------------------------------------------------------
def edge_lines(T, seed=3):
    """four reads of T positions in all: bad bytes inside (tokens reversed), shorter than any k, a filler that ends the stream, lower case"""
    rng = np.random.default_rng(seed)
    fixed = [b"ACGTTGCAGATTACAG" + b"NN" + b"CCGTATTGACCAGTA", b"ACG", b"acgtACGT"]
    filler = rng.choice(ACGT, T - 4 - sum(len(x) for x in fixed)).tobytes()
    lines = fixed[:2] + [filler] + fixed[2:]
    assert stream_T(lines) == T
    return lines


WORD_EDGES = {f"T = {T}": edge_lines(T) for T in (128, 129, 159, 160, 161, 191)}         # T % 64 = 0, 1, 31, 32, 33, 63
WORD_EDGES.update({
    "one empty read": [b""],                                                              # T = 1: nothing but a separator
    "one read of 1": [b"G"],
    "one read of 2048": [np.random.default_rng(8).choice(ACGT, 2048).tobytes()],          # a whole trip and one position
    "one read of 63": [b"ACGT" * 15 + b"ACG"],                                            # T = 64: the separator is bit 63, no tail
    "empty first and last reads": [b"", b"ACGTACGTAC", b"TTNGG", b""],
    "only empty reads": [b""] * 70,                                                       # T = 70: separators in two words
})


@gpu
@pytest.mark.parametrize("name", list(WORD_EDGES), ids=lambda s: s.replace(" ", "_"))
def test_word_edges(reader, packer, name):
    lines = WORD_EDGES[name]
    pack_and_check(reader, packer, host_batch(lines), lines, name)
    pack_and_check(reader, packer, device_batch(lines, lead=5, with_n_positions=False), lines, name + ", device batch")


# ---- 3. alignment ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def alignment_lines():
    """for every address mod 16 and every n from 1 to 32, a read of n bytes that starts at such an address and lies inside one half-word: one
    fetch of n bytes at that shift.  A filler read of 1 to 15 bytes in front of it moves the address, empty reads (a position each, no byte)
    move the place in the half-word.  In a contiguous batch (host, device) every pair (shift, n) occurs whatever the alignment of the bases
    themselves; in a text_split batch every read's address follows from its header instead, and only the shifts are known to be all there."""
    rng = np.random.default_rng(16)
    out, pos, byte = [], 0, 0

    def add(n):
        nonlocal pos, byte
        out.append(rng.choice(ACGT, n).tobytes())
        pos += n + 1
        byte += n

    for n in range(1, 33):
        for shift in range(16):
            if (shift - byte) % 16:
                add((shift - byte) % 16)
            while pos % 32 + n > 32:
                add(0)
            assert byte % 16 == shift and pos // 32 == (pos + n - 1) // 32
            add(n)
    out += [b"ACGTNACGT", b"", b"NNACGT" * 9, b"ACGT" * 40]
    return out


def fetches(lines, lead):
    """the (shift, shift + n) of every fetch k_pack makes: the part of a read inside one half-word, n bytes from an address that is `shift`
    bytes past a multiple of 16, for bases that begin `lead` bytes past one"""
    out, s, byte = set(), 0, lead
    for ln in lines:
        p = s
        while p < s + len(ln):
            n = min(s + len(ln), (p // 32 + 1) * 32) - p
            shift = (byte + p - s) % 16
            out.add((shift, shift + n))
            p += n
        s += len(ln) + 1
        byte += len(ln)
    return out


def test_the_alignment_batch_reaches_every_chunk_count_at_every_shift():
    """no device work.  shift + n = 16 and 17: one chunk and the first byte of a second; 32 and 33: two and the first byte of a third; 47: the
    most there is (shift 15, a whole half-word)"""
    want = {(sh, 16) for sh in range(16)} | {(sh, 17) for sh in range(16)} | {(sh, 32) for sh in range(16)} | {(sh, 33) for sh in range(1, 16)}
    want.add((15, 47))
    for lead in range(16):
        got = fetches(alignment_lines(), lead)
        assert want <= got, (lead, sorted(want - got))
        assert {(sh, sh + n) for sh in range(16) for n in range(1, 33)} <= got
    assert stream_T(alignment_lines()) < 30000


@gpu
@pytest.mark.parametrize("first_offset", [0, 1, 7, 8, 15] + [2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14])
def test_alignment_of_host_batches(reader, packer, first_offset):
    lines = alignment_lines()
    pack_and_check(reader, packer, host_batch(lines, first_offset), lines, f"host batch, offsets[0] = {first_offset}")


@gpu
@pytest.mark.parametrize("lead", range(16))
def test_alignment_of_device_batches(reader, packer, lead):
    """the tensor begins `lead` bytes into its allocation; with the total known to the caller and read back by the library; offsets[0] = 0 and 3"""
    lines = alignment_lines()
    for with_n_positions in (True, False):
        pack_and_check(reader, packer, device_batch(lines, lead, with_n_positions), lines, f"device batch {lead} bytes into its allocation")
    pack_and_check(reader, packer, device_batch(lines, lead, True, first_offset=3), lines, f"device batch {lead} bytes in, offsets[0] = 3")


@gpu
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_alignment_of_text_split_batches(reader, packer, fastq):
    """the reads lie inside raw text (fgpu_reads.starts) behind headers of 1 to 40 bytes, so a read's address no longer follows from the reads
    before it: every address mod 16 occurs (asserted), which fetch lengths meet which is left to the headers.  Three texts, one block"""
    lines = alignment_lines()
    for seed in (1, 2, 3):
        assert len({(len(h) + 1) % 16 for h in as_text(lines, fastq, seed).split(b"\n")[::4 if fastq else 2]}) == 16
        pack_and_check(reader, packer, text_batch(packer, lines, fastq, seed), lines, f"text_split batch, headers of seed {seed}")
    small = WORD_EDGES["empty first and last reads"]
    pack_and_check(reader, packer, text_batch(packer, small, fastq), small, "text_split batch with empty lines")


# ---- 4. byte values -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def byte_value_lines():
    """every byte value at every place of the 8 bytes k_pack converts at a time, between 0x00 and 0xFF and between good bytes; reads of one
    value only (one token: nothing for k_pack_fix to move, the planes are k_pack's own verdict unless it flags the read)"""
    out = []
    for g in range(8):
        lead = b"ACGTACGT"[:g]
        out.append(lead + b"".join(bytes([v, 0x00, 0xFF]) for v in range(256)))
        out.append(lead + b"".join(bytes([0xFF, v, 0x00]) for v in range(256)))
        out.append(lead + b"".join(bytes([v]) + b"ACGTACG"[:3 + v % 4] for v in range(256)))
    for v in range(256):
        out.append(bytes([v]) * (8 + v % 9))
    # the near misses by name: one bit from A C G T, their lower case, the neighbours in the alphabet, the high bit
    out.append(b"@BSUEFHVacgtNn" + bytes([0xC1, 0xC3, 0xC7, 0xD4, 0x01, 0x03, 0x07, 0x14]) + b"ACGT")
    return out


def test_the_byte_value_batch_puts_every_value_in_every_lane():
    """no device work: lane = place of the byte among the 8 converted together = its distance from the start of its fetch, mod 8"""
    lines = byte_value_lines()
    seen, s = set(), 0
    for ln in lines:
        for q, c in enumerate(ln):
            p = s + q
            seen.add((c, (p - max(s, p // 32 * 32)) % 8))
        s += len(ln) + 1
    assert len(seen) == 256 * 8
    assert stream_T(lines) < 70000


@gpu
def test_byte_values(reader, packer):
    lines = byte_value_lines()
    pack_and_check(reader, packer, host_batch(lines), lines, "byte values, host batch")
    pack_and_check(reader, packer, device_batch(lines, lead=11), lines, "byte values, device batch")


# ---- 5. token reversal --------------------------------------------------------------------------------------------------------------------
def scattered(n, seed, every):
    rng = np.random.default_rng(seed)
    r = rng.choice(ACGT, n)
    r[rng.integers(0, n, n // every)] = ord("N")
    return r.tobytes()


REVERSALS = {
    # three flagged reads in stream word 0 (positions 0-3, 4-8, 9-12), a fourth across words 0 and 1 of the codes: k_pack_fix's threads
    # update the same words at the same time
    "neighbours in one word": [b"ANC", b"GNNT", b"CNA", b"ACGTACGTACGTACGTANNACGTACGTTTT", b"TN", b"NT"],
    "bad bytes only at the start": [b"NNN" + b"ACGTTGCA" * 6, b"ACGT"],
    "bad bytes only at the end": [b"ACGTTGCA" * 6 + b"NNN", b"ACGT"],
    "bad bytes everywhere": [b"N" * 40, b"n" * 70, b"ACGT"],
    "single good and bad bytes in turn": [b"ANCNGNTN" * 10 + b"A", b"NANCNGNT" * 9],                 # 81 and 72 positions
    # a token of 41 good bytes that lies at positions 30-70 once reversed: over the 32- and the 64-position edge
    "a token across word edges": [b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTA" + b"N" + b"C" * 29, b"GG"],
    "a long read with scattered bad bytes": [b"ACGT", scattered(5000, 4, 50), b"", scattered(3000, 5, 400), b"TTTT"],
}


@gpu
@pytest.mark.parametrize("name", list(REVERSALS), ids=lambda s: s.replace(" ", "_"))
def test_token_reversal(reader, packer, name):
    lines = REVERSALS[name]
    if name == "a token across word edges":
        code, bad = P.stream(lines)
        assert bad[29] == 1 and not any(bad[30:71]) and bad[71] == 1
    pack_and_check(reader, packer, host_batch(lines), lines, name)
    pack_and_check(reader, packer, device_batch(lines, lead=9), lines, name + ", device batch")
    pack_and_check(reader, packer, text_batch(packer, lines, False), lines, name + ", text_split batch")


# ---- 6. the other producer: a pass 0 that keeps what it packs ---------------------------------------------------------------------------------
@gpu
def test_kept_blocks_of_pass_0_are_the_restatements(reader):
    batches = [WORD_EDGES["T = 129"], mixed(12), WORD_EDGES["T = 128"], REVERSALS["a long read with scattered bad bytes"]]
    ctx = api.Context(21, 128, 1)
    ctx.estimate_begin(14)
    ctx.estimate_keep(1 << 62)
    for lines in batches:
        ctx.estimate_batch(host_batch(lines))
    ctx.estimate_end()
    blocks = ctx.estimate_take_kept()
    assert len(blocks) == len(batches)
    for lines, pk in zip(batches, blocks):
        assert (pk.T, pk.n_reads, pk.nbytes) == (stream_T(lines), len(lines), P.nbytes_of(stream_T(lines)))
        assert_block(reader.read(ctx, pk.block_dev, pk.nbytes), lines, "kept block")
        assert ctx.lib.fgpu_device_free(ctx.h, pk.block_dev) == 0
    ctx.close()


# ---- 7. the consumers see only the format: blocks built on the host ------------------------------------------------------------------------------
CONSUMER_EDGES = {"T % 64 = 0": 0, "T % 64 = 1": 1}


def consumer_edge_lines(rest):
    """the reads of edge_lines() with one read three times, so that k-mers reach bloo2: T = 256 + rest"""
    lines = edge_lines(256 + rest - 3 * 41)
    return lines[:2] + [b"GATTACAGGCTTAACCGGTTACGATCGATCGGATCGATTA"] * 3 + lines[2:]


@functools.lru_cache(maxsize=None)
def consumer_case(name):
    """(lines, k, tai, n_hash) and per mercy flag the oracle's (bloo1, bloo2, stats, junction keys, junction records)"""
    if name == "ragged_k31":
        c = Case(name)
        lines, k = c.lines(), c.k
        tai, nh = api.load_filter_shape(c.E, c.S, c.fp)
        assert any(b"N" in ln.strip(b"N") for ln in lines)
    else:
        lines, k, tai, nh = (mixed(12) if name == "mixed" else consumer_edge_lines(CONSUMER_EDGES[name])), 15, 1 << 16, 2
        assert name == "mixed" or stream_T(lines) % 64 == CONSUMER_EDGES[name]
    bases, offs = po.reads_from_lines(lines)
    want = {}
    for mercy in (False, True):
        b1, b2, lst, osc = oracle_run((bases, offs), k, tai, nh, mercy=mercy)
        keys, recs = osc.junctions("creation")
        want[mercy] = (b1.bits().copy(), b2.bits().copy(),
                       {"reads_processed": lst.reads_processed, "unambiguous_reads": lst.unambiguous_reads, "kmers": lst.kmers, "to_bloo2": lst.to_bloo2},
                       keys, recs)
    assert want[False][2]["to_bloo2"] > 0
    return tuple(lines), k, tai, nh, want


def upload(ctx, dst, words):
    """host words into device memory at dst, through a tensor and the context's stream"""
    import torch
    t = torch.from_numpy(words.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    assert ctx.lib.fgpu_device_copy(ctx.h, dst, t.data_ptr(), words.nbytes) == 0
    ctx.synchronize()


def assert_the_oracles(ctx, st, lines, want):
    b1, b2, stats, okeys, orecs = want
    assert st == stats
    assert np.array_equal(ctx.bloom_download(L.BLOO1), b1), "bloo1 differs from the oracle's"
    assert np.array_equal(ctx.bloom_download(L.BLOO2), b2), "bloo2 differs from the oracle's"
    sc = api.ReadScanner(ctx)
    sc.scanReads([host_batch(list(lines))])
    keys, recs = sc.junctions()
    assert np.array_equal(keys, okeys) and np.array_equal(recs["dist"], orecs["dist"]) and np.array_equal(recs["cov"], orecs["cov"])


@gpu
@pytest.mark.parametrize("mercy", [False, True], ids=["plain", "mercy"])
@pytest.mark.parametrize("name", ["mixed", "T % 64 = 0", "T % 64 = 1", "ragged_k31"], ids=lambda s: s.replace(" ", "_"))
def test_host_built_blocks_load_to_the_oracles_filters(name, mercy):
    lines, k, tai, nh, want = consumer_case(name)
    block = want_block(lines)
    T, n = stream_T(lines), len(lines)
    # into a block a sliced pass expects: its digest is recomputed and compared with the restatement's
    ctx = api.Context(k, tai, nh, mercy=mercy)
    (ctx.load_slice_mercy_begin if mercy else ctx.load_slice_begin)(0, tai)
    pk = ctx.load_slice_expect(T, n)
    assert pk.nbytes == block.nbytes
    upload(ctx, pk.block_dev, block)
    ctx.load_slice_batch_packed(pk)
    if mercy:
        ctx.load_slice_mercy_probe()
    ctx.load_slice_commit()
    assert_the_oracles(ctx, ctx.load_slice_end(), lines, want[mercy])
    ctx.close()
    # into an allocation of the caller's that a plain pass adopts
    ctx = api.Context(k, tai, nh, mercy=mercy)
    p = C.c_void_p()
    assert ctx.lib.fgpu_device_alloc(ctx.h, block.nbytes, C.byref(p)) == 0
    upload(ctx, p.value, block)
    ctx.load_begin()
    ctx.load_batch_packed(L.Packed(p.value, block.nbytes, T, n))
    assert_the_oracles(ctx, ctx.load_end(), lines, want[mercy])
    ctx.close()


@gpu
def test_a_changed_padding_word_under_an_unchanged_trailer_is_refused():
    lines, k, tai, nh, want = consumer_case("T % 64 = 0")
    plane = P.n_words_of(stream_T(lines)) + P.PADW
    for at, value in ((2 * plane - 1, 1), (3 * plane - 1, P.GOLDEN)):          # the last padding word of the codes, of the bad plane
        block = want_block(lines).copy()
        assert int(block[at]) in (0, 0xFFFFFFFFFFFFFFFF)
        block[at] = value
        ctx = api.Context(k, tai, nh)
        ctx.load_slice_begin(0, tai)
        pk = ctx.load_slice_expect(stream_T(lines), len(lines))
        upload(ctx, pk.block_dev, block)
        ctx.load_slice_batch_packed(pk)
        ctx.load_slice_commit()
        st = L.LoadStats()
        assert ctx.lib.fgpu_load_slice_end(ctx.h, C.byref(st)) == L.ERR_ARG and b"trailer" in ctx.lib.fgpu_last_error(ctx.h)
        ctx.close()
