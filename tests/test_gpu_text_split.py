"""fgpu_text_split (faucet_amd/csrc/text.hip) against the restatement of the reference's reading loop (tests/getline_ref.py, pinned to the
compiled reference by tests/golden/make_input_golden.py): the number of reads, every read's start and length, and the bytes consumed, read
back from the device -- nothing goes through a filter.  Final and non-final chunks of malformed text, every prefix of them, the word edges
of the newline plane, buffers that still hold an earlier chunk, text that is on the device already, more than one block and scan tile, the
second round of the grid-stride loops; and the command line on the golden cases of tests/golden/input_side/.  Needs an MI355X."""
import functools
import os
import subprocess

import numpy as np
import pytest

from faucet_amd import api
from tests import getline_ref as G
from tests.test_gpu_vs_reference_fuzz import EXE, REF_BIN, cli_against_reference
from tests.test_input_side_cpu import CASES, HAND_WRITTEN, case, counter_lines, golden_files

gpu = pytest.mark.gpu          # the tests that cut text on the device; the checks of the expectations themselves run anywhere


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(21, 1 << 12, 2)
    c.text_reserve(16384)
    yield c
    c.close()


def read_back(ctx, rb):
    """(starts, offsets) of a text_split batch on the host: copied on the context's stream into a buffer of torch's, as n_reads and
    2 * n_reads + 1 words of 64 bits"""
    import torch
    n = rb.n_reads
    if n == 0:
        return np.zeros(0, np.uint64), np.zeros(1, np.uint64)
    buf = torch.empty(2 * n + 1, dtype=torch.int64, device="cuda")
    assert ctx.lib.fgpu_device_copy(ctx.h, buf.data_ptr(), rb.starts_ptr, 8 * n) == 0
    assert ctx.lib.fgpu_device_copy(ctx.h, buf.data_ptr() + 8 * n, rb.offsets_ptr, 8 * (n + 1)) == 0
    ctx.synchronize()
    host = buf.cpu().numpy().view(np.uint64)
    return host[:n], host[n:]


def split(ctx, text, fastq, final, **kw):
    """one call: (read ranges [(start, end)], consumed) as the device has them"""
    rb, used = ctx.text_split(text, fastq, final, **kw)
    starts, offs = read_back(ctx, rb)
    if rb.n_reads:
        assert offs[0] == 0
    lens = np.diff(offs)
    return [(int(s), int(s + n)) for s, n in zip(starts, lens)], used


def check(ctx, text, fastq, final, what=""):
    got = split(ctx, text, fastq, final)
    want = G.chunk(text, fastq, final)
    assert got == want, (what, fastq, final, len(text), text[-80:], got[1], want[1], [x for x in zip(got[0], want[0]) if x[0] != x[1]][:3])


# ---- golden texts and small hand-written ones: whole, and every prefix ------------------------------------------------------------------------
def distinct_texts():
    """(name, text, fastq) of every golden text (the paired-end cases read the same text as the single-end ones) and of the hand-written
    ones as FASTA and as FASTQ, in a fixed order"""
    out = [(n[:-3], case(n).reads_text(), case(n).fastq) for n in CASES if n.endswith("_se")]
    return out + [(f"hand{i}_{'fq' if fastq else 'fa'}", t, fastq) for i, t in enumerate(HAND_WRITTEN) for fastq in (False, True)]


@functools.lru_cache(maxsize=None)
def own_prefix_lengths():
    """name -> the lengths of those prefixes of the text that are not prefixes of a text of the same kind earlier in distinct_texts():
    the golden texts share their first records, and a prefix is cut once (a function of the list alone, not of what ran before)"""
    out = {}
    texts = distinct_texts()
    for i, (name, text, fastq) in enumerate(texts):
        earlier = [other for _, other, fq in texts[:i] if fq == fastq]
        common = 0                                           # the longest prefix shared with an earlier text
        for other in earlier:
            n = min(len(text), len(other))
            neq = np.flatnonzero(np.frombuffer(text[:n], np.uint8) != np.frombuffer(other[:n], np.uint8))
            common = max(common, int(neq[0]) if neq.size else n)
        out[name] = list(range(common + 1 if earlier else 0, len(text) + 1))
    return out


TEXT_NAMES = [n for n, _, _ in distinct_texts()]


def test_every_prefix_of_every_text_is_cut_by_some_case():
    """no device work: between them the cases below cut every prefix of every text"""
    own = own_prefix_lengths()
    cut = {(fastq, text[:n]) for name, text, fastq in distinct_texts() for n in own[name]}
    for name, text, fastq in distinct_texts():
        assert all((fastq, text[:n]) in cut for n in range(len(text) + 1)), name
    assert sum(len(v) for v in own.values()) < 40_000


@gpu
@pytest.mark.parametrize("final", [False, True], ids=["not_final", "final"])
@pytest.mark.parametrize("name", TEXT_NAMES)
def test_whole_texts_and_every_prefix_follow_the_restatement(ctx, name, final):
    text, fastq = next((t, f) for n, t, f in distinct_texts() if n == name)
    check(ctx, text, fastq, final, name)
    for n in own_prefix_lengths()[name]:
        check(ctx, text[:n], fastq, final, f"{name}[:{n}]")


# ---- the word edges of the newline plane -----------------------------------------------------------------------------------------------------
def edge_texts():
    out = []
    for n in (1, 63, 64, 65, 127, 128, 129):
        body = (b"ACGTTGCA" * 20)[:n]
        edges = [p for p in (0, 62, 63, 64, 65, n - 1) if p < n]
        for p in edges:                                  # one newline, at an edge
            out.append(body[:p] + b"\n" + body[p + 1:])
        every = bytearray(body)
        for p in edges:                                  # all of them: records that begin and end on both sides of a word's edge
            every[p] = 10
        out.append(bytes(every))
        out.append(b"\n" * n)                            # nothing but newlines: whole words of them from 64 on
        if n >= 128:
            out.append(body[:64] + b"\n" * 64 + body[128:])      # a word of 64 newlines between words without one
            out.append(b"\n" * 64 + body[64:])
        for step in (3, 5, 31, 33):                      # lines of step - 1 bytes: records that straddle words, at every phase
            out.append(bytes(10 if i % step == step - 1 else c for i, c in enumerate(body)))
    return out


@gpu
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_word_edges_of_the_newline_plane(ctx, fastq):
    for text in edge_texts():
        for final in (False, True):
            check(ctx, text, fastq, final)


# ---- buffers that hold an earlier chunk ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("reserve", [0, 16384, 1000], ids=["no_reserve", "reserve_for_all", "reserve_below_a_later_chunk"])
def test_a_short_chunk_in_buffers_that_held_newlines(reserve):
    """The three sets of buffers are used in turn: the fourth chunk lands where the first was.  The first is several KB of newlines, the
    fourth is short and ends inside a word, so the bytes behind it -- in the text buffer and in the newline plane -- are old newlines;
    then a chunk larger than anything before (the buffers grow under the batches), and short ones again in every set."""
    c = api.Context(21, 1 << 12, 2)
    try:
        if reserve:
            c.text_reserve(reserve)
        fa, fq = case("fa_wellformed_se").reads_text(), case("fq_header_unterminated_se").reads_text()
        short = [b"ACGT\nACGTACGTAC\nTTGCA\nAC", b"h\nAC", b"ACGTA\n\nGG\nTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT"]
        chunks = [b"\n" * 6001, fa, fq, short[0], short[1], short[2], b"\n" * 9000 + fa, short[0], short[2], short[1], short[0]]
        assert all(len(s) % 64 for s in short)
        for i, text in enumerate(chunks):
            for fastq in (False, True):                   # (two calls per chunk: a chunk meets both other sets' leftovers too)
                for final in (False, True):
                    check(c, text, fastq, final, f"chunk {i}")
    finally:
        c.close()


@gpu
def test_a_short_chunk_three_calls_after_a_chunk_of_newlines():
    """the same with exactly one call per chunk, so that the short chunk IS in the set the newlines were in"""
    for final in (False, True):
        c = api.Context(21, 1 << 12, 2)
        try:
            for text in (b"\n" * 6001, b"h\nACGT\n", b"h\nAC\nh2\nGT\n", b"ACGT\nACGTACGTAC\nTTGCA\nAC", b"h\nAC", b"\n", b"x"):
                check(c, text, False, final)
        finally:
            c.close()


# ---- text that is on the device already -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_text_on_the_device_at_every_address_mod_16(ctx, fastq):
    """The text lies inside a larger device buffer whose every other byte is a newline: a byte read in front of the text or behind nbytes
    changes the counts.  The batch points into the caller's buffer, and says what the call on host text says."""
    import torch
    texts = [case("fq_header_unterminated_se" if fastq else "fa_header_unterminated_se").reads_text()[-700:],
             case("fq_ends_inside_quality_se" if fastq else "fa_sequence_unterminated_se").reads_text()[:333],
             b"ACGT\nACGTACGTAC\nTTGCA\nAC\n", b"x", b"\n", b"ACGTACGTACGTACGTACGTA" * 4]
    for text in texts:
        for lead in range(256, 272):
            buf = torch.full((lead + len(text) + 300,), 10, dtype=torch.uint8, device="cuda")
            buf[lead:lead + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            assert buf.data_ptr() % 256 == 0
            for final in (False, True):
                rb, used = ctx.text_split(buf.data_ptr() + lead, fastq, final, text_on_device=True, nbytes=len(text))
                assert rb.n_reads == 0 or rb.bases_ptr == buf.data_ptr() + lead
                starts, offs = read_back(ctx, rb)
                got = ([(int(s), int(s + n)) for s, n in zip(starts, np.diff(offs))], used)
                assert got == G.chunk(text, fastq, final) == split(ctx, text, fastq, final), (lead, final, text[-40:])
            assert bytes(buf.cpu().numpy()) == b"\n" * lead + text + b"\n" * 300            # the call only reads


# ---- large texts: the expectation from the newline positions, with numpy --------------------------------------------------------------------
def numpy_chunk(text: np.ndarray, fastq, final):
    """(starts, lengths, consumed) of the reading loop on a chunk, from the positions of its newlines alone"""
    n, P = len(text), 4 if fastq else 2
    nl = np.flatnonzero(text == 10).astype(np.int64)
    open_tail = n > 0 and text[-1] != 10
    line_start = np.concatenate([[0], nl + 1])            # line i begins here; the last entry: the tail without a newline (or n)
    line_end = np.concatenate([nl, [n]])
    if final:
        n_lines = len(nl) + (1 if open_tail else 0)
        n_rec, consumed = -(-n_lines // P), n
    else:
        n_lines = len(nl)
        n_rec = n_lines // P
        consumed = int(nl[n_rec * P - 1]) + 1 if n_rec else 0
    at = np.arange(n_rec, dtype=np.int64) * P + 1                        # the read is line 1 of its record
    there = at < n_lines
    at = np.minimum(at, len(line_start) - 1)
    starts, ends = np.where(there, line_start[at], n), np.where(there, line_end[at], n)
    if final and open_tail and n_lines % P == 1:                         # the last line is a header cut off by the end of the file: it is the read
        starts[-1], ends[-1] = line_start[n_lines - 1], n
    return starts.astype(np.uint64), (ends - starts).astype(np.uint64), consumed


def check_numpy(ctx, text: np.ndarray, fastq, final):
    rb, used = ctx.text_split(text.tobytes(), fastq, final)
    starts, offs = read_back(ctx, rb)
    want_starts, want_lens, want_used = numpy_chunk(text, fastq, final)
    assert rb.n_reads == len(want_starts) and used == want_used, (fastq, final, rb.n_reads, len(want_starts), used, want_used)
    assert np.array_equal(starts, want_starts), int(np.flatnonzero(starts != want_starts)[0])
    assert np.array_equal(np.diff(offs), want_lens) and offs[0] == 0, int(np.flatnonzero(np.diff(offs) != want_lens)[0])


def test_numpy_expectation_is_the_restatement():
    """no device work: on the golden texts and their prefixes both expectations say the same"""
    for name, text, fastq in distinct_texts():
        for n in sorted({len(text), len(text) - 1, len(text) // 2, len(text) // 3, 1, 0} - {-1}):
            for final in (False, True):
                s, ln, used = numpy_chunk(np.frombuffer(text[:n], np.uint8), fastq, final)
                want, want_used = G.chunk(text[:n], fastq, final)
                assert [(int(a), int(a + b)) for a, b in zip(s, ln)] == want and used == want_used, (name, n, final)


@gpu
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_more_than_one_block_and_scan_tile(fastq):
    """a few hundred KB: line lengths 0 to 300, a third of the lines empty, runs of empty lines longer than a word; 5 000 words of the
    newline plane (20 blocks), tens of thousands of records"""
    rng = np.random.default_rng(17 + fastq)
    lens = rng.integers(0, 301, 4000)
    lens[rng.random(4000) < 0.33] = 0
    lens[1000:1200] = 0
    lens[-1] = 77
    text = np.full(int(lens.sum()) + len(lens), ord("A"), np.uint8)
    text[np.cumsum(lens + 1) - 1] = 10
    assert 300_000 < len(text) < 500_000
    c = api.Context(21, 1 << 12, 2)
    try:
        for final in (False, True):
            check_numpy(c, text, fastq, final)
            check_numpy(c, text[:-1], fastq, final)                     # the last line without its newline
            got = split(c, text[:-1].tobytes(), fastq, final)
            assert got == G.chunk(text[:-1].tobytes(), fastq, final)
        for cut in (3, 40, 78, 79):                                     # an open last line that is a header / a read / a FASTQ tail line
            check_numpy(c, text[:-cut], fastq, True)
    finally:
        c.close()


@gpu
def test_the_second_round_of_the_grid_stride_loops():
    """Just over 64 MiB: more words of the newline plane than 4096 blocks of 256 lanes take in one round, which is what every full-size
    chunk of the command line is once a tail is carried in front of it.  A pattern of about 1 KB, tiled."""
    rng = np.random.default_rng(5)
    lens = np.concatenate([rng.integers(0, 120, 17), [0, 0, 1]])
    pattern = np.full(int(lens.sum()) + len(lens), ord("C"), np.uint8)
    pattern[np.cumsum(lens + 1) - 1] = 10
    assert 800 < len(pattern) < 1300
    size = (64 << 20) + 1000
    text = np.resize(pattern, size)
    assert (size + 63) // 64 > 4096 * 256 and text[-1] != 10
    c = api.Context(21, 1 << 12, 2)
    try:
        check_numpy(c, text, False, False)
        check_numpy(c, text, True, True)
        nl = np.flatnonzero(text == 10)
        m = len(nl) - len(nl) % 2                                        # an even number of lines, then three bytes of a header cut off: the read
        cut_off = text[:int(nl[m - 1]) + 4].copy()
        cut_off[-3:] = ord("C")
        assert (len(cut_off) + 63) // 64 > 4096 * 256
        check_numpy(c, cut_off, False, True)
        assert split(c, cut_off[-5000:].tobytes(), False, True)[0][-1] == (4997, 5000)
    finally:
        c.close()


# ---- through the product ----------------------------------------------------------------------------------------------------------------------
CLI_FEEDS = {"default": [], "chunk_mb_1": ["-chunk_mb", "1"], "batch_reads_3": ["-batch_reads", "3"], "gpus_3": ["-gpus", "3"]}


@gpu
@pytest.mark.parametrize("name", CASES)
def test_command_line_writes_the_golden_by_every_feed(name, tmp_path):
    c = case(name)
    inp = str(tmp_path / ("reads.fq" if c.fastq else "reads.fa"))
    with open(inp, "wb") as f:
        f.write(c.reads_text())
    want = golden_files(c)
    for feed, extra in CLI_FEEDS.items():
        d = tmp_path / feed
        d.mkdir()
        if feed == "default" and os.path.exists(REF_BIN):            # the reference itself travelled: every file and the log line for line, too
            _, stdout = cli_against_reference(inp, c.meta["args"], d)
            prefix = str(d / "gpu" / "out")
        else:
            prefix = str(d / "out")
            r = subprocess.run(["stdbuf", "-o0", EXE, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", prefix] + c.meta["args"] + extra,
                               capture_output=True, text=True, errors="replace", timeout=600)
            assert r.returncode == 0, (feed, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
            stdout = r.stdout
        assert counter_lines(stdout) == c.meta["counter_lines"], feed
        for ext, data in want.items():
            with open(prefix + "." + ext, "rb") as f:
                assert f.read() == data, (feed, ext)
