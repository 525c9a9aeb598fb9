"""The input side without a GPU: which bytes of a file are reads at all.

The expectation is the reference's reading loop restated as a stream simulation (tests/getline_ref.py), which tests/golden/make_input_golden.py
pinned to the COMPILED REFERENCE on malformed FASTA / FASTQ text (tests/golden/input_side/: no final newline, a last header with and without
its newline, cut sequence, '+' and quality lines, blank lines that shift every line's role, CRLF, a single line, a lone newline).  Held to it:
  * the restatement itself, again, where the reference binary is at hand;
  * the command line linked with the CPU stand-in of the C ABI (tests/stub/faucet_gpu_stub.cpp), by its three feeds -- device-shaped chunks,
    host getline batches, read shards -- against the golden's files and counter lines;
  * faucet_amd/host/text_source.h alone (tests/host/text_source_check.cpp): TextSource at chunk sizes from one byte up, over the whole file
    and over the shards' byte ranges, record_cuts, ReadSource -- built plain, under address + undefined-behaviour and under the thread sanitizer."""
import functools
import gzip
import os
import shutil
import subprocess

import pytest

from tests import getline_ref as G
from tests.golden_util import GOLDEN, Case
from tests.test_host_sanitizers import REF_BIN, ROOT, SOURCES

INPUT_SIDE = os.path.join(GOLDEN, "input_side")
CASES = sorted(os.listdir(INPUT_SIDE))
COUNTER_LINES = ("Reads processed:", "Unambiguous reads:", "Weights after load:", "Distinct junctions:", "Empty count:")
FEEDS = {"default": [], "batch_reads_3": ["-batch_reads", "3"], "gpus_3": ["-gpus", "3"]}

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(os.path.join(INPUT_SIDE, name))


def counter_lines(stdout):
    """the counter lines as printed, in order (the scan's progress line ends without a newline: "Empty count" follows it on the same line)"""
    out = []
    for ln in stdout.replace("\r", "\n").splitlines():
        at = [ln.find(p) for p in COUNTER_LINES if p in ln]
        if at:
            out.append(ln[min(at):].strip())
    return out


def golden_files(c):
    with gzip.open(os.path.join(c.dir, "out.bloom.gz"), "rb") as f, gzip.open(os.path.join(c.dir, "out.junctions.gz"), "rb") as g:
        return {"bloom": f.read(), "junctions": g.read()}


def run_and_compare(exe, c, tmp_path, extra, env=None, reads_text=None):
    """`exe` on the case's text (or on `reads_text` as FASTA): the golden's .bloom and .junctions byte for byte, and its counter lines"""
    fastq = c.fastq and reads_text is None
    inp = str(tmp_path / ("reads.fq" if fastq else "reads.fa"))
    with open(inp, "wb") as f:
        f.write(c.reads_text() if reads_text is None else reads_text)
    args = c.meta["args"] if reads_text is None else [a for a in c.meta["args"] if a != "--fastq"]
    prefix = str(tmp_path / "out")
    r = subprocess.run(["stdbuf", "-o0", exe, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", prefix] + args + list(extra),
                       capture_output=True, text=True, errors="replace", timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert counter_lines(r.stdout) == c.meta["counter_lines"]
    for ext, want in golden_files(c).items():
        with open(prefix + "." + ext, "rb") as f:
            assert f.read() == want, ext
    return r


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def test_the_golden_holds_the_cases_it_was_made_for():
    names = {n[3:-3] for n in CASES}
    for kind in ("fa", "fq"):
        for name in ("wellformed", "no_final_newline", "header_unterminated", "header_terminated", "sequence_unterminated", "blank_front",
                     "blank_middle", "blank_end", "crlf", "single_line", "newline_alone"):
            for ends in ("se", "pe"):
                assert f"{kind}_{name}_{ends}" in CASES
    assert {"ends_in_plus", "ends_in_plus_newline", "ends_inside_quality"} <= names
    assert any(case(n).counters["load_reads_processed"] % 2 for n in CASES)
    assert sum(os.path.getsize(os.path.join(INPUT_SIDE, n, f)) for n in CASES for f in os.listdir(os.path.join(INPUT_SIDE, n))) < 150_000


@pytest.mark.parametrize("name", CASES)
def test_restatement_counts_the_reads_the_reference_counted(name):
    c = case(name)
    text = c.reads_text()
    reads = G.reads(text, c.fastq)
    assert len(reads) == c.counters["load_reads_processed"] == c.counters["scan_reads_processed"]
    assert all(text[a:b] == r and b"\n" not in r for (a, b), r in zip(G.records(text, c.fastq), reads))
    assert G.chunk(text, c.fastq, True) == (G.records(text, c.fastq), len(text))
    if "eof_header" in c.meta["tags"]:              # the last line, a header without its newline, is the last read
        assert reads[-1] and text.endswith(reads[-1]) and not text.endswith(b"\n") and text.count(b"\n") % (4 if c.fastq else 2) == 0
    if name[3:-3] == "header_terminated":
        assert reads[-1] == b"" and text.endswith(b"\n")


def test_restatement_of_a_chunk_that_is_not_the_last():
    fa = b"h1\nAC\nh2\nGT\nh3"
    assert G.chunk(fa, False, False) == ([(3, 5), (9, 11)], 12) and G.consumed(fa[:11], False) == 6 and G.consumed(fa[:5], False) == 0
    assert G.chunk(fa[:5], False, False) == ([], 0) and G.chunk(b"", False, False) == ([], 0) and G.chunk(b"", False, True) == ([], 0)
    assert G.records(fa, False) == [(3, 5), (9, 11), (12, 14)]                 # "h3": the header is the read
    assert G.records(fa + b"\n", False) == [(3, 5), (9, 11), (15, 15)]         # with its newline: an empty read at the end of the text
    fq = b"h\nACGT\n+\nIIII\nh2\nAC\n+\nII"
    assert G.chunk(fq, True, False) == ([(2, 6)], 14) and G.records(fq, True) == [(2, 6), (17, 19)]
    assert G.records(b"\n", False) == [(1, 1)] and G.records(b"x", True) == [(0, 1)] and G.records(b"\n\nx", False) == [(1, 1), (2, 3)]


def test_restatement_of_the_cuts():
    text = b"a\nbb\nccc\ndddd\ne\nff\n"                  # lines start at 0 2 5 9 14 16; 19 bytes
    assert G.cuts(text, 2, 1, 1) == [0, 19]
    assert G.cuts(text, 2, 1, 2) == [0, 14, 19]           # nominal 9 starts line 3: odd, so on to line 4
    assert G.cuts(text, 2, 1, 3) == [0, 14, 14, 19]       # nominals 6, 12
    assert G.cuts(text, 2, 2, 2) == [0, 14, 19] and G.cuts(text, 4, 1, 2) == [0, 14, 19]
    assert G.cuts(text, 2, 2, 4) == [0, 14, 14, 14, 19]   # nominals 4, 9, 14: line 4 starts at 14
    assert G.cuts(text, 2, 2, 5) == [0, 14, 14, 14, 19, 19]      # nominals 3, 7, 11, 15: behind 14 no line's index is a multiple of 4
    assert G.cuts(text[:-1], 2, 1, 9)[-1] == 18 and G.cuts(b"", 2, 1, 3) == [0, 0, 0, 0] and G.cuts(b"x", 2, 1, 3) == [0, 0, 0, 1]


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/faucet_ref is built where the reference tree is at hand (make -C oracle ref)")
@pytest.mark.parametrize("name", CASES)
def test_reference_on_the_normalised_file_writes_the_golden(name, tmp_path):
    """every read of the restatement as a FASTA record of its own: the compiled reference makes of it what it made of the text itself"""
    c = case(name)
    run_and_compare(REF_BIN, c, tmp_path, [], reads_text=b"".join(b">\n" + r + b"\n" for r in G.reads(c.reads_text(), c.fastq)))


# ---- the command line on the CPU stand-in ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("input_side") / "faucet_stub")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *SOURCES, "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@needs_gxx
@pytest.mark.parametrize("feed", list(FEEDS))
@pytest.mark.parametrize("name", CASES)
def test_command_line_on_the_stand_in_writes_the_golden(cli, name, feed, tmp_path):
    run_and_compare(cli, case(name), tmp_path, FEEDS[feed], env={k: v for k, v in os.environ.items() if k != "FAUCET_SHARD_PROTOCOL"})


# ---- text_source.h alone -------------------------------------------------------------------------------------------------------------------------
HAND_WRITTEN = [b"", b"\n", b"\n\n", b"ACGT", b"h\nAC", b"h\nAC\n", b"h\nAC\nh2", b"h\nAC\nh2\n", b"h\n\nh\n\n", b"\n\n\nAC\n\n",
                b"h\nACGT\n+\nIIII\nh2\nAC\n+\nII", b"h\nACGT\n+\nIIII\nh2", b"h\r\nAC\r\nh2\r\nGT", b"x" * 300 + b"\ny\n" + b"z" * 200]


def check_texts():
    """every golden text once (the paired-end cases read the same text), and small hand-written ones as FASTA and as FASTQ"""
    out = [(n, case(n).reads_text(), case(n).fastq) for n in CASES if n.endswith("_se")]
    return out + [(f"hand{i}_{'fq' if fastq else 'fa'}", t, fastq) for i, t in enumerate(HAND_WRITTEN) for fastq in (False, True)]


def parse_check_output(stdout):
    """-> (cuts {(group, n): offsets}, feeds [(kind, key, reads, batches, bytes)]) from the program's output"""
    cuts, feeds, cur = {}, [], None
    lines = stdout.split("\n")
    assert lines[-2:] == ["ok", ""], lines[-3:]
    for ln in lines[:-2]:
        w = ln.split(" ")
        if w[0] == "cuts":
            cuts[(int(w[1]), int(w[2]))] = [int(x) for x in w[3:]]
        elif w[0] in ("source", "getline"):
            assert cur is None
            cur = [w[0], tuple(w[1:]), []]
        elif w[0] == "read":
            cur[2].append(b"" if w[1] == "-" else bytes.fromhex(w[1]))
        else:
            assert w[0] == "batches", ln
            feeds.append((cur[0], cur[1], cur[2], int(w[1]), int(w[2])))
            cur = None
    assert cur is None
    return cuts, feeds


@needs_gxx
@pytest.mark.parametrize("sanitizer", ["none", "address,undefined", "thread"])
def test_text_source_record_cuts_and_read_source_follow_the_restatement(sanitizer, tmp_path):
    exe = str(tmp_path / "text_source_check")
    flags = ["-O1"] if sanitizer == "none" else ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizer]
    r = subprocess.run(["g++", "-std=c++11", *flags, "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "faucet_amd", "host"),
                        os.path.join(ROOT, "tests", "host", "text_source_check.cpp"), SOURCES[1], SOURCES[2], "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    for i, (name, text, fastq) in enumerate(check_texts()):
        path = str(tmp_path / f"text{i}")
        with open(path, "wb") as f:
            f.write(text)
        r = subprocess.run([exe, path, str(int(fastq))], capture_output=True, text=True, env=env, timeout=300)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (name, r.stderr[-4000:])
        assert r.returncode == 0, (name, r.returncode, r.stdout[-500:], r.stderr[-2000:])
        cuts, feeds = parse_check_output(r.stdout)
        want = G.reads(text, fastq)
        P = 4 if fastq else 2
        assert sorted(cuts) == [(g, n) for g in (1, 2) for n in range(1, 10)], name
        for (group, n), got in cuts.items():                 # (n = 9 is more than the records of the short texts: empty shards)
            assert got == G.cuts(text, P, group, n), (name, group, n)
        whole = [f for f in feeds if f[0] == "source" and f[1][1] == "all"]
        assert [int(f[1][0]) for f in whole] == [1, 2, 3, 7, 23, 64, 4096], name
        for _, (chunk, _, _), got, batches, handed in whole:
            # chunks of a few bytes hold no complete record: their text is carried in front of the next one, not lost
            assert got == want and handed == len(text) and batches <= max(len(want), 0) and (batches > 0) == bool(want), (name, chunk)
        shards = [f for f in feeds if f[0] == "source" and f[1][1] != "all"]
        assert len(shards) == 2 * 2 * sum(range(1, 10)), name
        at = 0
        for group in (1, 2):
            for n in range(1, 10):
                for chunk in (7, 4096):
                    mine = shards[at:at + n]
                    at += n
                    for r_, (_, (ch, b, e), got, _, handed) in enumerate(mine):
                        assert (int(ch), int(b), int(e)) == (chunk, cuts[(group, n)][r_], cuts[(group, n)][r_ + 1]), name
                        assert got == G.reads(text[int(b):int(e)], fastq) and handed == int(e) - int(b), (name, group, n, chunk, r_)
                    assert [x for f in mine for x in f[2]] == want, (name, group, n, chunk)      # the shards' reads, concatenated, are the file's
        lines = [f for f in feeds if f[0] == "getline"]
        assert [int(f[1][0]) for f in lines] == [1, 3, 1000], name
        for _, (batch,), got, batches, _ in lines:
            assert got == want and batches == -(-len(want) // int(batch)), (name, batch)
