"""`faucet -gpus N --scan_kept` under FAUCET_SHARD_PROTOCOL=slices, host side, where there is no GPU.

  * the command line linked against tests/stub/faucet_gpu_stub.cpp (as tests/test_slices_host_cpu.py links it): the stand-in has none of the
    entry points, so the refusals are what can be seen -- each before the input is opened (a FIFO nobody writes to would block the run);
  * the ranges of pass 2 over kept batches of a piped stream (faucet_amd/host/kept_ranges.h) against a restatement in plain Python;
  * the turn-taking reader and the board walked in the stream's order (text_source.h TurnSource, batch_board.h StreamCursor) as a stand-alone
    program (tests/host/turn_source_check.cpp), built plain, with -fsanitize=thread and with -fsanitize=address,undefined, reading a FIFO:
    the reads in consume order are those of the reference's reading loop (tests/getline_ref.py), and an abort wakes every waiter.
No sanitizer is put on anything loaded into python."""
import os
import random
import shutil
import subprocess
import threading

import pytest

from tests import getline_ref as G
from tests.golden_util import Case
from tests.test_host_sanitizers import ROOT, SOURCES

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

HOST = os.path.join(ROOT, "faucet_amd", "host")
SAN_ENV = dict(TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")


# ---- 1. the stub-linked command line ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("multi_scan_kept") / "faucet_stub")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *SOURCES, "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def refused(cli, tmp_path, extra, env, scan_kept=True, scan_file=False):
    """the run on a FIFO that nobody writes to: it must end by itself, with exit code 2, nothing on stdout and nothing written"""
    c = Case("c1_k21")
    fifo = str(tmp_path / "reads.fifo")
    if not os.path.exists(fifo):
        os.mkfifo(fifo)
    cwd = tmp_path / f"refused{len(os.listdir(str(tmp_path)))}"
    cwd.mkdir()
    args = ["-read_load_file", fifo] + (["-read_scan_file", fifo] if scan_file else []) + (["--scan_kept"] if scan_kept else [])
    r = subprocess.run([cli] + args + ["-file_prefix", "out", "-gpus", "2"] + extra + c.meta["args"], cwd=str(cwd), capture_output=True, text=True,
                       timeout=60, env=dict({k: v for k, v in os.environ.items() if k != "FAUCET_SHARD_PROTOCOL"}, **env))
    assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert os.listdir(str(cwd)) == []
    return r


SLICES = {"FAUCET_SHARD_PROTOCOL": "slices"}


def test_without_the_variable_both_old_refusals_are_unchanged(cli, tmp_path):
    r = refused(cli, tmp_path, [], {})
    assert r.stdout == "" and r.stderr == "--scan_kept needs -gpus 1: read shards and filter slices keep batches of their own\n"
    r = refused(cli, tmp_path, [], {"FAUCET_SHARD_PROTOCOL": "presence"})
    assert r.stdout == "" and "--scan_kept needs -gpus 1" in r.stderr
    r = refused(cli, tmp_path, [], {}, scan_kept=False, scan_file=True)      # a pipe with -gpus N: behind the settings, before it is opened
    assert "is not a regular file: with -gpus the read shards are byte ranges of their input (pipes need -gpus 1)" in r.stderr
    assert "Reads processed" not in r.stdout


def test_under_slices_the_flag_is_refused_by_naming_the_missing_entry_points(cli, tmp_path):
    r = refused(cli, tmp_path, [], SLICES)
    assert r.stdout == "" and "--scan_kept with -gpus 2" in r.stderr and "lacks the entry points" in r.stderr
    for name in ("fgpu_load_slice_keep_reads", "fgpu_load_slice_packed_reads", "fgpu_load_slice_expect_reads", "fgpu_load_slice_adopt_reads",
                 "fgpu_scan_kept_range", "fgpu_scan_batch_kept", "fgpu_scan_prepare_kept"):
        assert name in r.stderr
    assert "-gpus 1" in r.stderr                             # what to do instead


@pytest.mark.parametrize("extra,words", [(["-bloom_file", "some.bloom"], ["-bloom_file", "leave --scan_kept out"]),
                                         (["-batch_reads", "100"], ["-batch_reads", "leave -batch_reads out"])])
def test_the_other_refusals_under_slices(cli, tmp_path, extra, words):
    r = refused(cli, tmp_path, extra, SLICES)
    assert r.stdout == "" and all(w in r.stderr for w in words), r.stderr


def test_a_pipe_under_slices_without_the_flag_and_estimate_on_a_pipe(cli, tmp_path):
    r = refused(cli, tmp_path, [], SLICES, scan_kept=False, scan_file=True)
    assert "is not a regular file" in r.stderr and "--scan_kept" in r.stderr and "Reads processed" not in r.stdout
    # --estimate on a pipe with several GPUs: pass 0 keeps its reads on one device only -- the message that was there
    c = Case("c1_k21")
    fifo = str(tmp_path / "reads.fifo")
    cwd = tmp_path / "estimate"
    cwd.mkdir()
    args = [a for a in c.meta["args"]]
    for flag in ("-estimated_kmers", "-singletons"):
        at = args.index(flag)
        del args[at:at + 2]
    r = subprocess.run([cli, "-read_load_file", fifo, "-read_scan_file", fifo, "--estimate", "-file_prefix", "out", "-gpus", "2"] + args, cwd=str(cwd),
                       capture_output=True, text=True, timeout=60, env=dict(os.environ, **SLICES))
    assert r.returncode in (1, 2) and r.stdout == "" and "is not a regular file" in r.stderr and os.listdir(str(cwd)) == [], (r.returncode, r.stderr)


# ---- 2. pass 2's ranges over kept batches ----------------------------------------------------------------------------------------------------
def ranges_restated(T, reads, n, group):
    """n + 1 bounds: range r ends behind the first batch at which the running sum of T reaches (r + 1) * total // n -- and, for groups of
    reads, at which the reads so far are whole groups; the last range ends behind the last batch"""
    total, bounds, g = sum(T), [0], 0
    for r in range(n - 1):
        target = (r + 1) * total // n
        while g < len(T) and (sum(T[:g]) < target or (group > 1 and sum(reads[:g]) % group)):
            g += 1
        bounds.append(g)
    return bounds + [len(T)]


def test_the_ranges_of_pass_2_follow_the_restatement(tmp_path):
    exe = str(tmp_path / "kept_ranges_check")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-Wall", "-Wextra", "-I", HOST,
                        os.path.join(ROOT, "tests", "host", "kept_ranges_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    rng = random.Random(7)
    cases = []
    for n in range(1, 9):
        for group in (1, 2):
            cases += [(n, group, [], []), (n, group, [1000], [10]), (n, group, [640] * 7, [4] * 7), (n, group, [5, 5, 1 << 40, 5], [1, 1, 3, 1]),
                      (n, group, [3] * 5, [1] * 5), (n, group, [(1 << 62)] * 3, [2] * 3)]
            for _ in range(25):
                G_ = rng.randint(1, 40)
                reads = [rng.randint(1, 9) for _ in range(G_)]
                if group == 2 and sum(reads) % 2:
                    reads[-1] += 1                           # whole pairs in all
                cases.append((n, group, [rng.randint(1, 1 << rng.randint(1, 30)) + x for x in reads], reads))
    text = "".join(f"{n} {group} {len(T)} {' '.join(map(str, T))} {' '.join(map(str, reads))}\n" for n, group, T, reads in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-3000:]
    r2 = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=dict(os.environ, **SAN_ENV))
    assert r2.stdout == r.stdout                             # deterministic
    got = [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    assert len(got) == len(cases)
    for (n, group, T, reads), b in zip(cases, got):
        assert b == ranges_restated(T, reads, n, group), (n, group, T, reads, b)
        assert len(b) == n + 1 and b[0] == 0 and b[-1] == len(T) and all(x <= y for x, y in zip(b, b[1:]))      # contiguous and covering
        if group == 2:
            assert all(sum(reads[:x]) % 2 == 0 for x in b if x < len(T))      # no pair straddles two ranks (the last bound is the stream's end, whatever it holds)
    # the edges by hand
    assert ranges_restated([640] * 7, [4] * 7, 3, 1) == [0, 3, 5, 7] and ranges_restated([1000], [10], 8, 1) == [0] + [1] * 8
    assert ranges_restated([5, 5, 1 << 40, 5], [1] * 4, 4, 1) == [0, 3, 3, 3, 4] and ranges_restated([], [], 3, 1) == [0, 0, 0, 0]
    assert ranges_restated([7], [1], 8, 1) == [0, 0] + [1] * 7                 # 1 * 7 // 8 = 0 is reached before any batch: an empty first range


# ---- 3. the turn-taking reader and the board in the stream's order ---------------------------------------------------------------------------
def feed_fifo(path, text):
    def feed():
        try:
            with open(path, "wb") as f:
                for lo in range(0, len(text), 333):
                    f.write(text[lo:lo + 333])
                    f.flush()
        except BrokenPipeError:
            pass
    t = threading.Thread(target=feed, daemon=True)
    t.start()
    return t


@pytest.mark.parametrize("sanitizer", ["none", "thread", "address,undefined"])
def test_ranks_that_take_turns_at_one_pipe_consume_the_reference_s_reads(sanitizer, tmp_path):
    exe = str(tmp_path / "turn_source_check")
    flags = ["-O1"] if sanitizer == "none" else ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizer]
    r = subprocess.run(["g++", "-std=c++11", *flags, "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                        os.path.join(ROOT, "tests", "host", "turn_source_check.cpp"), SOURCES[1], SOURCES[2], "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, **SAN_ENV)
    texts = [(Case("ragged_k31").reads_text()[:20000], False), (Case("pe_fastq_k21").reads_text()[:30000], True),
             (b"h\nAC\nh2\n\nh3\nGGT", False), (b"", False)]
    runs = 0
    for text, fastq in texts:
        want = G.reads(text, fastq)
        for n, chunk in ((1, 64), (2, 64), (3, 257), (5, 4096), (8, 1 << 20)) if len(text) > 1000 else ((2, 64), (8, 1 << 20)):
            fifo = str(tmp_path / f"in{runs}.fifo")
            runs += 1
            os.mkfifo(fifo)
            writer = feed_fifo(fifo, text)
            r = subprocess.run([exe, fifo, str(int(fastq)), str(n), str(chunk)], capture_output=True, text=True, env=env, timeout=300)
            writer.join(timeout=10)
            assert not writer.is_alive()
            assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
            lines = r.stdout.split("\n")
            assert r.returncode == 0 and lines[-2:] == ["ok", ""], (n, chunk, r.returncode, r.stdout[-500:], r.stderr[-2000:])
            got = [b"" if ln == "read -" else bytes.fromhex(ln[5:]) for ln in lines if ln.startswith("read ")]
            assert got == want, (n, chunk, len(got), len(want))
            batches = int(next(ln for ln in lines if ln.startswith("batches ")).split()[1])
            assert (batches > 0) == bool(want) and (chunk > 300 or len(text) < 1000 or batches >= 2 * n)      # small chunks: every thread has had turns
    # an abort in the middle: the thread that is handed chunk 3 aborts instead; every thread comes back, each of them told
    text = Case("ragged_k31").reads_text()[:20000]
    for n in (2, 5):
        fifo = str(tmp_path / f"abort{n}.fifo")
        os.mkfifo(fifo)
        writer = feed_fifo(fifo, text)
        r = subprocess.run([exe, fifo, "0", str(n), "257", "3"], capture_output=True, text=True, env=env, timeout=300)
        writer.join(timeout=10)
        assert not writer.is_alive()
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert r.returncode == 0 and r.stdout.split("\n")[-3:] == [f"aborted {n}", "ok", ""], (r.returncode, r.stdout[-500:], r.stderr[-2000:])
