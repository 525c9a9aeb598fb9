"""The host side of FAUCET_SHARD_PROTOCOL=slices without a GPU.

The command line links untouched against tests/stub/faucet_gpu_stub.cpp, which answers only the read-shard protocols: shard_host.h refers to
the sliced pass' entry points weakly, finds them missing and refuses the protocol before pass 1; without the variable the run is what it was.
The board that carries the batch descriptions between the ranks' threads (faucet_amd/host/batch_board.h) is exercised alone by
tests/host/batch_board_check.cpp under the thread sanitizer and under the address + undefined-behaviour sanitizers."""
import gzip
import os
import shutil
import subprocess

import pytest

from tests.golden_util import Case
from tests.test_host_sanitizers import ROOT, SOURCES

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slices_host") / "faucet_stub")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *SOURCES, "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]      # (a test of a function's address against null that the compiler knows the answer to)
    return exe


def _run(cli, c, tmp_path, tag, env):
    inp = str(tmp_path / ("reads.fq" if c.fastq else "reads.fa"))
    with open(inp, "wb") as f:
        f.write(c.reads_text())
    prefix = str(tmp_path / tag)
    r = subprocess.run([cli, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", prefix, "-gpus", "2", "-chunk_mb", "1"] + c.meta["args"],
                       capture_output=True, text=True, timeout=600,
                       env=dict({k: v for k, v in os.environ.items() if k != "FAUCET_SHARD_PROTOCOL"}, FGPU_CLI_TIMES="1", **env))
    return prefix, r


@pytest.mark.parametrize("case", ["se_cleaning_k21", "mercy_k21"])
def test_slices_are_refused_where_the_library_lacks_the_entry_points(cli, case, tmp_path):
    c = Case(case)
    prefix, r = _run(cli, c, tmp_path, "slices", {"FAUCET_SHARD_PROTOCOL": "slices"})
    assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "FAUCET_SHARD_PROTOCOL=slices" in r.stderr and "lacks the entry points" in r.stderr
    for name in ("fgpu_load_slice_", "fgpu_group_allgather", "fgpu_scan_resident_base"):
        assert name in r.stderr
    assert "pass 1 (shards" not in r.stderr and not os.path.exists(prefix + ".bloom")      # before pass 1


@pytest.mark.parametrize("case", ["se_cleaning_k21", "mercy_k21"])
def test_without_the_variable_the_run_is_what_it_was(cli, case, tmp_path):
    c = Case(case)
    prefix, r = _run(cli, c, tmp_path, "default", {})
    assert r.returncode == (0 if c.no_cleaning else 3), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "pass 1 (shards, presence protocol)" in r.stderr and "filter slices" not in r.stderr
    for ext in ("bloom", "junctions", "short_pair_filter", "long_pair_filter"):
        gold = os.path.join(c.dir, f"out.{ext}.gz")
        if not os.path.exists(gold):
            continue
        with open(prefix + "." + ext, "rb") as f, gzip.open(gold, "rb") as g:
            assert f.read() == g.read(), ext


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_batch_board_under_sanitizers(sanitizer, tmp_path):
    """four publisher / consumer threads over a few hundred batches, uneven shards, an empty one, and an abort that wakes every waiter:
    clean, and every consumer saw the same file-order list (the program checks it and says "ok")"""
    exe = str(tmp_path / "batch_board_check")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitizer, "-Wall", "-Wextra", "-I",
                        os.path.join(ROOT, "faucet_amd", "host"), os.path.join(ROOT, "tests", "host", "batch_board_check.cpp"), "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=66",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])
