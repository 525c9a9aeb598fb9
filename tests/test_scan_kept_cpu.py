"""faucet --scan_kept, host side, where there is no GPU: the command line linked against tests/stub/faucet_gpu_stub.cpp (as tests/test_estimate_cpu.py
links it) -- the stand-in has none of the entry points of the kept scan, the command line refers to them weakly, links unchanged and refuses
the flag by name; the refusals that need no device come before any input is opened; the optional -read_scan_file; the usage text."""
import os
import subprocess

import pytest

from tests.golden_util import Case
from tests.test_estimate_cpu import _args, _reads, cli  # noqa: F401  (the fixture: the command line built against tests/stub)

ENTRY_POINTS = ("fgpu_scan_kept_state", "fgpu_scan_batch_kept", "fgpu_estimate_keep_reads", "fgpu_estimate_take_kept_reads", "fgpu_load_batch_packed_reads")


def _run(exe, *args, timeout=60):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def _idle_fifo(tmp_path, name="load.fifo"):
    """a pipe nobody writes to: a command line that opened it would block until the test's timeout"""
    fifo = str(tmp_path / name)
    os.mkfifo(fifo)
    return fifo


def _nothing_written(tmp_path, prefix):
    return not any(f.startswith(os.path.basename(prefix) + ".") for f in os.listdir(tmp_path))


def test_scan_kept_is_refused_where_the_library_lacks_the_entry_points(cli, tmp_path):  # noqa: F811
    c = Case("c1_k21")
    fifo, prefix = _idle_fifo(tmp_path), str(tmp_path / "out")
    for scan_file in (["-read_scan_file", fifo], []):
        r = _run(cli, "-read_load_file", fifo, *scan_file, "-file_prefix", prefix, "--scan_kept", *c.meta["args"])
        assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        assert "--scan_kept" in r.stderr and "lacks the entry points" in r.stderr
        for name in ENTRY_POINTS:
            assert name in r.stderr
        assert r.stdout == "" and _nothing_written(tmp_path, prefix)      # before anything is opened, sized or printed


def test_without_the_flag_the_stand_in_runs_as_before(cli, tmp_path):  # noqa: F811
    """the weak references change nothing for a run that does not ask for them: the golden's files"""
    c = Case("c1_k21")
    inp, prefix = _reads(c, tmp_path), str(tmp_path / "out")
    r = _run(cli, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", prefix, *c.meta["args"], timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    with open(prefix + ".bloom", "rb") as f:
        assert f.read() == c.bloom().tobytes()
    with open(prefix + ".junctions") as f:
        assert f.read().split("\n")[:-1] == c.junction_lines()


@pytest.mark.parametrize("extra,words", [(["-gpus", "2"], "-gpus 1"), (["-bloom_file", "some.bloom"], "-bloom_file")])
def test_read_shards_and_a_bloom_file_are_refused_before_any_input_is_opened(cli, tmp_path, extra, words):  # noqa: F811
    c = Case("c1_k21")
    fifo, prefix = _idle_fifo(tmp_path), str(tmp_path / "out")
    for scan_file in (["-read_scan_file", fifo], []):
        r = _run(cli, "-read_load_file", fifo, *scan_file, "-file_prefix", prefix, "--scan_kept", *extra, *c.meta["args"])
        assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        assert "--scan_kept" in r.stderr and words in r.stderr and "lacks the entry points" not in r.stderr
        assert r.stdout == "" and _nothing_written(tmp_path, prefix)


def test_the_scan_file_is_optional_only_with_the_flag(cli, tmp_path):  # noqa: F811
    c = Case("c1_k21")
    fifo, prefix = _idle_fifo(tmp_path), str(tmp_path / "out")
    r = _run(cli, "-read_load_file", fifo, "-file_prefix", prefix, *c.meta["args"])
    assert r.returncode == 1 and "Some required argument is missing." in r.stderr and r.stdout == ""
    # the flag excuses the scan file and nothing else
    r = _run(cli, "-read_scan_file", fifo, "-file_prefix", prefix, "--scan_kept", *c.meta["args"])
    assert r.returncode == 1 and "Some required argument is missing." in r.stderr
    r = _run(cli, "-read_load_file", fifo, "--scan_kept", *c.meta["args"])
    assert r.returncode == 1 and "Some required argument is missing." in r.stderr
    r = _run(cli, "-read_load_file", fifo, "-file_prefix", prefix, "--scan_kept", *_args(c))
    assert r.returncode == 1 and "Some required argument is missing." in r.stderr
    # ... except what --estimate excuses beside it (refused further on: the stand-in has neither)
    r = _run(cli, "-read_load_file", fifo, "-file_prefix", prefix, "--scan_kept", "--estimate", *_args(c))
    assert r.returncode == 2 and "lacks the entry points" in r.stderr and r.stdout == ""
    assert _nothing_written(tmp_path, prefix)


def test_the_usage_text_lists_the_flag(cli):  # noqa: F811
    for args in ([], ["--help"], ["-bogus"]):
        r = _run(cli, *args)
        assert r.returncode == 1 and "--scan_kept" in r.stderr and "-read_scan_file may be left out" in r.stderr


# ---- the ABI: what the library exports and the ctypes table binds ------------------------------------------------------------------------------
def test_the_library_exports_the_entry_points_and_the_header_declares_them():
    import ctypes as C
    import re

    from faucet_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "faucet_gpu.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"^int " + name + r"\(fgpu_ctx\* ctx", hdr, re.M), name
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert re.search(r"#define FGPU_LOAD_KEEP_READS +8\b", hdr) and L.LOAD_KEEP_READS == 8
    assert L.LOAD_KEEP_READS & (L.LOAD_KEEP_CARRY | L.LOAD_SHARD_TIMES | L.LOAD_SHARD_PLANES) == 0
    assert C.sizeof(L.KeptReads) == 24 and [f[0] for f in L.KeptReads._fields_] == ["offsets_dev", "n_reads", "max_read_len"]
    assert re.search(r"#define FGPU_ABI_VERSION +3\b", hdr) and lib.fgpu_abi_version() == 3
    # without a context every one of them is an argument error, not a crash
    assert lib.fgpu_scan_kept_state(None, None, None, None, None) == L.ERR_ARG
    assert lib.fgpu_scan_batch_kept(None, C.c_uint64(0), None) == L.ERR_ARG
    assert lib.fgpu_estimate_keep_reads(None) == L.ERR_ARG
    assert lib.fgpu_estimate_take_kept_reads(None, None, C.c_uint64(0), None) == L.ERR_ARG
    assert lib.fgpu_load_batch_packed_reads(None, None, None) == L.ERR_ARG
