"""faucet --scan_kept: pass 1 keeps its reads on the device and pass 2 scans them, so -read_scan_file may be left out and one reading of the
input -- a file, or one pipe -- serves the whole run.  Every output file is the golden's (written by the compiled reference) and stdout is the
stdout of the run that was given the same file twice.  Needs an MI355X."""
import os
import subprocess

import pytest

from tests import estimate_ref as R
from tests.golden_util import Case
from tests.test_gpu_estimate import CLI, _round, _stable, _without_counts
from tests.test_gpu_estimate_stream import feeders, output_files, written_input

pytestmark = pytest.mark.gpu

BITS = 14
KEPT_SCAN = "pass 2 (scan of kept reads)"
TEXT_SCAN = "pass 2 (read + scan)"
NAMES = ("Read load file name:", "Read scan file name:")


def run(cwd, args, env=None, timeout=120):
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([CLI, "-file_prefix", "out"] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, FGPU_CLI_TIMES="1", **(env or {})))


def ok_code(c):
    return 0 if c.no_cleaning else 3


def golden_bytes(c, ext):
    if ext == "bloom":
        return c.bloom().tobytes()
    if ext == "junctions":
        return ("\n".join(c.junction_lines()) + "\n").encode()
    return c.pair_filter(ext.split("_")[0]).tobytes()


def assert_golden_files(c, cwd, only=None):
    for ext in only or output_files(c):
        with open(os.path.join(cwd, "out." + ext), "rb") as f:
            assert f.read() == golden_bytes(c, ext), ext


def two_file_run(c, inp, tmp_path, args=None):
    g = run(str(tmp_path / "twice"), ["-read_load_file", inp, "-read_scan_file", inp] + (args or c.meta["args"]))
    assert g.returncode == ok_code(c), g.stdout[-2000:] + g.stderr[-3000:]
    assert TEXT_SCAN in g.stderr and KEPT_SCAN not in g.stderr and "reads kept" not in g.stderr
    return g


def without_names(out):
    return [ln for ln in _stable(out) if not ln.startswith(NAMES)]


# ---- 1. a regular file, no -read_scan_file ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21", "mercy_k21", "se_cleaning_k21"])
def test_a_regular_file_is_read_once(name, tmp_path):
    c = Case(name)
    inp = written_input(c, tmp_path)
    r = run(str(tmp_path / "kept"), ["-read_load_file", inp, "--scan_kept"] + c.meta["args"])
    assert r.returncode == ok_code(c), r.stdout[-2000:] + r.stderr[-3000:]
    assert "pass 1 (read + load, reads kept)" in r.stderr and KEPT_SCAN in r.stderr and TEXT_SCAN not in r.stderr
    assert_golden_files(c, str(tmp_path / "kept"))
    g = two_file_run(c, inp, tmp_path)
    assert _stable(r.stdout) == _stable(g.stdout)            # "Read scan file name:" prints the load file's name
    assert_golden_files(c, str(tmp_path / "twice"))


# ---- 2. one FIFO is the only input -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimate", [False, True], ids=["counts_given", "estimate"])
@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21"])
def test_one_fifo_serves_the_whole_run(name, estimate, tmp_path):
    c = Case(name)
    fifo = str(tmp_path / "reads.fifo")
    os.mkfifo(fifo)
    writers = feeders(c.reads_text(), [fifo])
    if estimate:
        empty, once, _ = R.golden_counts(name, BITS)
        _, f0, f1 = R.solve(empty, once, BITS)
        f0, f1 = _round(f0), max(_round(f1), 1)
        args = _without_counts(c.meta["args"])
        r = run(str(tmp_path / "kept"), ["-read_load_file", fifo, "--scan_kept", "--estimate", "-estimate_bits", str(BITS)] + args)
    else:
        r = run(str(tmp_path / "kept"), ["-read_load_file", fifo, "--scan_kept"] + c.meta["args"])
    assert r.returncode == ok_code(c), r.stdout[-2000:] + r.stderr[-3000:]
    for t in writers:
        t.join(timeout=10)
        assert not t.is_alive()
    if estimate:
        marks = ["pass 0 (read + estimate, reads kept)", "pass 1 (load from kept reads, reads kept)", KEPT_SCAN]
        assert r.stdout.split("\n")[:2] == [f"Estimated distinct k-mers (F0): {f0}", f"Estimated singletons (f1): {f1}"], r.stdout[:500]
    else:
        marks = ["pass 1 (read + load, reads kept)", KEPT_SCAN]
    at = [r.stderr.index(m) for m in marks]
    assert at == sorted(at) and TEXT_SCAN not in r.stderr, r.stderr[-3000:]
    assert [ln for ln in r.stdout.split("\n") if ln.startswith(NAMES)] == [f"{NAMES[0]} {fifo}", f"{NAMES[1]} {fifo}"]
    inp = written_input(c, tmp_path)
    if estimate:                                             # the run that was given the two numbers and the file twice
        g = two_file_run(c, inp, tmp_path, args + ["-estimated_kmers", str(f0), "-singletons", str(f1)])
        assert without_names(r.stdout)[2:] == without_names(g.stdout)
        for ext in output_files(c):
            with open(os.path.join(str(tmp_path / "kept"), "out." + ext), "rb") as a, open(os.path.join(str(tmp_path / "twice"), "out." + ext), "rb") as b:
                assert a.read() == b.read(), ext
    else:
        g = two_file_run(c, inp, tmp_path)
        assert without_names(r.stdout) == without_names(g.stdout)
        assert_golden_files(c, str(tmp_path / "kept"))


# ---- 3. keeping that cannot complete -------------------------------------------------------------------------------------------------------------
def test_a_fifo_whose_reads_do_not_fit_ends_with_the_bloom_file_written(tmp_path):
    c = Case("c1_k21")
    fifo = str(tmp_path / "reads.fifo")
    os.mkfifo(fifo)
    writers = feeders(c.reads_text(), [fifo])
    cwd = str(tmp_path / "kept")
    r = run(cwd, ["-read_load_file", fifo, "--scan_kept"] + c.meta["args"], env={"FAUCET_DEBUG_SCAN_KEPT_BUDGET": "64"})
    assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    for t in writers:
        t.join(timeout=10)
        assert not t.is_alive()
    assert "--scan_kept" in r.stderr and "budget 64 bytes" in r.stderr and "bytes kept" in r.stderr
    assert "-bloom_file out.bloom -read_scan_file" in r.stderr
    assert "pass 2 (" not in r.stderr                      # (no scan was begun)
    assert_golden_files(c, cwd, only=["bloom"])
    assert not os.path.exists(os.path.join(cwd, "out.junctions"))


def test_a_regular_file_without_a_scan_file_ends_the_same_way(tmp_path):
    c = Case("c1_k21")
    inp = written_input(c, tmp_path)
    cwd = str(tmp_path / "kept")
    r = run(cwd, ["-read_load_file", inp, "--scan_kept"] + c.meta["args"], env={"FAUCET_DEBUG_SCAN_KEPT_BUDGET": "64"})
    assert r.returncode == 2 and "budget 64 bytes" in r.stderr and "-bloom_file out.bloom" in r.stderr, r.stderr[-3000:]
    assert_golden_files(c, cwd, only=["bloom"])


@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21"])
def test_a_regular_file_with_a_scan_file_falls_back_with_one_note(name, tmp_path):
    c = Case(name)
    inp = written_input(c, tmp_path)
    cwd = str(tmp_path / "kept")
    r = run(cwd, ["-read_load_file", inp, "-read_scan_file", inp, "--scan_kept"] + c.meta["args"], env={"FAUCET_DEBUG_SCAN_KEPT_BUDGET": "64"})
    assert r.returncode == ok_code(c), r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stderr.count("note: --scan_kept") == 1 and "budget 64 bytes" in r.stderr and TEXT_SCAN in r.stderr and KEPT_SCAN not in r.stderr
    assert_golden_files(c, cwd)
    # ... and with room, the scan file that was given is not read: the kept reads are
    r = run(str(tmp_path / "room"), ["-read_load_file", inp, "-read_scan_file", str(tmp_path / "never_opened.fa"), "--scan_kept"] + c.meta["args"])
    assert r.returncode == ok_code(c) and KEPT_SCAN in r.stderr and "note: --scan_kept" not in r.stderr, r.stderr[-3000:]
    assert_golden_files(c, str(tmp_path / "room"))


# ---- 4. refusals, before any input is opened -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,words", [(["-gpus", "2"], "-gpus 1"), (["-bloom_file", "some.bloom"], "-bloom_file")])
def test_read_shards_and_a_bloom_file_are_refused_and_nothing_is_written(extra, words, tmp_path):
    c = Case("c1_k21")
    fifo = str(tmp_path / "reads.fifo")
    os.mkfifo(fifo)                                          # nobody writes: opening it would block until the timeout
    cwd = str(tmp_path / "refused")
    r = run(cwd, ["-read_load_file", fifo, "--scan_kept"] + extra + c.meta["args"], timeout=60)
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "--scan_kept" in r.stderr and words in r.stderr
    assert os.listdir(cwd) == []
