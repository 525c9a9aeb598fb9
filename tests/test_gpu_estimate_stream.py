"""faucet --estimate on a stream: -read_load_file is a pipe, pass 0 keeps the batches it packs and pass 1 loads from them, so one reading
serves both -- the reference's two process substitutions with no counts given by hand.  stdout behind the two estimate lines and every output
file are those of a run on the regular file that was given the two numbers.  Needs an MI355X."""
import os
import subprocess
import threading

import pytest

from tests import estimate_ref as R
from tests.golden_util import Case
from tests.test_gpu_estimate import CLI, _cli, _round, _stable, _without_counts

pytestmark = pytest.mark.gpu

BITS = 14
KEPT_MARKS = ["pass 0 (read + estimate, reads kept)", "pass 1 (load from kept reads)"]


def estimates(name):
    empty, once, _ = R.golden_counts(name, BITS)
    _, f0, f1 = R.solve(empty, once, BITS)
    return _round(f0), max(_round(f1), 1)


def written_input(c, tmp_path):
    inp = str(tmp_path / ("reads.fq" if c.fastq else "reads.fa"))
    with open(inp, "wb") as f:
        f.write(c.reads_text())
    return inp


def output_files(c):
    return ["bloom", "junctions"] + ([] if c.no_cleaning else ["short_pair_filter"] + (["long_pair_filter"] if c.paired else []))


def assert_same_run(c, a_dir, b_dir, a_stdout, b_stdout, a_skip):
    assert _stable(a_stdout)[a_skip:] == _stable(b_stdout)
    for ext in output_files(c):
        with open(os.path.join(a_dir, "out." + ext), "rb") as a, open(os.path.join(b_dir, "out." + ext), "rb") as b:
            assert a.read() == b.read(), ext


def feeders(text, paths):
    """one writer thread per FIFO; a reader that goes away early ends the writer, it does not leave it blocked"""
    def feed(path):
        try:
            with open(path, "wb") as f:                      # blocks until the CLI opens its end
                for lo in range(0, len(text), 777):          # odd-sized writes: short reads on the other side
                    f.write(text[lo:lo + 777])
                    f.flush()
        except BrokenPipeError:
            pass
    threads = [threading.Thread(target=feed, args=(p,), daemon=True) for p in paths]
    for t in threads:
        t.start()
    return threads


def given_run(c, inp, tmp_path):
    f0, f1 = estimates(c.name)
    g = _cli(str(tmp_path / "given"), inp, _without_counts(c.meta["args"]) + ["-estimated_kmers", str(f0), "-singletons", str(f1)])
    assert g.returncode == (0 if c.no_cleaning else 3), g.stdout[-2000:] + g.stderr[-3000:]
    return g


@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21", "mercy_k21"])
def test_both_inputs_are_fifos_and_no_counts_are_given(name, tmp_path):
    c = Case(name)
    f0, f1 = estimates(name)
    pipes = [str(tmp_path / "load.fifo"), str(tmp_path / "scan.fifo")]
    for p in pipes:
        os.mkfifo(p)
    writers = feeders(c.reads_text(), pipes)
    cwd = str(tmp_path / "stream")
    os.makedirs(cwd)
    r = subprocess.run([CLI, "-read_load_file", pipes[0], "-read_scan_file", pipes[1], "-file_prefix", "out"] + _without_counts(c.meta["args"]) +
                       ["--estimate", "-estimate_bits", str(BITS)], cwd=cwd, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, FGPU_CLI_TIMES="1"))
    assert r.returncode == (0 if c.no_cleaning else 3), r.stdout[-2000:] + r.stderr[-3000:]
    for t in writers:
        t.join(timeout=10)
        assert not t.is_alive()
    assert r.stdout.split("\n")[:2] == [f"Estimated distinct k-mers (F0): {f0}", f"Estimated singletons (f1): {f1}"], r.stdout[:500]
    assert r.stderr.index(KEPT_MARKS[0]) < r.stderr.index(KEPT_MARKS[1]) and "pass 1 (read + load)" not in r.stderr, r.stderr[-3000:]
    assert "reads consumed: %d" % c.counters["load_reads_processed"] in r.stdout
    g = given_run(c, written_input(c, tmp_path), tmp_path)
    # (the two runs name their inputs differently: the two lines that print the names are compared apart)
    names = ("Read load file name:", "Read scan file name:")
    strip = lambda out: "\n".join(ln for ln in out.split("\n") if not ln.startswith(names))
    assert [ln for ln in r.stdout.split("\n") if ln.startswith(names)] == [f"{names[0]} {pipes[0]}", f"{names[1]} {pipes[1]}"]
    assert_same_run(c, cwd, str(tmp_path / "given"), strip(r.stdout), strip(g.stdout), 2)


@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21"])
def test_a_regular_file_takes_the_kept_path_on_request(name, tmp_path):
    c = Case(name)
    inp = written_input(c, tmp_path)
    args = _without_counts(c.meta["args"]) + ["--estimate", "-estimate_bits", str(BITS)]
    plain = _cli(str(tmp_path / "plain"), inp, args, env={"FGPU_CLI_TIMES": "1"})
    kept = _cli(str(tmp_path / "kept"), inp, args, env={"FGPU_CLI_TIMES": "1", "FAUCET_ESTIMATE_KEEP": "1"})
    ok = 0 if c.no_cleaning else 3
    assert plain.returncode == ok and kept.returncode == ok, kept.stdout[-2000:] + kept.stderr[-3000:]
    assert "pass 1 (read + load)" in plain.stderr and KEPT_MARKS[0] not in plain.stderr and KEPT_MARKS[1] not in plain.stderr
    assert kept.stderr.index(KEPT_MARKS[0]) < kept.stderr.index(KEPT_MARKS[1]) and "pass 1 (read + load)" not in kept.stderr
    assert_same_run(c, str(tmp_path / "kept"), str(tmp_path / "plain"), kept.stdout, plain.stdout, 0)
    # a budget no batch fits: back to reading the file twice, with one note
    back = _cli(str(tmp_path / "back"), inp, args, env={"FGPU_CLI_TIMES": "1", "FAUCET_ESTIMATE_KEEP": "1", "FAUCET_ESTIMATE_KEEP_BYTES": "64"})
    assert back.returncode == ok, back.stdout[-2000:] + back.stderr[-3000:]
    assert back.stderr.count("stopped keeping") == 1 and "pass 1 (read + load)" in back.stderr and KEPT_MARKS[1] not in back.stderr
    assert_same_run(c, str(tmp_path / "back"), str(tmp_path / "plain"), back.stdout, plain.stdout, 0)


def test_a_fifo_that_does_not_fit_the_budget_ends_the_run_and_frees_its_writer(tmp_path):
    c = Case("c1_k21")
    fifo = str(tmp_path / "load.fifo")
    os.mkfifo(fifo)
    writers = feeders(c.reads_text(), [fifo])
    r = _cli(str(tmp_path / "out"), fifo, _without_counts(c.meta["args"]) + ["--estimate", "-estimate_bits", str(BITS)],
             env={"FAUCET_ESTIMATE_KEEP_BYTES": "64"})
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "--estimate" in r.stderr and "-estimated_kmers" in r.stderr and "-singletons" in r.stderr and "budget 64 bytes" in r.stderr
    for t in writers:
        t.join(timeout=10)
        assert not t.is_alive()


def test_a_fifo_with_read_shards_is_refused_before_it_is_opened(tmp_path):
    c = Case("c1_k21")
    fifo = str(tmp_path / "load.fifo")
    os.mkfifo(fifo)                                          # nobody writes: opening it would block
    r = subprocess.run([CLI, "-read_load_file", fifo, "-read_scan_file", fifo, "-file_prefix", str(tmp_path / "out")] + _without_counts(c.meta["args"]) +
                       ["--estimate", "-gpus", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "is not a regular file: with -gpus the read shards are byte ranges of their input (pipes need -gpus 1)" in r.stderr
