"""`faucet -gpus N --scan_kept` with FAUCET_SHARD_PROTOCOL=slices: the sliced pass 1 keeps the reads, pass 2 scans the kept batches -- rank 0
by fgpu_scan_batch_kept, the ranks above by fgpu_scan_prepare_kept -- so -read_load_file is read ONCE and may be a pipe: the ranks then take
turns at one reader, pass 2's shards are ranges of the stream's batches and read offsets change ranks between the passes
(faucet_amd/host/shard_host.h, batch_board.h, kept_ranges.h, text_source.h).  The N contexts share the box's one device.  Every file is the
COMPILED REFERENCE's (tests/golden/*, or oracle/_ref/faucet_ref run on the same text)."""
import os
import re
import subprocess

import pytest

from tests import test_gpu_vs_reference_fuzz as fuzz
from tests.golden_util import Case
from tests.test_gpu_estimate import _stable
from tests.test_gpu_estimate_stream import feeders, written_input
from tests.test_gpu_multi import CLI, _same_files
from tests.test_gpu_multi_slices import repeated

pytestmark = pytest.mark.gpu

SLICES = {"FAUCET_SHARD_PROTOCOL": "slices", "FGPU_CLI_TIMES": "1", "FGPU_DEBUG_DELTA_CHECK": "1"}
KEPT_LOAD = "pass 1 (shards, filter slices, reads kept)"
KEPT_SCAN = "pass 2 (scan of kept reads)"
NAMES = ("Read load file name:", "Read scan file name:")


def run(args, env, timeout=600):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env))
    assert "merged in-map planes differ" not in r.stderr, r.stderr[-2000:]
    return r


def ok_code(c):
    return 0 if c.no_cleaning else 3


def reused_by_rank(err):
    return {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"rank (\d+) pass 2 \(scan of kept reads\): .*valid_reused (\d+)", err)}


def joined(writers):
    for t in writers:
        t.join(timeout=10)
        assert not t.is_alive()


# ---- 1. a regular file, no -read_scan_file ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gpus", [2, 3])
@pytest.mark.parametrize("case", ["c1_k21", "se_cleaning_k21", "mercy_k21", "pe_fastq_k21", "pe_repeats_k25"])
def test_a_regular_file_is_read_once_by_the_sliced_ranks(case, gpus, tmp_path):
    c = Case(case)
    inp = written_input(c, tmp_path)
    prefix = str(tmp_path / "kept")
    r = run(["-read_load_file", inp, "--scan_kept", "-file_prefix", prefix, "-gpus", str(gpus)] + c.meta["args"], SLICES)
    assert r.returncode == ok_code(c), r.stdout[-2000:] + r.stderr[-3000:]
    _same_files(c, prefix)
    cn = c.counters
    assert f"Distinct junctions: {cn['distinct_junctions']} " in r.stdout
    assert f"Number of processed kmers: {cn['nb_processed']} " in r.stdout
    assert f"Number of kmers that we j-checked: {cn['nb_jcheck_kmer']} " in r.stdout
    assert f"Reads processed: {cn['load_reads_processed']}" in r.stdout
    assert f"Unambiguous reads: {cn['load_unambiguous']}" in r.stdout
    if c.paired:
        assert f"Empty count: {cn['empty_count']}, not empty count: {cn['not_empty_count']}" in r.stdout
    assert KEPT_LOAD in r.stderr and "pass 2 (read + scan)" not in r.stderr, r.stderr[-3000:]
    assert sorted(reused_by_rank(r.stderr)) == list(range(gpus)), r.stderr[-3000:]
    # stdout is that of the run that was given the file twice, without the flag ("Read scan file name:" prints the load file's name)
    twice = str(tmp_path / "twice")
    g = run(["-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", twice, "-gpus", str(gpus)] + c.meta["args"], SLICES)
    assert g.returncode == ok_code(c) and KEPT_SCAN not in g.stderr and "reads kept" not in g.stderr, g.stderr[-3000:]
    assert [ln.replace(prefix, "<prefix>") for ln in _stable(r.stdout)] == [ln.replace(twice, "<prefix>") for ln in _stable(g.stdout)]


# ---- 2. one FIFO is the only input -----------------------------------------------------------------------------------------------------------
def against_the_reference_from_a_fifo(c, path, args, gpus, tmp_path, extra=()):
    """the compiled reference on the file at `path`; the command line on a FIFO that is fed the same text, its only input.  Every file the
    command line writes the reference wrote too, with the same bytes; the counters line for line.  Returns the command line's run"""
    ref_dir, gpu_dir = tmp_path / "ref", tmp_path / "gpu"
    ref_dir.mkdir()
    gpu_dir.mkdir()
    rr = subprocess.run(["stdbuf", "-o0", fuzz.REF_BIN, "-read_load_file", path, "-read_scan_file", path, "-file_prefix", str(ref_dir / "out")] + args,
                        capture_output=True, text=True, errors="replace", timeout=600)
    fifo = str(tmp_path / "reads.fifo")
    os.mkfifo(fifo)
    with open(path, "rb") as f:
        writers = feeders(f.read(), [fifo])
    rg = run(["-read_load_file", fifo, "--scan_kept", "-file_prefix", str(gpu_dir / "out"), "-gpus", str(gpus), "-chunk_mb", "1"] + args + list(extra), SLICES)
    assert rg.returncode == (0 if "--no_cleaning" in args else 3), rg.stdout[-2000:] + rg.stderr[-3000:]
    joined(writers)
    mine = sorted(os.listdir(gpu_dir))
    assert any(f.endswith(".bloom") for f in mine) and any(f.endswith(".junctions") for f in mine), mine
    for f in mine:
        assert (gpu_dir / f).read_bytes() == (ref_dir / f).read_bytes(), f
    for line in fuzz.LINES:
        want = [ln.strip() for ln in rr.stdout.splitlines() if ln.startswith(line)]
        got = [ln.strip() for ln in rg.stdout.splitlines() if ln.startswith(line)]
        assert want == got, (line, want, got)
    a = [ln.replace(str(ref_dir), "<prefix>") for ln in fuzz.stdout_lines(rr.stdout) if not ln.startswith(NAMES)]
    b = [ln.replace(str(gpu_dir), "<prefix>") for ln in fuzz.stdout_lines(rg.stdout) if not ln.startswith(NAMES)]
    assert b and b[-1].startswith("Number of junctions:") and a[:len(b)] == b, [x for x in zip(a, b) if x[0] != x[1]][:5]
    assert [ln for ln in rg.stdout.split("\n") if ln.startswith(NAMES)] == [f"{NAMES[0]} {fifo}", f"{NAMES[1]} {fifo}"]
    return rg


@pytest.mark.skipif(not os.path.exists(fuzz.REF_BIN), reason="oracle/_ref/faucet_ref was not built (make -C oracle ref)")
@pytest.mark.parametrize("mercy", [False, True], ids=["plain", "mercy"])
@pytest.mark.parametrize("gpus", [2, 3])
@pytest.mark.parametrize("case", ["ragged_k31", "pe_repeats_k25"])
def test_one_fifo_serves_the_sliced_ranks(case, gpus, mercy, tmp_path):
    """just over 3 MiB in chunks of at most 1 MiB: six batches taken in turns, so every rank packs batches that another rank scans"""
    c, path = repeated(case, tmp_path)
    rg = against_the_reference_from_a_fifo(c, path, c.meta["args"] + (["--mercy"] if mercy else []), gpus, tmp_path)
    err = rg.stderr
    assert KEPT_LOAD in err and "pass 2 (read + scan)" not in err, err[-3000:]
    m = re.search(r"the read offsets of (\d+) of (\d+) batches changed ranks", err)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) >= 2 * gpus, err[-3000:]
    reused = reused_by_rank(err)
    print(f"\noffsets of {m.group(1)} of {m.group(2)} batches changed ranks; valid_reused per rank: {reused}")
    assert sorted(reused) == list(range(gpus)) and all(v > 0 for v in reused.values()), err[-3000:]


def fifo_run(text, args, gpus, tmp_path, tag, env=None):
    fifo = str(tmp_path / f"{tag}.fifo")
    os.mkfifo(fifo)
    writers = feeders(text, [fifo])
    prefix = str(tmp_path / tag)
    r = run(["-read_load_file", fifo, "--scan_kept", "-file_prefix", prefix, "-gpus", str(gpus)] + args, dict(SLICES, **(env or {})))
    joined(writers)
    return prefix, r


def test_more_ranks_than_batches_from_a_fifo(tmp_path):
    """8 ranks on a 30-record stream (one batch: seven empty ranges, seven ranks that pack nothing) and 2 ranks on a one-batch stream: the
    files of -gpus 1"""
    c = Case("c1_k21")
    few = b"\n".join(c.reads_text().split(b"\n")[:60]) + b"\n"
    inp = tmp_path / "few.fa"
    inp.write_bytes(few)
    one = str(tmp_path / "one")
    r = run(["-read_load_file", str(inp), "-read_scan_file", str(inp), "-file_prefix", one] + c.meta["args"], {})
    assert r.returncode == 0, r.stderr[-3000:]
    want = (open(one + ".bloom", "rb").read(), open(one + ".junctions", "rb").read(), re.findall(r"Reads processed: \d+", r.stdout))
    for gpus in (8, 2):
        prefix, r = fifo_run(few, c.meta["args"], gpus, tmp_path, f"few_{gpus}")
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert KEPT_LOAD in r.stderr and sorted(reused_by_rank(r.stderr)) == list(range(gpus)), r.stderr[-3000:]
        assert re.search(r"the read offsets of \d+ of 1 batches changed ranks", r.stderr), r.stderr[-3000:]
        assert (open(prefix + ".bloom", "rb").read(), open(prefix + ".junctions", "rb").read(), re.findall(r"Reads processed: \d+", r.stdout)) == want


# ---- 3. keeping that cannot complete ---------------------------------------------------------------------------------------------------------
def test_a_fifo_that_does_not_fit_ends_the_run_with_nothing_written(tmp_path):
    c = Case("c1_k21")
    prefix, r = fifo_run(c.reads_text(), c.meta["args"], 2, tmp_path, "lean", env={"FAUCET_DEBUG_SLICES_BUDGET": "4096"})
    assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "load pass failed" in r.stderr and "budget 4096 bytes" in r.stderr and re.search(r"\d+ bytes kept", r.stderr), r.stderr[-3000:]
    assert "pass 1 (shards" not in r.stderr and not os.path.exists(prefix + ".bloom") and not os.path.exists(prefix + ".junctions")


def planes_and_offsets(c, gpus=2):
    """what the ranks of a run over the golden's file keep: the planes of the whole stream (one batch per rank: the file is smaller than a
    chunk) and the read offsets of a rank's own batch -- the most over the ranks, and the input x 5/8 the run is refused above"""
    lines = c.reads_text().split(b"\n")[:-1]
    per = 4 if c.fastq else 2
    seqs = lines[1::per]
    size = len(c.reads_text())
    return sum(len(s) + 1 for s in seqs), len(seqs), (size * 5 + 7) // 8


def test_a_regular_file_whose_reads_cannot_all_be_kept_falls_back_to_its_scan_file(tmp_path):
    c = Case("c1_k21")
    inp = written_input(c, tmp_path)
    T, n_reads, refused_above = planes_and_offsets(c)
    # room for the input x 5/8 that the sliced pass asks for up front, none for the last read offsets beside the planes
    budget = refused_above
    planes_at_least = 5 * (T // 64) * 8
    assert planes_at_least + 8 * (n_reads // 2) > budget, "this golden's headers leave room for its offsets: the knob below decides instead"
    prefix = str(tmp_path / "back")
    r = run(["-read_load_file", inp, "-read_scan_file", inp, "--scan_kept", "-file_prefix", prefix, "-gpus", "2"] + c.meta["args"],
            dict(SLICES, FAUCET_DEBUG_SLICES_BUDGET=str(budget)))
    assert r.returncode == ok_code(c), r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stderr.count("note: --scan_kept") == 1 and f"budget {budget} bytes" in r.stderr and KEPT_SCAN not in r.stderr, r.stderr[-3000:]
    assert "pass 1 (shards, filter slices)" in r.stderr and KEPT_LOAD not in r.stderr
    _same_files(c, prefix)
    # ... and without a scan file the run ends behind <prefix>.bloom and names the restart
    alone = str(tmp_path / "alone")
    r = run(["-read_load_file", inp, "--scan_kept", "-file_prefix", alone, "-gpus", "2"] + c.meta["args"], dict(SLICES, FAUCET_DEBUG_SLICES_BUDGET=str(budget)))
    assert r.returncode == 2 and f"-bloom_file {alone}.bloom -read_scan_file" in r.stderr and "pass 2 (" not in r.stderr, r.stderr[-3000:]
    with open(alone + ".bloom", "rb") as f:
        assert f.read() == c.bloom().tobytes()
    assert not os.path.exists(alone + ".junctions")


# ---- 4. refusals that need no device: before any input is opened -----------------------------------------------------------------------------
@pytest.mark.parametrize("extra,env,words", [([], {}, "--scan_kept needs -gpus 1"), (["-bloom_file", "some.bloom"], SLICES, "-bloom_file"),
                                             (["-batch_reads", "100"], SLICES, "-batch_reads")])
def test_what_stays_refused_is_refused_before_the_input_is_opened(extra, env, words, tmp_path):
    c = Case("c1_k21")
    fifo = str(tmp_path / "reads.fifo")
    os.mkfifo(fifo)                                          # nobody writes: opening it would block until the timeout
    cwd = tmp_path / "refused"
    cwd.mkdir()
    r = subprocess.run([CLI, "-read_load_file", fifo, "--scan_kept", "-file_prefix", "out", "-gpus", "2"] + extra + c.meta["args"], cwd=str(cwd),
                       capture_output=True, text=True, timeout=60, env=dict({k: v for k, v in os.environ.items() if k != "FAUCET_SHARD_PROTOCOL"}, **env))
    assert r.returncode == 2 and r.stdout == "" and words in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert os.listdir(str(cwd)) == []
