"""`faucet -gpus N` with FAUCET_SHARD_PROTOCOL=slices: pass 1 by filter slices in the C++ host (faucet_amd/host/shard_host.h, batch_board.h).
Every rank packs the batches of its own read shard, the packed blocks travel rank to rank, all ranks load the whole stream into their slice
of the filters, the planes are ORed over the ranks and the filters gathered by slices.  The N contexts share the box's one device.  Every
file is the COMPILED REFERENCE's (tests/golden/*, or oracle/_ref/faucet_ref run on the spot), dump order included."""
import os
import re
import subprocess

import pytest

from tests import test_gpu_vs_reference_fuzz as fuzz
from tests.golden_util import Case
from tests.test_gpu_multi import CLI, _run, _same_files

pytestmark = pytest.mark.gpu

SLICES = {"FAUCET_SHARD_PROTOCOL": "slices", "FGPU_CLI_TIMES": "1"}


@pytest.mark.parametrize("gpus", [2, 3, 4])
@pytest.mark.parametrize("case", ["c1_k21", "ragged_k31", "se_cleaning_k21", "mercy_k21", "pe_mercy_k21", "pe_repeats_k25", "onehash_k25"])
def test_sliced_cli_writes_the_reference_files(case, gpus, tmp_path):
    """the files and counters test_sharded_cli_writes_the_reference_files checks, with pass 1 by filter slices: plain and --mercy (the lockstep
    of a batch, its fail plane over the ranks, its probe), single and paired ends, cleaning, one hash function"""
    c = Case(case)
    prefix, r = _run(c, tmp_path, gpus, env=SLICES)
    assert r.returncode == (0 if c.no_cleaning else 3), r.stdout[-2000:] + r.stderr[-3000:]
    assert "pass 1 (shards, filter slices)" in r.stderr and "pass 1 (filter slices): pack + publish" in r.stderr, r.stderr[-3000:]
    _same_files(c, prefix)
    cn = c.counters
    assert f"Distinct junctions: {cn['distinct_junctions']} " in r.stdout
    assert f"Number of processed kmers: {cn['nb_processed']} " in r.stdout
    assert f"Number of kmers that we j-checked: {cn['nb_jcheck_kmer']} " in r.stdout
    assert f"Reads processed: {cn['load_reads_processed']}" in r.stdout
    assert f"Unambiguous reads: {cn['load_unambiguous']}" in r.stdout
    if c.paired:
        assert f"Empty count: {cn['empty_count']}, not empty count: {cn['not_empty_count']}" in r.stdout


def repeated(case, tmp_path, at_least=(3 << 20) + 1):
    """the golden's records, whole, repeated to just over 3 MiB: with -chunk_mb 1 every one of three shards is cut into three batches"""
    c = Case(case)
    text = c.reads_text()
    assert text.endswith(b"\n")
    path = str(tmp_path / ("reads.fq" if c.fastq else "reads.fa"))
    with open(path, "wb") as f:
        f.write(text * (at_least // len(text) + 1))
    assert os.path.getsize(path) > 3 << 20
    return c, path


@pytest.mark.skipif(not os.path.exists(fuzz.REF_BIN), reason="oracle/_ref/faucet_ref was not built (make -C oracle ref)")
@pytest.mark.parametrize("mercy", [False, True], ids=["plain", "mercy"])
@pytest.mark.parametrize("case", ["ragged_k31", "pe_repeats_k25"])
def test_several_batches_per_shard_equal_the_compiled_reference(case, mercy, tmp_path, monkeypatch):
    """three shards of three batches each, against the compiled reference run on the same text; the last rank's scan shard begins behind the
    six batches of the shards below it (fgpu_scan_resident_base) and still answers validity from the planes its pass 1 kept"""
    c, path = repeated(case, tmp_path)
    runs = []
    real_run = subprocess.run

    def recording_run(*a, **kw):
        runs.append(real_run(*a, **kw))
        return runs[-1]

    monkeypatch.setattr(fuzz.subprocess, "run", recording_run)
    args = c.meta["args"] + (["--mercy"] if mercy else [])
    writes = (".bloom", ".junctions") if c.no_cleaning else (".bloom", ".junctions", ".short_pair_filter") + ((".long_pair_filter",) if c.paired else ())
    fuzz.cli_against_reference(path, args, tmp_path, cli_extra=["-gpus", "3", "-chunk_mb", "1"], env=SLICES, writes=writes)
    err = runs[-1].stderr
    assert "pass 1 (shards, filter slices)" in err, err[-3000:]
    reused = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"rank (\d+) pass 2: .*valid_reused (\d+)", err)}
    print(f"\nvalid_reused per rank: {reused}")
    assert sorted(reused) == [0, 1, 2] and all(v > 0 for v in reused.values()), err[-3000:]


def test_more_shards_than_records_by_slices(tmp_path):
    """8 shards of a 30-record file: shards without a batch, ranks whose slice of the filter is all they contribute"""
    c = Case("c1_k21")
    few = b"\n".join(c.reads_text().split(b"\n")[:60]) + b"\n"
    inp = tmp_path / "few.fa"
    inp.write_bytes(few)
    outs = {}
    for gpus, env in ((1, {}), (8, SLICES)):
        prefix = str(tmp_path / f"few_{gpus}")
        r = subprocess.run([CLI, "-read_load_file", str(inp), "-read_scan_file", str(inp), "-file_prefix", prefix, "-gpus", str(gpus)] + c.meta["args"],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr[-3000:]
        assert ("filter slices" in r.stderr) == (gpus == 8)
        outs[gpus] = (open(prefix + ".bloom", "rb").read(), open(prefix + ".junctions", "rb").read(), re.findall(r"Reads processed: \d+", r.stdout))
    assert outs[1] == outs[8]
    if os.path.exists(fuzz.REF_BIN):                 # ... and the compiled reference's own files on those 30 records
        ref = str(tmp_path / "ref")
        subprocess.run([fuzz.REF_BIN, "-read_load_file", str(inp), "-read_scan_file", str(inp), "-file_prefix", ref] + c.meta["args"],
                       capture_output=True, text=True, timeout=600)
        assert outs[8][:2] == (open(ref + ".bloom", "rb").read(), open(ref + ".junctions", "rb").read())


@pytest.mark.parametrize("mercy", [False, True], ids=["plain", "mercy"])
def test_an_input_over_the_resident_budget_is_refused_before_pass_1(mercy, tmp_path):
    """every rank keeps the whole input in its packed form: 5/8 of a byte per input byte, 9/8 with --mercy.  Over the smallest budget of the
    ranks (here: what FAUCET_DEBUG_SLICES_BUDGET says they have) the run ends before pass 1, exit code 2, the numbers in the message"""
    c = Case("mercy_k21" if mercy else "c1_k21")
    size = len(c.reads_text())
    need = (size * (9 if mercy else 5) + 7) // 8
    prefix, r = _run(c, tmp_path, 2, env=dict(SLICES, FAUCET_DEBUG_SLICES_BUDGET=str(need - 1)))
    assert r.returncode == 2, r.stdout[-2000:] + r.stderr[-3000:]
    assert "load pass failed" in r.stderr and str(size) in r.stderr and str(need) in r.stderr and str(need - 1) in r.stderr
    assert ("9/8" if mercy else "5/8") in r.stderr
    assert "pass 1 (shards" not in r.stderr and not os.path.exists(prefix + ".bloom")
    prefix, r = _run(c, tmp_path, 2, env=dict(SLICES, FAUCET_DEBUG_SLICES_BUDGET=str(need)), tag="fits")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    _same_files(c, prefix)
