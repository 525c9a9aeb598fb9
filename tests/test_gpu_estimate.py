"""Pass 0 on the device (fgpu_estimate_*, faucet_amd/csrc/estimate.hip): the counts of the sketch equal the numpy restatement's
(tests/estimate_ref.py) word for word -- on every golden's reads, in one batch and in seven, from host, device and fgpu_text_split batches, on a
synthetic batch built for the places the kernel can go wrong --, the pass keeps to its place in the context's state machine, and
`faucet --estimate` fills in -estimated_kmers / -singletons with the numbers the restatement gives.  Needs an MI355X."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from tests import estimate_ref as R
from tests.golden_util import CASES, Case
from tests.test_gpu_multi import _same_files
from tests.test_gpu_parity import chunks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "faucet_amd", "faucet")
BITS = [10, 14, 22]


def placeholder(k, **kw):
    """the context of a caller that does not know its sizes yet: the pass reads neither tai nor n_hash"""
    return api.Context(k, 128, 1, **kw)


def sketch(ctx, batches, r_bits):
    ctx.estimate_begin(r_bits)
    for b in batches:
        ctx.estimate_batch(b)
    return ctx.estimate_end()


def assert_counts(got, want, r_bits):
    empty, once, kmers = want
    assert (got["empty"], got["once"], got["kmers"], got["r_bits"]) == (empty, once, kmers, r_bits)
    level, f0, f1 = R.solve(empty, once, r_bits)
    assert got["level"] == level and got["f0"] == pytest.approx(f0, rel=1e-12) and got["f1"] == pytest.approx(f1, rel=1e-12)


def host_arrays(lines):
    b = api.ReadBatch.from_lines(lines)
    return b.bases, b.offsets


@pytest.mark.parametrize("name", CASES)
def test_counts_equal_the_restatement_on_every_golden(name):
    """one batch and seven, 2^10, 2^14 and 2^22 cells per level, all on one context: every pass starts from clean planes"""
    c = Case(name)
    lines = c.lines()
    bases, offs = host_arrays(lines)
    seven = chunks(bases, offs, 7)
    # the split leaves duplicates of one k-mer in different batches
    cuts = np.linspace(0, len(lines), 8).astype(int)
    first, rest = R.canon_kmers(lines[:cuts[1]], c.k), R.canon_kmers(lines[cuts[1]:], c.k)
    assert len(np.intersect1d(first, rest)) > 0
    ctx = placeholder(c.k)
    for r_bits in BITS:
        want = R.golden_counts(name, r_bits)
        assert_counts(sketch(ctx, [api.ReadBatch(bases, offs)], r_bits), want, r_bits)
        assert_counts(sketch(ctx, seven, r_bits), want, r_bits)
    ctx.close()


@pytest.mark.parametrize("name", ["c1_k21", "pe_fastq_k21"])
def test_device_and_text_split_batches_give_the_same_counts(name):
    import torch
    c = Case(name)
    want = R.golden_counts(name, 14)
    ctx = placeholder(c.k)
    # the file's text, records split on the device: two chunks, the second one final
    text = c.reads_text()
    ctx.estimate_begin(14)
    batch, used = ctx.text_split(text[:len(text) // 2], c.fastq, False)
    ctx.estimate_batch(batch)
    batch, rest = ctx.text_split(text[used:], c.fastq, True)
    ctx.estimate_batch(batch)
    assert used + rest == len(text)
    assert_counts(ctx.estimate_end(), want, 14)
    # device pointers, with and without the total the caller may know
    bases, offs = host_arrays(c.lines())
    d_bases, d_offs = torch.from_numpy(bases).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    for n_positions in (None, int(offs[-1]) + len(offs) - 1):
        b = api.ReadBatch(d_bases.data_ptr(), d_offs.data_ptr(), n_reads=len(offs) - 1, on_device=True, keepalive=(d_bases, d_offs), n_positions=n_positions)
        assert_counts(sketch(ctx, [b], 14), want, 14)
    ctx.close()


def test_default_bits_are_30():
    """2^30 cells per level, 1 GiB of planes for the duration of the pass; the restatement counts cells with np.unique"""
    c = Case("ragged_k31")
    ctx = placeholder(c.k)
    got = sketch(ctx, [api.ReadBatch(*host_arrays(c.lines()))], 0)
    assert_counts(got, R.golden_counts("ragged_k31", 30), 30)
    assert got["level"] == 0
    distinct, singletons = R.exact(R.golden_canon("ragged_k31"))
    assert abs(got["f0"] - distinct) <= 0.01 * distinct and abs(got["f1"] - singletons) <= 0.01 * singletons
    ctx.close()


def synthetic_lines():
    """reads that start at every offset modulo 32 of the packed stream, N's and lower case, reads shorter than any k, an empty read, poly-A and
    poly-T (canonical form 0: h = 0, clz = 64, level 3, cell 0), one read four times, reads whose k-mers occur once, and more than 2^20 + 5
    stream positions in all"""
    rng = np.random.default_rng(20261019)
    genome = rng.integers(0, 4, 6000)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def read(start, length):
        return acgt[genome[start:start + length]].tobytes()

    lines = [read(int(rng.integers(0, 5000)), 33 + i) for i in range(64)]          # lengths 33..96: every start offset modulo 32
    damaged = bytearray(read(100, 120))
    damaged[40:41] = b"N"
    damaged[77:80] = b"acg"
    lines += [bytes(damaged), b"NNNNNNNN", b"ACG", b"", b"A", b"A" * 60, b"T" * 60, b"", read(7, 31), read(7, 30), b"acgtacgtacgtacgtacgtacgtacgtacgtacgtacgt"]
    lines += [read(2000, 101)] * 4
    lines += [read(int(s), 100) for s in rng.integers(0, 5900, 10500)]             # 1.06 M positions: the grid strides
    lines += [acgt[rng.integers(0, 4, 50)].tobytes() for _ in range(300)]          # k-mers seen once (at k = 31)
    lines += [b"", b"GATTACA" * 9, b"T" * 31 + b"A" * 31]
    return lines


@pytest.fixture(scope="module")
def synthetic():
    lines = synthetic_lines()
    starts = np.cumsum([0] + [len(x) + 1 for x in lines[:64]])[:64]
    assert set(int(s) % 32 for s in starts) == set(range(32))
    assert sum(len(x) + 1 for x in lines) > (1 << 20) + 5
    return lines


@pytest.mark.parametrize("k", [31, 5])
def test_synthetic_batch_equals_the_restatement(synthetic, k):
    canon = R.canon_kmers(synthetic, k)
    assert (canon == 0).sum() >= 2 * (60 - k + 1)                     # the poly-A and poly-T reads
    bases, offs = host_arrays(synthetic)
    ctx = placeholder(k)
    empty_batch = api.ReadBatch.from_lines([])
    for r_bits in (8, 16):
        want = R.counts(canon, r_bits)
        assert_counts(sketch(ctx, [api.ReadBatch(bases, offs)], r_bits), want, r_bits)
        # ... cut in three, with empty batches before, between and behind
        parts = chunks(bases, offs, 3)
        assert_counts(sketch(ctx, [empty_batch, parts[2], empty_batch, parts[0], parts[1], empty_batch], r_bits), want, r_bits)
    ctx.close()


@pytest.mark.parametrize("k", [31, 5])
def test_poly_a_and_poly_t_land_in_cell_0_of_level_3(k):
    ctx = placeholder(k)
    m = 1 << 8
    got = sketch(ctx, [api.ReadBatch.from_lines([b"A" * 40, b"T" * 40])], 8)
    assert got["empty"] == [m, m, m, m - 1] and got["once"] == [0, 0, 0, 0] and got["kmers"] == 2 * (40 - k + 1)
    # one occurrence alone: the cell is hit once
    got = sketch(ctx, [api.ReadBatch.from_lines([b"T" * k])], 8)
    assert got["empty"] == [m, m, m, m - 1] and got["once"] == [0, 0, 0, 1] and got["kmers"] == 1
    # nothing at all: an empty batch, reads shorter than k, no batch
    got = sketch(ctx, [api.ReadBatch.from_lines([]), api.ReadBatch.from_lines([b"ACGT"[:k - 1], b""])], 8)
    assert got["empty"] == [m] * 4 and got["once"] == [0] * 4 and got["kmers"] == 0 and (got["level"], got["f0"], got["f1"]) == (0, 0.0, 0.0)
    assert sketch(ctx, [], 8)["empty"] == [m] * 4
    ctx.close()


def test_kmers_equal_a_load_of_the_same_reads(synthetic):
    c = Case("ragged_k31")
    for lines, k in ((c.lines(), c.k), (synthetic, 31), (synthetic, 5)):
        bases, offs = host_arrays(lines)
        ctx = api.Context(k, 1 << 20, 3)
        got = sketch(ctx, chunks(bases, offs, 3), 12)
        ctx.load_begin()
        for b in chunks(bases, offs, 2):
            ctx.load_batch(b)
        st = ctx.load_end()
        assert got["kmers"] == st["kmers"] == len(R.canon_kmers(lines, k))
        ctx.close()


def test_a_sketch_too_full_is_a_capacity_error_with_the_counts_filled_in():
    """4 M random 31-mers: level 3 holds a 16^-3 sample of them, about 980, in 2^8 cells -- a load of 3.8, some 6 cells left empty of the 32 the
    solve asks for"""
    k, rng = 31, np.random.default_rng(5)
    lines = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4000)].tobytes() for _ in range(1000)]
    batch = api.ReadBatch(*host_arrays(lines))
    want = R.counts(R.canon_kmers(lines, k), 8)
    ctx = placeholder(k)
    assert R.solve(want[0], want[1], 8) is None
    ctx.estimate_begin(8)
    ctx.estimate_batch(batch)
    with pytest.raises(api.FaucetGpuError, match="raise r_bits"):
        ctx.estimate_end()
    got = ctx.last_estimate
    assert (got["empty"], got["once"], got["kmers"], got["level"]) == (want[0], want[1], want[2], -1)
    ctx.estimate_begin(8)                         # the pass was over: the next one begins, from clean planes
    assert ctx.estimate_end()["empty"] == [1 << 8] * 4
    ctx.close()


def refused(ctx, rc_want, fn, *args):
    rc = fn(ctx.h, *args)
    assert rc == rc_want, (rc, ctx.lib.fgpu_last_error(ctx.h))


def test_the_pass_keeps_to_its_place_in_the_state_machine():
    c = Case("c1_k21")
    lib = L.load()
    ctx = api.Context(c.k, 1 << 20, 3)
    batch = api.ReadBatch(*host_arrays(c.lines()[:200]))
    s, e = batch.c_struct(), L.Estimate()
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_batch, C.byref(s))              # before begin
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_end, C.byref(e))
    refused(ctx, L.ERR_ARG, lib.fgpu_estimate_begin, 7)
    refused(ctx, L.ERR_ARG, lib.fgpu_estimate_begin, 35)
    ctx.load_begin()
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_begin, 10)                      # inside a load pass
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_batch, C.byref(s))
    ctx.load_batch(batch)
    load_stats = ctx.load_end()
    bloo2 = ctx.bloom_download(L.BLOO2)
    ctx.scan_begin()
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_begin, 10)                      # inside a scan pass
    ctx.scan_batch(batch)
    scan_stats = ctx.scan_end()
    ctx.estimate_begin(10)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_begin, 0)                           # load, sliced load, scan, presence inside an estimate pass
    refused(ctx, L.ERR_STATE, lib.fgpu_load_slice_begin, 0, 512)
    refused(ctx, L.ERR_STATE, lib.fgpu_scan_begin)
    refused(ctx, L.ERR_STATE, lib.fgpu_presence_batch, C.byref(s))
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_begin, 10)
    refused(ctx, L.ERR_STATE, lib.fgpu_load_batch, C.byref(s))
    ctx.estimate_batch(batch)
    got = ctx.estimate_end()
    assert_counts(got, R.counts(R.canon_kmers(c.lines()[:200], c.k), 10), 10)
    assert got["kmers"] == load_stats["kmers"]
    refused(ctx, L.ERR_STATE, lib.fgpu_estimate_end, C.byref(e))                # over
    # the pass left the filters and the junction map alone: the same load and scan again give what they gave
    assert np.array_equal(ctx.bloom_download(L.BLOO2), bloo2)
    ctx.load_begin()
    ctx.load_batch(batch)
    assert ctx.load_end() == load_stats and np.array_equal(ctx.bloom_download(L.BLOO2), bloo2)
    ctx.scan_begin()
    ctx.scan_batch(batch)
    again = ctx.scan_end()
    assert {k: again[k] for k in ("n_junctions", "nb_processed", "nb_skipped", "kmers")} == {k: scan_stats[k] for k in ("n_junctions", "nb_processed", "nb_skipped", "kmers")}
    ctx.close()


def test_a_context_can_be_destroyed_inside_the_pass():
    ctx = placeholder(21)
    ctx.estimate_begin(20)
    ctx.estimate_batch(api.ReadBatch.from_lines([b"ACGTTGCAACGTTGCAACGTTGCAACG"]))
    ctx.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _without_counts(args):
    out, i = [], 0
    while i < len(args):
        if args[i] in ("-estimated_kmers", "-singletons"):
            i += 2
            continue
        out.append(args[i])
        i += 1
    return out


def _cli(cwd, inp, args, env=None):
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([CLI, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", "out"] + args, cwd=cwd, capture_output=True, text=True,
                          timeout=600, env=dict(os.environ, **(env or {})))


def _stable(stdout):
    """stdout without the two lines that hold wall-clock seconds (time(), whole seconds: they differ when a run crosses a second's boundary)"""
    return [ln for ln in stdout.split("\n") if not ln.startswith("Time to load:") and not ln.startswith("Time in seconds for read scan:")]


def _round(x):
    return int(math.floor(x + 0.5))             # llround for positive values


@pytest.mark.parametrize("bits", [None, 14], ids=["default_bits", "14_bits"])
@pytest.mark.parametrize("name", ["c1_k21", "ragged_k31", "pe_fastq_k21"])
def test_cli_estimate_fills_in_the_two_counts(name, bits, tmp_path):
    c = Case(name)
    inp = str(tmp_path / ("reads.fq" if c.fastq else "reads.fa"))
    with open(inp, "wb") as f:
        f.write(c.reads_text())
    r_bits = bits or 30
    empty, once, _ = R.golden_counts(name, r_bits)
    _, f0, f1 = R.solve(empty, once, r_bits)
    want_f0, want_f1 = _round(f0), max(_round(f1), 1)
    ok = 0 if c.no_cleaning else 3
    extra = ["-estimate_bits", str(bits)] if bits else []

    r = _cli(str(tmp_path / "estimated"), inp, _without_counts(c.meta["args"]) + ["--estimate"] + extra, env={"FGPU_CLI_TIMES": "1"})
    assert r.returncode == ok, r.stdout[-2000:] + r.stderr[-3000:]
    head = r.stdout.split("\n")[:2]
    assert head == [f"Estimated distinct k-mers (F0): {want_f0}", f"Estimated singletons (f1): {want_f1}"], r.stdout[:500]
    assert f"Estimated number of distinct kmers, for sizing bloom filter: {want_f0}." in r.stdout
    assert re.search(r"\[cli\] pass 0 \(read \+ estimate\) +[0-9.]+ ms", r.stderr), r.stderr[-3000:]
    assert r.stderr.index("pass 0 (read + estimate)") < r.stderr.index("pass 1 (read + load)")

    # the same numbers given by hand, no --estimate: the same files, and the same stdout behind the two estimate lines
    g = _cli(str(tmp_path / "given"), inp, _without_counts(c.meta["args"]) + ["-estimated_kmers", str(want_f0), "-singletons", str(want_f1)])
    assert g.returncode == ok, g.stdout[-2000:] + g.stderr[-3000:]
    assert "Estimated distinct" not in g.stdout
    assert _stable(r.stdout)[2:] == _stable(g.stdout)
    exts = ["bloom", "junctions"] + ([] if c.no_cleaning else ["short_pair_filter"] + (["long_pair_filter"] if c.paired else []))
    for ext in exts:
        with open(str(tmp_path / "estimated" / ("out." + ext)), "rb") as a, open(str(tmp_path / "given" / ("out." + ext)), "rb") as b:
            assert a.read() == b.read(), ext
    for ext in set(["short_pair_filter", "long_pair_filter"]) - set(exts):
        assert not os.path.exists(str(tmp_path / "estimated" / ("out." + ext)))

    # both counts given alongside --estimate: nothing to estimate, the golden's own run
    b = _cli(str(tmp_path / "both"), inp, c.meta["args"] + ["--estimate"] + extra, env={"FGPU_CLI_TIMES": "1"})
    assert b.returncode == ok, b.stdout[-2000:] + b.stderr[-3000:]
    assert "Estimated distinct k-mers" not in b.stdout and "Estimated singletons" not in b.stdout and "pass 0" not in b.stderr
    _same_files(c, str(tmp_path / "both" / "out"))


def test_cli_estimate_with_read_shards_runs_pass_0_on_the_first_device(tmp_path):
    c = Case("se_cleaning_k21")
    inp = str(tmp_path / "reads.fa")
    with open(inp, "wb") as f:
        f.write(c.reads_text())
    empty, once, _ = R.golden_counts(c.name, 14)
    _, f0, f1 = R.solve(empty, once, 14)
    args = _without_counts(c.meta["args"]) + ["-estimate_bits", "14"]
    r = _cli(str(tmp_path / "shards"), inp, args + ["--estimate", "-gpus", "2"])
    assert r.returncode == 3, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.split("\n")[:2] == [f"Estimated distinct k-mers (F0): {_round(f0)}", f"Estimated singletons (f1): {max(_round(f1), 1)}"]
    g = _cli(str(tmp_path / "one"), inp, args + ["-estimated_kmers", str(_round(f0)), "-singletons", str(max(_round(f1), 1))])
    assert g.returncode == 3
    for ext in ("bloom", "junctions", "short_pair_filter"):
        with open(str(tmp_path / "shards" / ("out." + ext)), "rb") as a, open(str(tmp_path / "one" / ("out." + ext)), "rb") as b:
            assert a.read() == b.read(), ext
