"""Pass 0 without a GPU: the arithmetic that turns a sketch's counts into -estimated_kmers (F0) and -singletons (f1), and the command line's
handling of --estimate where the library has no estimate pass.

fgpu_estimate_solve is host code; it is checked against the formulas of include/faucet_gpu.h on the counts the numpy restatement of the sketch
(tests/estimate_ref.py) gives for the reads of every golden, and the estimates themselves against exact np.unique counts.  The command line is
linked against tests/stub/faucet_gpu_stub.cpp, as tests/test_slices_host_cpu.py links it: the stand-in has no fgpu_estimate_*."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from faucet_amd import _lib as L
from faucet_amd import api
from tests import estimate_ref as R
from tests.golden_util import CASES, Case
from tests.test_host_sanitizers import ROOT, SOURCES

BITS = [10, 14, 22]


def _solve_raw(empty, once, r_bits):
    e = L.Estimate()
    e.empty[:], e.once[:], e.r_bits = empty, once, r_bits
    rc = L.load().fgpu_estimate_solve(C.byref(e))
    return rc, e


def test_struct_layout_matches_the_header():
    assert C.sizeof(L.Estimate) == 96
    assert (L.EST_LEVELS, L.EST_SHIFT, L.EST_MIN_BITS, L.EST_MAX_BITS, L.EST_DEFAULT_BITS) == (4, 4, 8, 34, 30)


@pytest.mark.parametrize("r_bits", BITS)
@pytest.mark.parametrize("name", CASES)
def test_solve_equals_the_formulas_on_every_golden(name, r_bits):
    empty, once, _ = R.golden_counts(name, r_bits)
    want = R.solve(empty, once, r_bits)
    assert want is not None
    level, f0, f1 = api.estimate_solve(empty, once, r_bits)
    print(name, r_bits, "level", level, want[0], "f0", f0, want[1], "f1", f1, want[2])
    assert level == want[0]
    assert abs(f0 - want[1]) <= 1e-12 * want[1]
    assert abs(f1 - want[2]) <= 1e-12 * want[2]
    rc, e = _solve_raw(empty, once, r_bits)
    assert rc == L.OK and (e.level, e.f0, e.f1) == (level, f0, f1)


def test_small_sketches_of_the_goldens_start_from_levels_1_and_2():
    levels = {name: R.solve(*R.golden_counts(name, 10)[:2], 10)[0] for name in CASES}
    assert levels["c1_k21"] == 1 and levels["twohash_k31_L150"] == 2
    assert set(levels.values()) == {1, 2}
    assert {R.solve(*R.golden_counts(name, 22)[:2], 22)[0] for name in CASES} == {0}


@pytest.mark.parametrize("name", CASES)
def test_estimates_at_22_bits_are_within_a_percent_of_the_exact_counts(name):
    """the sketch is deterministic, so this is a fact about these reads, not a sample: the restatement stays within 0.05 % (F0) and 0.14 % (f1)"""
    distinct, singletons = R.exact(R.golden_canon(name))
    empty, once, kmers = R.golden_counts(name, 22)
    assert kmers == len(R.golden_canon(name)) > distinct > singletons > 0
    level, f0, f1 = api.estimate_solve(empty, once, 22)
    print(name, "F0", f0, distinct, f0 / distinct - 1, "f1", f1, singletons, f1 / singletons - 1)
    assert level == 0
    assert abs(f0 - distinct) <= 0.01 * distinct
    assert abs(f1 - singletons) <= 0.01 * singletons


def test_level_3_not_usable_is_a_capacity_error():
    m = 1 << 12
    rc, e = _solve_raw([0, 0, 0, m // 8 - 1], [5, 5, 5, 5], 12)
    assert rc == L.ERR_CAPACITY and e.level == -1 and e.f0 == 0 and e.f1 == 0
    assert list(e.empty) == [0, 0, 0, m // 8 - 1] and list(e.once) == [5, 5, 5, 5]      # the counts stay
    with pytest.raises(api.FaucetGpuError, match="raise r_bits"):
        api.estimate_solve([m, m, m, 0], [0, 0, 0, 0], 12)


def test_an_eighth_of_the_cells_empty_is_usable_exactly():
    m = 1 << 12
    # level 3 alone: levels 0..2 are one cell short of the bar
    rc, e = _solve_raw([m // 8 - 1] * 3 + [m // 8], [0, 0, 0, 100], 12)
    assert rc == L.OK and e.level == 3
    assert e.f0 == pytest.approx(16.0 ** 3 * m * 2.0794415416798357, rel=1e-12)      # ln 8
    assert e.f1 == pytest.approx(16.0 ** 3 * m * 100 / (m // 8), rel=1e-12)
    # a usable level below an unusable one does not count: levels l..3 must ALL be usable
    rc, e = _solve_raw([m, m // 8 - 1, m // 2, m // 2], [0, 0, 7, 9], 12)
    assert rc == L.OK and e.level == 2
    want = R.solve([m, m // 8 - 1, m // 2, m // 2], [0, 0, 7, 9], 12)
    assert (e.level, e.f0, e.f1) == pytest.approx(want, rel=1e-12)
    # ... and all four at the bar start from level 0
    rc, e = _solve_raw([m // 8] * 4, [1, 2, 3, 4], 12)
    assert rc == L.OK and e.level == 0 and e.f1 == pytest.approx(8.0 * 10, rel=1e-12)


@pytest.mark.parametrize("r_bits", [7, 35, -1, 0])
def test_r_bits_outside_8_to_34_is_an_argument_error(r_bits):
    m = 1 << 8
    rc, e = _solve_raw([m] * 4, [0] * 4, r_bits)
    assert rc == L.ERR_ARG and e.level == -1
    with pytest.raises(ValueError):
        api.estimate_solve([m] * 4, [0] * 4, r_bits)


@pytest.mark.parametrize("r_bits", [8, 34])
def test_the_ends_of_the_range_solve(r_bits):
    m = 1 << r_bits
    assert api.estimate_solve([m] * 4, [0] * 4, r_bits) == (0, 0.0, 0.0)
    level, f0, f1 = api.estimate_solve([m // 2] * 4, [m // 4] * 4, r_bits)
    assert level == 0 and f0 == pytest.approx(4 * m * 0.6931471805599453, rel=1e-12) and f1 == pytest.approx(2.0 * m, rel=1e-12)


def test_counts_no_sketch_gives_are_an_argument_error():
    m = 1 << 10
    assert _solve_raw([m + 1, m, m, m], [0] * 4, 10)[0] == L.ERR_ARG
    assert _solve_raw([m, m, m, m - 3], [0, 0, 0, 4], 10)[0] == L.ERR_ARG
    assert L.load().fgpu_estimate_solve(None) == L.ERR_ARG


def test_an_all_empty_sketch_gives_0_and_0():
    for r_bits in (8, 22, 30, 34):
        m = 1 << r_bits
        assert api.estimate_solve([m] * 4, [0] * 4, r_bits) == (0, 0.0, 0.0)


# ---- the command line, linked against the CPU stand-in of the ABI -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("estimate_host") / "faucet_stub")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), *SOURCES, "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _args(c, drop=("-estimated_kmers", "-singletons")):
    a, out, i = c.meta["args"], [], 0
    while i < len(a):
        if a[i] in drop:
            i += 2
            continue
        out.append(a[i])
        i += 1
    return out


def _reads(c, tmp_path):
    inp = str(tmp_path / ("reads.fq" if c.fastq else "reads.fa"))
    with open(inp, "wb") as f:
        f.write(c.reads_text())
    return inp


def test_estimate_is_refused_where_the_library_lacks_the_entry_points(cli, tmp_path):
    c = Case("c1_k21")
    inp, prefix = _reads(c, tmp_path), str(tmp_path / "out")
    r = subprocess.run([cli, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", prefix, "--estimate"] + _args(c),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "--estimate" in r.stderr and "lacks the entry points" in r.stderr
    for name in ("fgpu_estimate_begin", "fgpu_estimate_batch", "fgpu_estimate_end"):
        assert name in r.stderr
    assert r.stdout == "" and not os.path.exists(prefix + ".bloom")      # before anything is read, sized or printed


def test_estimate_with_both_counts_given_runs_as_without_it(cli, tmp_path):
    """nothing is left to estimate: no pass 0, so the stand-in's missing entry points do not matter, and the files are the golden's"""
    c = Case("c1_k21")
    inp, prefix = _reads(c, tmp_path), str(tmp_path / "out")
    r = subprocess.run([cli, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", prefix, "--estimate", "-estimate_bits", "14"] + c.meta["args"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == (0 if c.no_cleaning else 3), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "Estimated distinct k-mers" not in r.stdout and "Estimated singletons" not in r.stdout
    with open(prefix + ".bloom", "rb") as f:
        assert f.read() == c.bloom().tobytes()
    with open(prefix + ".junctions") as f:
        assert f.read().split("\n")[:-1] == c.junction_lines()


def test_estimate_needs_a_regular_load_file(cli, tmp_path):
    """pass 0 reads -read_load_file once more than the run does: a pipe ends the run with exit code 1 before it is opened (nobody writes to it here)"""
    c = Case("c1_k21")
    fifo, prefix = str(tmp_path / "load.fifo"), str(tmp_path / "out")
    os.mkfifo(fifo)
    r = subprocess.run([cli, "-read_load_file", fifo, "-read_scan_file", fifo, "-file_prefix", prefix, "--estimate"] + _args(c),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "--estimate" in r.stderr and "not a regular file" in r.stderr and r.stdout == ""
    r = subprocess.run([cli, "-read_load_file", str(tmp_path / "missing.fa"), "-read_scan_file", fifo, "-file_prefix", prefix, "--estimate"] + _args(c),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "not a regular file" in r.stderr


def test_without_estimate_the_two_counts_are_still_required(cli, tmp_path):
    c = Case("c1_k21")
    inp, prefix = _reads(c, tmp_path), str(tmp_path / "out")
    base = [cli, "-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", prefix]
    for drop in (("-estimated_kmers", "-singletons"), ("-estimated_kmers",), ("-singletons",)):
        r = subprocess.run(base + _args(c, drop), capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Some required argument is missing." in r.stderr and r.stdout == "", (drop, r.returncode, r.stderr[-500:])
    # -estimate_bits alone asks for nothing, and takes 8..34 only
    r = subprocess.run(base + _args(c) + ["-estimate_bits", "14"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Some required argument is missing." in r.stderr
    for bad in ("7", "35"):
        r = subprocess.run(base + c.meta["args"] + ["--estimate", "-estimate_bits", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "-estimate_bits must be in 8..34" in r.stderr
    # another required argument missing is not excused by --estimate
    r = subprocess.run([cli, "-read_load_file", inp, "-file_prefix", prefix, "--estimate"] + _args(c), capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Some required argument is missing." in r.stderr
