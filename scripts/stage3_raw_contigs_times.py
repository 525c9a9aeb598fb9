"""What does the reference's <prefix>.raw_contigs.fasta cost on the device (fgpu_stage3_raw_contigs: the two record arrays of the build to the
host, the plan, the emission kernels; then fgpu_stage3_fasta_take), and what did the same file cost before this call existed?  (GPU box; one
GPU; measurement, no bar.)

BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31 -- loaded and scanned once; the scan's own junction map
handed to Stage 3 (the map of profiles/stage3_build.txt).  Every repetition starts from a build that has just finished and is still on the
device (fgpu_stage3_build, not timed: profiles/stage3_build.txt has it); the two ways take turns.

  device    fgpu_stage3_raw_contigs + fgpu_stage3_fasta_take: wall time, host clock around calls that end synchronised, no events; then the
            library's own kernel times of one more call with events on, apart
  baseline  what exists without the call: fgpu_stage3_build_take (all six arrays to the host), the same fgpu_raw_plan, and the FASTA assembled
            on the host in C++ from the 2-bit words (scripts/micro/host_fasta.cpp, one thread), split into its three parts
Both files are compared byte for byte.

    python scripts/stage3_raw_contigs_times.py > profiles/stage3_raw_contigs.txt"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from faucet_amd import _lib as L  # noqa: E402
from faucet_amd import api  # noqa: E402

REPS = 7
K, MRL = 31, 100
tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "host_fasta.so")
subprocess.run(["g++", "-std=c++11", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "scripts", "micro", "host_fasta.cpp"), "-o", so], check=True)
host = C.CDLL(so)
host.host_fasta.restype = C.c_uint64
host.host_fasta.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_void_p]

dev = torch.device("cuda", 0)
n, E, S = 10_000_000, 100_000_000, 20_000_000
tai, nh = api.load_filter_shape(E, S)
reads = bench.make_reads(bench.make_genome(20_000_000, 2, dev), n, 100, 0.01, 1000, dev)
ctx = api.Context(K, tai, nh)
lst, sst, b2, keys, recs = bench.step_single(ctx, bench.device_batches(reads, bench.batch_bounds(n, 1_000_000, 2)))
keys, recs = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(recs, dtype=api.JUNC_DTYPE)
del reads
ctx.stage3_set_junctions(keys, recs)
print(f"config 2's scanned map: {len(keys)} junctions; max_read_length {MRL}", flush=True)


def now():
    ctx.synchronize()
    return time.perf_counter()


def device_way():
    built = ctx.stage3_build(MRL, take=False)
    assert built["status"] == 0
    t0 = now()
    data, info = ctx.stage3_raw_contigs(MRL)
    t1 = now()
    return 1e3 * (t1 - t0), data, info, built


def baseline_way():
    built = ctx.stage3_build(MRL, take=False)
    nc, nt, ns, nv = built["totals"]
    t0 = now()
    out, calls = np.empty(nc, dtype=api.CONTIG_DTYPE), np.empty(nc, dtype=api.BUILD_DTYPE)
    text, kmers, dist, cov = np.empty(nt, dtype=np.uint64), np.empty(ns, dtype=np.uint64), np.empty(ns, dtype=np.uint8), np.empty(nv, dtype=np.uint8)
    ctx._c(ctx.lib.fgpu_stage3_build_take(ctx.h, out.ctypes.data, calls.ctypes.data, nc, text.ctypes.data, nt, kmers.ctypes.data, dist.ctypes.data, ns, cov.ctypes.data, nv))
    t1 = time.perf_counter()
    seqs = np.empty(nc, dtype=api.FASTA_SEQ_DTYPE)
    n_out, ri = C.c_uint64(0), L.RawInfo()
    assert ctx.lib.fgpu_raw_plan(keys.ctypes.data, recs.ctypes.data, len(keys), out.ctypes.data, calls.ctypes.data, nc, K, MRL, seqs.ctypes.data, nc, C.byref(n_out),
                                 C.byref(ri)) == L.PLAN_OK
    t2 = time.perf_counter()
    size = host.host_fasta(seqs.ctypes.data, n_out.value, text.ctypes.data, K, None)
    data = np.empty(size, dtype=np.uint8)
    host.host_fasta(seqs.ctypes.data, n_out.value, text.ctypes.data, K, data.ctypes.data)
    t3 = time.perf_counter()
    return (1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)), data.tobytes(), ri.as_dict()


def spread(v):
    v = sorted(v)
    return f"min {v[0]:.1f} ms, median {v[len(v) // 2]:.1f}, max {v[-1]:.1f} ({len(v)} repetitions)"


device_way(), baseline_way()                                      # (warm up: code objects, rocPRIM's choices, the host's pages)
d_ms, b_ms = [], []
for _ in range(REPS):                                             # the two ways in turn
    t, d_data, d_info, built = device_way()
    d_ms.append(t)
    t, b_data, b_info = baseline_way()
    b_ms.append(t)
assert d_data == b_data and d_info == b_info, "the two ways wrote different files"
print(f"the build: {built['totals'][0]} calls, {built['totals'][1]} text words; the file: {len(d_data)} bytes, {d_info}")
print("\n## device: fgpu_stage3_raw_contigs + fgpu_stage3_fasta_take")
print("wall " + spread(d_ms))
print("\n## baseline: fgpu_stage3_build_take + fgpu_raw_plan + the FASTA assembled on the host (C++, one thread)")
print("wall " + spread([t[0] for t in b_ms]))
for i, part in enumerate(("fgpu_stage3_build_take", "fgpu_raw_plan", "host assembly (sized, then written)")):
    print(f"  {part}: " + spread([t[1 + i] for t in b_ms]))
print(f"\nbyte for byte the same file; the baseline's minimum over the device's: {min(t[0] for t in b_ms) / min(d_ms):.2f} x")

ctx.stage3_build(MRL, take=False)
ctx.profile_enable(True)
ctx.kernel_times_reset()
t0 = now()
ctx.stage3_raw_contigs(MRL)
wall = 1e3 * (now() - t0)
kt = {k_: v for k_, v in ctx.kernel_times().items() if k_.startswith("s3f_")}
ctx.profile_enable(False)
total = sum(v[1] for v in kt.values())
print(f"\n## kernels of one more device call with events on (wall {wall:.1f} ms, the emission kernels {total:.2f} ms; the rest is the two record arrays' way to the host, "
      "the plan on the host, the records' way back, rocPRIM's two scans and the file's way to the host)")
for k_, (launches, t) in sorted(kt.items()):
    print(f"  {k_:10s} {launches:3d} launch(es) {t:8.3f} ms  {100 * t / total:5.1f} % of the kernels, {100 * t / wall:5.1f} % of the call")
ctx.close()
