"""What does ContigGraph::printGraph's file cost on the device, part by part, and what does the same file cost by the route that exists without
these calls?  (GPU box; one GPU; measurement, no bar.)

BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31 -- loaded and scanned once; the scan's own junction map
handed to Stage 3 (the map of profiles/stage3_build.txt).  Every repetition starts from a build that has just finished and is still on the
device (fgpu_stage3_build, not timed).  Host clock around calls that end synchronised, no events.

1. fgpu_stage3_raw_graph (<prefix>.raw_graph.fastg) and fgpu_stage3_fasta_take.  The call's parts under the library's own host clocks
   (fgpu_diag_fastg_times): the build's records and the map to the host; the summaries; the graph made of the build; the walk; the records' lists
   and the join; fgpu_stage3_fastg (its checks, the records' way to the device, the three kernels).  Then the kernels of one more call with
   events on: the join's (s3j_) and the FASTG's (s3g_).
2. The DETIPPED graph by two routes in turn, each from a fresh fgpu_stage3_detip (not timed):
     device  fgpu_stage3_graph_fastg + fgpu_stage3_fasta_take
     host    what exists without the call: fgpu_stage3_graph_take, fgpu_stage3_join of the graph's lists taken to the host
             (fgpu_stage3_join_take), and the text formatted on the host in C++, one thread (scripts/micro/host_fastg.cpp: the same walk, the
             same name function; sized, then written)
   The two files differ in <this> only (the host route has the graph's record numbers, not the live graph's contig numbers): compared with
   the numbers taken out.

    python scripts/stage3_fastg_times.py > profiles/stage3_fastg.txt"""
import ctypes as C
import os
import re
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

REPS = 5
K, MRL = 31, 100
PARTS = ("records and map to the host", "summaries", "graph of the build", "walk (fastg_records)", "lists and fgpu_stage3_join", "fgpu_stage3_fastg")
so = os.path.join(tempfile.mkdtemp(), "host_fastg.so")
subprocess.run(["g++", "-std=c++14", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "scripts", "micro", "host_fastg.cpp"), "-o", so], check=True)
host = C.CDLL(so)
host.host_fastg.restype = C.c_uint64
host.host_fastg.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]

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


def spread(v):
    v = sorted(v)
    return f"min {v[0]:.1f} ms, median {v[len(v) // 2]:.1f}, max {v[-1]:.1f} ({len(v)} repetitions)"


def parts():
    ms = (C.c_double * 6)()
    ctx._c(ctx.lib.fgpu_diag_fastg_times(ctx.h, ms))
    return [float(v) for v in ms]


def call(fn, *args):
    """(ms of the call, ms of the copy-out, the call's parts, the file, info)"""
    nbytes, fi = C.c_uint64(0), L.FastgInfo()
    t0 = now()
    ctx._c(fn(ctx.h, *args, C.byref(nbytes), C.byref(fi)))
    t1 = now()
    p = parts()
    data = ctx.stage3_fasta_take(nbytes.value)
    t2 = now()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), p, data, fi.as_dict()


# ---- 1. the raw graph ----
def raw():
    built = ctx.stage3_build(MRL, take=False)
    assert built["status"] == 0
    return call(ctx.lib.fgpu_stage3_raw_graph, MRL) + (built,)


raw()                                                             # (warm up: code objects, rocPRIM's choices, the host's pages)
runs = [raw() for _ in range(REPS)]
data, info, built = runs[-1][3:]
print(f"\n# 1. fgpu_stage3_raw_graph.  The build: {built['totals'][0]} calls; the file: {len(data)} bytes, {data.count(10) // 4} records, {info}")
print("call     " + spread([r[0] for r in runs]))
for i, part in enumerate(PARTS):
    print(f"  {part:32s} " + spread([r[2][i] for r in runs]))
print("  (the parts' sum)                 " + spread([sum(r[2]) for r in runs]))
print("copy-out " + spread([r[1] for r in runs]) + "  fgpu_stage3_fasta_take")
ctx.stage3_build(MRL, take=False)
ctx.profile_enable(True)
ctx.kernel_times_reset()
wall = call(ctx.lib.fgpu_stage3_raw_graph, MRL)[0]
kt = {k_: v for k_, v in ctx.kernel_times().items() if k_.startswith(("s3g_", "s3j_"))}
ctx.profile_enable(False)
print(f"kernels of one more call with events on (call {wall:.1f} ms, these kernels {sum(v[1] for v in kt.values()):.2f} ms)")
for k_, (launches, t) in sorted(kt.items()):
    print(f"  {k_:14s} {launches:3d} launch(es) {t:8.3f} ms")
del data, runs


# ---- 2. the detipped graph: the device's route and the host's, in turn ----
def device_route():
    ctx.stage3_build(MRL, take=False)
    ctx.stage3_detip(MRL)
    return call(ctx.lib.fgpu_stage3_graph_fastg)


def host_route():
    ctx.stage3_build(MRL, take=False)
    ctx.stage3_detip(MRL)
    t0 = now()
    out, one = L.TipsOut(), np.zeros(1, dtype=np.uint64)          # (the C ABI itself: no Python lists between the steps)
    out.list_first = one.ctypes.data
    assert ctx.lib.fgpu_stage3_graph_take(ctx.h, C.byref(out)) == L.ERR_ARG       # no room: how much is needed
    nodes, contigs = np.empty(out.n_nodes, dtype=api.TIPS_NODE_DTYPE), np.empty(out.n_contigs, dtype=api.TIPS_CONTIG_DTYPE)
    first, pieces = np.empty(out.n_contigs + 1, dtype=np.uint64), np.empty(out.n_pieces, dtype=api.JOIN_PIECE_DTYPE)
    out.nodes, out.nodes_cap, out.contigs, out.list_first, out.contigs_cap = nodes.ctypes.data, len(nodes), contigs.ctypes.data, first.ctypes.data, len(contigs)
    out.pieces, out.pieces_cap = pieces.ctypes.data, len(pieces)
    ctx._c(ctx.lib.fgpu_stage3_graph_take(ctx.h, C.byref(out)))
    t1 = time.perf_counter()
    joined, totals = np.empty(len(contigs), dtype=api.JOINED_DTYPE), (C.c_uint64 * 3)()
    ctx._c(ctx.lib.fgpu_stage3_join(ctx.h, first.ctypes.data, len(contigs), pieces.ctypes.data, len(pieces), None, 0, None, 0, None, 0, None, 0, joined.ctypes.data, totals))
    text, dist, cov = np.empty(totals[0], dtype=np.uint64), np.empty(totals[1], dtype=np.uint8), np.empty(totals[2], dtype=np.uint8)
    ctx._c(ctx.lib.fgpu_stage3_join_take(ctx.h, text.ctypes.data, len(text), dist.ctypes.data, len(dist), cov.ctypes.data, len(cov)))
    t2 = now()
    args = (nodes.ctypes.data, len(nodes), contigs.ctypes.data, len(contigs), joined.ctypes.data, text.ctypes.data, MRL)
    size = host.host_fastg(*args, None)
    out = np.empty(max(size, 1), dtype=np.uint8)
    host.host_fastg(*args, out.ctypes.data)
    t3 = time.perf_counter()
    return (1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)), out[:size].tobytes()


device_route(), host_route()
d_runs, h_runs = [], []
for _ in range(REPS):
    d_runs.append(device_route())
    h_runs.append(host_route())
d_data, h_data = d_runs[-1][3], h_runs[-1][1]
strip = lambda b: re.sub(rb"NODE_0x[0-9a-f]+_", b"NODE_", b)      # noqa: E731
assert strip(d_data) == strip(h_data), "the two routes wrote different files"
print(f"\n# 2. the detipped graph: {len(d_data)} bytes, {d_data.count(10) // 4} records, {d_runs[-1][4]}")
print("## device: fgpu_stage3_graph_fastg + fgpu_stage3_fasta_take")
print("wall     " + spread([r[0] + r[1] for r in d_runs]))
print("  call     " + spread([r[0] for r in d_runs]))
for i, part in enumerate(PARTS):
    if any(r[2][i] for r in d_runs):
        print(f"    {part:30s} " + spread([r[2][i] for r in d_runs]))
print("  copy-out " + spread([r[1] for r in d_runs]))
print("## host: fgpu_stage3_graph_take + fgpu_stage3_join taken to the host + the text formatted in C++ (one thread)")
print("wall     " + spread([r[0][0] for r in h_runs]))
for i, part in enumerate(("fgpu_stage3_graph_take", "fgpu_stage3_join + fgpu_stage3_join_take",
                          "host formatting (sized, then written)")):
    print(f"  {part}: " + spread([r[0][1 + i] for r in h_runs]))
print(f"\nthe same file but for <this>; the host route's minimum over the device route's: {min(r[0][0] for r in h_runs) / min(r[0] + r[1] for r in d_runs):.2f} x")
ctx.close()
