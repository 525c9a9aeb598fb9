"""What does ContigGraph::deleteTipsAndClean and the contig file behind it cost on the device's build (fgpu_stage3_detip: the two record arrays of
the build to the host, fgpu_tips_plan, fgpu_stage3_join of the print records over the build where it lies, fgpu_stage3_fasta_joined of the joined
text where it lies; then fgpu_stage3_fasta_take), and what would the same file cost on the host?  (GPU box; one GPU; measurement, no bar: the
parent commit cannot do the step at all.)

BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31 -- loaded and scanned once; the scan's own junction map
handed to Stage 3 (the map of profiles/stage3_build.txt and profiles/stage3_raw_contigs.txt).  Every repetition starts from a build that has just
finished and is still on the device (fgpu_stage3_build, not timed); the two ways take turns.

  device  fgpu_stage3_detip + fgpu_stage3_fasta_take: wall time, host clock around calls that end synchronised, no events; then the library's own
          kernel times of one more call with events on, apart; the plan's share is the host route's fgpu_tips_plan, which is the same call
  host    fgpu_stage3_build_take (all six arrays to the host), the same fgpu_tips_plan, and the print records joined and printed on the host
          in C++ from the 2-bit words (scripts/micro/host_detip.cpp, one thread), split into its three parts
Both files are compared byte for byte.

    python scripts/stage3_detip_times.py > profiles/stage3_detip.txt"""
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

REPS = int(os.environ.get("DETIP_REPS", "5"))
K, MRL = 31, 100
tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "host_detip.so")
subprocess.run(["g++", "-std=c++11", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "scripts", "micro", "host_detip.cpp"), "-o", so], check=True)
host = C.CDLL(so)
host.host_detip_fasta.restype = C.c_uint64
host.host_detip_fasta.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]

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
    data, info = ctx.stage3_detip(MRL)
    t1 = now()
    return 1e3 * (t1 - t0), data, info, built


def host_way():
    built = ctx.stage3_build(MRL, take=False)
    nc, nt, ns, nv = built["totals"]
    t0 = now()
    out, calls = np.empty(nc, dtype=api.CONTIG_DTYPE), np.empty(nc, dtype=api.BUILD_DTYPE)
    text, kmers, dist, cov = np.empty(nt, dtype=np.uint64), np.empty(ns, dtype=np.uint64), np.empty(ns, dtype=np.uint8), np.empty(nv, dtype=np.uint8)
    ctx._c(ctx.lib.fgpu_stage3_build_take(ctx.h, out.ctypes.data, calls.ctypes.data, nc, text.ctypes.data, nt, kmers.ctypes.data, dist.ctypes.data, ns, cov.ctypes.data, nv))
    t1 = time.perf_counter()
    nodes, tigs = np.empty(len(keys), dtype=api.TIPS_NODE_DTYPE), np.empty(nc, dtype=api.TIPS_CONTIG_DTYPE)      # (the room fgpu_stage3_detip gives it)
    first, pieces = np.empty(nc + 1, dtype=np.uint64), np.empty(nc, dtype=api.JOIN_PIECE_DTYPE)
    pfirst, number, ppieces = np.empty(nc + 1, dtype=np.uint64), np.empty(nc, dtype=np.uint32), np.empty(2 * nc, dtype=api.JOIN_PIECE_DTYPE)
    o, ti = L.TipsOut(), L.TipsInfo()
    o.nodes, o.nodes_cap, o.contigs, o.list_first, o.contigs_cap = nodes.ctypes.data, len(nodes), tigs.ctypes.data, first.ctypes.data, nc
    o.pieces, o.pieces_cap, o.print_first, o.print_number, o.print_cap = pieces.ctypes.data, nc, pfirst.ctypes.data, number.ctypes.data, nc
    o.print_pieces, o.print_pieces_cap = ppieces.ctypes.data, 2 * nc
    assert ctx.lib.fgpu_tips_plan(keys.ctypes.data, recs.ctypes.data, len(keys), out.ctypes.data, calls.ctypes.data, nc, K, MRL, C.byref(o), C.byref(ti)) == L.PLAN_OK
    t2 = time.perf_counter()
    size = host.host_detip_fasta(pfirst.ctypes.data, number.ctypes.data, o.n_print, ppieces.ctypes.data, out.ctypes.data, text.ctypes.data, K, None)
    data = np.empty(size, dtype=np.uint8)
    host.host_detip_fasta(pfirst.ctypes.data, number.ctypes.data, o.n_print, ppieces.ctypes.data, out.ctypes.data, text.ctypes.data, K, data.ctypes.data)
    t3 = time.perf_counter()
    longest = int(np.diff(pfirst[:o.n_print + 1]).max()) if o.n_print else 0
    return (1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)), data.tobytes(), ti.as_dict(), (o.n_nodes, o.n_contigs, o.n_pieces, o.n_print, o.n_print_pieces, longest)


def spread(v):
    v = sorted(v)
    return f"min {v[0]:.1f} ms, median {v[len(v) // 2]:.1f}, max {v[-1]:.1f} ({len(v)} repetitions)"


device_way(), host_way()                                          # (warm up: code objects, rocPRIM's choices, the host's pages)
d_ms, h_ms = [], []
for _ in range(REPS):                                             # the two ways in turn
    t, d_data, d_info, built = device_way()
    d_ms.append(t)
    t, h_data, h_info, sizes = host_way()
    h_ms.append(t)
assert d_data == h_data and d_info == h_info, "the two ways wrote different files"
print(f"the build: {built['totals'][0]} calls, {built['totals'][1]} text words; the file: {len(d_data)} bytes, {d_info}")
print("the graph left: %d nodes, %d contigs of %d pieces; %d records of %d pieces, the longest list %d pieces" % sizes)
print("\n## device: fgpu_stage3_detip + fgpu_stage3_fasta_take")
print("wall " + spread(d_ms))
print("\n## host: fgpu_stage3_build_take + fgpu_tips_plan + the records joined and printed on the host (C++, one thread)")
print("wall " + spread([t[0] for t in h_ms]))
for i, part in enumerate(("fgpu_stage3_build_take", "fgpu_tips_plan", "host join and print (sized, then written)")):
    print(f"  {part}: " + spread([t[1 + i] for t in h_ms]))
plan = min(t[2] for t in h_ms)
print(f"\nbyte for byte the same file; the host route's minimum over the device's: {min(t[0] for t in h_ms) / min(d_ms):.2f} x; "
      f"the plan (the same call in both) is {100 * plan / min(d_ms):.0f} % of the device call's minimum")

ctx.stage3_build(MRL, take=False)
ctx.profile_enable(True)
ctx.kernel_times_reset()
t0 = now()
ctx.stage3_detip(MRL)
wall = 1e3 * (now() - t0)
kt = {k_: v for k_, v in ctx.kernel_times().items() if k_.startswith(("s3f_", "s3j_"))}
ctx.profile_enable(False)
total = sum(v[1] for v in kt.values())
print(f"\n## kernels of one more device call with events on (wall {wall:.1f} ms, the join and emission kernels {total:.2f} ms; the rest is the two record arrays' way to "
      "the host, the plan on the host, the lists' way back, rocPRIM's scan and the file's way to the host)")
for k_, (launches, t) in sorted(kt.items()):
    print(f"  {k_:18s} {launches:3d} launch(es) {t:8.3f} ms  {100 * t / total:5.1f} % of the kernels, {100 * t / wall:5.1f} % of the call")
ctx.close()
