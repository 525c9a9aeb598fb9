"""What does ContigGraph::removeChimerasAndClean and the contig file behind it cost on the device's build, now that the graph lives between the
steps (fgpu_stage3_dechimera: fgpu_stage3_cov_calls on the build where it lies, the summaries folded into the live graph fgpu_stage3_detip left,
the step, fgpu_stage3_join of the print records, fgpu_stage3_fasta_joined; then fgpu_stage3_fasta_take), and what would the same file cost on the
host, from the build?  (GPU box; one GPU; measurement, no bar: the parent commit cannot do the step at all.)

BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31 -- loaded and scanned once; the scan's own junction map
handed to Stage 3 (the map of profiles/stage3_build.txt, stage3_raw_contigs.txt and stage3_detip.txt).  Every repetition starts from a build that
has just finished and is still on the device and, for the device's way, from a fgpu_stage3_detip on it (neither timed); the two ways take turns.

  device  fgpu_stage3_dechimera + fgpu_stage3_fasta_take: wall time, host clock around calls that end synchronised, no events.  Its four parts,
          each under a clock of its own in every repetition:
            summaries  fgpu_stage3_cov_calls on the same build, the same call once more (wall)
            plan step  what the call does on the host, in scripts/micro/host_dechimera.cpp over clean_graph.h itself, on a graph made and detipped
                       without coverages as the context holds it: the summaries folded into the live contigs, removeChimerasAndClean,
                       printContigs' two passes -- three clocks
            join       fgpu_stage3_join of the same print records over the build where it lies (wall: the build's records to the host, the host's
                       check of the lists, the lists to the device, three kernels, the sums back)
            emission   fgpu_stage3_fasta_joined of the joined text where it lies, and fgpu_stage3_fasta_take (wall, each)
          and what of the call's wall time the four do not account for
  host    fgpu_stage3_build_take (all six arrays to the host), the summaries by numpy, fgpu_chimera_plan FROM THE BUILD (graph, detip, chimeras,
          print records), and the print records joined and printed on the host in C++ (scripts/micro/host_detip.cpp, one thread)
  step    the chimera step now that the graph is not made again (the plan step's three clocks) beside what making the graph and detipping it
          costs in the same program (two more clocks), which a step that started from the build would pay again
Both files are compared byte for byte.

    python scripts/stage3_dechimera_times.py > profiles/stage3_dechimera.txt"""
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

REPS = int(os.environ.get("DECHIMERA_REPS", "5"))
K, MRL = 31, 100
tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "host_detip.so")
subprocess.run(["g++", "-std=c++11", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "scripts", "micro", "host_detip.cpp"), "-o", so], check=True)
host = C.CDLL(so)
host.host_detip_fasta.restype = C.c_uint64
host.host_detip_fasta.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
so2 = os.path.join(tmp, "host_dechimera.so")
subprocess.run(["g++", "-std=c++11", "-O3", "-shared", "-fPIC", os.path.join(ROOT, "scripts", "micro", "host_dechimera.cpp"), "-o", so2], check=True)   # (-O3: the library's)
steps = C.CDLL(so2)
steps.host_dechimera_times.restype = C.c_int
steps.host_dechimera_times.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_double),
                                       C.POINTER(C.c_uint64)]

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
    ctx.stage3_detip(MRL)
    t0 = now()
    data, info = ctx.stage3_dechimera()
    t1 = now()
    ctx.stage3_cov_calls()                                        # (once, so that the timed one is not the first)
    t2 = now()
    cov = ctx.stage3_cov_calls()
    t3 = now()
    return 1e3 * (t1 - t0), 1e3 * (t3 - t2), data, info, built, cov


def summaries_by_numpy(out, cov):
    s = np.zeros(len(out), dtype=api.COV_SUMMARY_DTYPE)
    first, m = out["cov_first"].astype(np.int64), out["n_cov"].astype(np.int64)
    if len(out):
        total = np.concatenate([[0], np.cumsum(cov, dtype=np.uint64)])
        s["sum"], s["n"] = total[first + m] - total[first], m
        s["first"], s["last"] = cov[first], cov[first + m - 1]
    return s


def host_way():
    built = ctx.stage3_build(MRL, take=False)
    nc, nt, ns, nv = built["totals"]
    t0 = now()
    out, calls = np.empty(nc, dtype=api.CONTIG_DTYPE), np.empty(nc, dtype=api.BUILD_DTYPE)
    text, kmers, dist, cov = np.empty(nt, dtype=np.uint64), np.empty(ns, dtype=np.uint64), np.empty(ns, dtype=np.uint8), np.empty(nv, dtype=np.uint8)
    ctx._c(ctx.lib.fgpu_stage3_build_take(ctx.h, out.ctypes.data, calls.ctypes.data, nc, text.ctypes.data, nt, kmers.ctypes.data, dist.ctypes.data, ns, cov.ctypes.data, nv))
    t1 = time.perf_counter()
    sums = summaries_by_numpy(out, cov)
    t2 = time.perf_counter()
    nodes, tigs = np.empty(len(keys), dtype=api.TIPS_NODE_DTYPE), np.empty(nc, dtype=api.TIPS_CONTIG_DTYPE)      # (the room fgpu_stage3_detip gives its plan)
    first, pieces = np.empty(nc + 1, dtype=np.uint64), np.empty(nc, dtype=api.JOIN_PIECE_DTYPE)
    pfirst, number, ppieces = np.empty(nc + 1, dtype=np.uint64), np.empty(nc, dtype=np.uint32), np.empty(2 * nc, dtype=api.JOIN_PIECE_DTYPE)
    o, ti, ci = L.TipsOut(), L.TipsInfo(), L.ChimeraInfo()
    o.nodes, o.nodes_cap, o.contigs, o.list_first, o.contigs_cap = nodes.ctypes.data, len(nodes), tigs.ctypes.data, first.ctypes.data, nc
    o.pieces, o.pieces_cap, o.print_first, o.print_number, o.print_cap = pieces.ctypes.data, nc, pfirst.ctypes.data, number.ctypes.data, nc
    o.print_pieces, o.print_pieces_cap = ppieces.ctypes.data, 2 * nc
    assert ctx.lib.fgpu_chimera_plan(keys.ctypes.data, recs.ctypes.data, len(keys), out.ctypes.data, calls.ctypes.data, nc, sums.ctypes.data, K, MRL, C.byref(o), C.byref(ti),
                                     C.byref(ci)) == L.PLAN_OK
    t3 = time.perf_counter()
    size = host.host_detip_fasta(pfirst.ctypes.data, number.ctypes.data, o.n_print, ppieces.ctypes.data, out.ctypes.data, text.ctypes.data, K, None)
    data = np.empty(size, dtype=np.uint8)
    host.host_detip_fasta(pfirst.ctypes.data, number.ctypes.data, o.n_print, ppieces.ctypes.data, out.ctypes.data, text.ctypes.data, K, data.ctypes.data)
    t4 = time.perf_counter()
    sizes = (o.n_nodes, o.n_contigs, o.n_pieces, o.n_print, o.n_print_pieces, int(np.diff(pfirst[:o.n_print + 1]).max()) if o.n_print else 0)
    parts = (1e3 * (t4 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t4 - t3))
    # ---- the device call's host part, clock by clock, over the same arrays (graph, detip | set_cov, the step, print_records)
    ms, counts = (C.c_double * 5)(), (C.c_uint64 * 3)()
    assert steps.host_dechimera_times(keys.ctypes.data, recs.ctypes.data, len(keys), out.ctypes.data, calls.ctypes.data, nc, sums.ctypes.data, K, MRL, ms, counts) == L.PLAN_OK
    assert list(counts) == [ci.removed, ci.print.nodes, ci.print.records]
    # ---- the device call's join and emission, each a call of its own over the same print records, on a build that lies on the device again
    assert ctx.stage3_build(MRL, take=False)["totals"] == built["totals"]
    n_print, joined, totals, nbytes = int(o.n_print), np.empty(int(o.n_print), dtype=api.JOINED_DTYPE), (C.c_uint64 * 3)(), C.c_uint64(0)
    j0 = now()
    ctx._c(ctx.lib.fgpu_stage3_join(ctx.h, pfirst.ctypes.data, n_print, ppieces.ctypes.data, int(o.n_print_pieces), None, 0, None, 0, None, 0, None, 0, joined.ctypes.data, totals))
    j1 = now()
    ctx._c(ctx.lib.fgpu_stage3_fasta_joined(ctx.h, joined.ctypes.data, number.ctypes.data, n_print, None, 0, C.byref(nbytes)))
    j2 = now()
    printed = ctx.stage3_fasta_take(nbytes.value)
    j3 = now()
    assert printed == data.tobytes(), "the join and the emission called apart wrote another file"
    return parts, data.tobytes(), ci.as_dict(), sizes, sums, list(ms), (1e3 * (j1 - j0), 1e3 * (j2 - j1), 1e3 * (j3 - j2))


def spread(v):
    v = sorted(v)
    return f"min {v[0]:.1f} ms, median {v[len(v) // 2]:.1f}, max {v[-1]:.1f} ({len(v)} repetitions)"


device_way(), host_way()                                          # (warm up: code objects, rocPRIM's choices, the host's pages)
d_ms, s_ms, h_ms, p_ms, j_ms = [], [], [], [], []
for _ in range(REPS):                                             # the two ways in turn
    t, ts, d_data, d_info, built, d_cov = device_way()
    d_ms.append(t)
    s_ms.append(ts)
    t, h_data, h_info, sizes, h_cov, tp, tj = host_way()
    h_ms.append(t)
    p_ms.append(tp)
    j_ms.append(tj)
assert d_data == h_data and d_info == h_info, "the two ways wrote different files"
assert d_cov.tobytes() == h_cov.tobytes(), "the device's summaries are not numpy's"
print(f"the build: {built['totals'][0]} calls, {built['totals'][3]} coverage entries; the file: {len(d_data)} bytes, {d_info}")
print("the graph left: %d nodes, %d contigs of %d pieces; %d records of %d pieces, the longest list %d pieces" % sizes)
print("\n## device: fgpu_stage3_dechimera + fgpu_stage3_fasta_take, on the live graph fgpu_stage3_detip left")
print("wall " + spread(d_ms))
plan_ms = [t[2] + t[3] + t[4] for t in p_ms]
emit_ms = [t[1] + t[2] for t in j_ms]
print("  summaries: fgpu_stage3_cov_calls (the same call once more, alone): " + spread(s_ms))
print("  plan step: the summaries folded, removeChimerasAndClean, printContigs' two passes (host program over clean_graph.h): " + spread(plan_ms))
for i, part in ((2, "set_cov (the summaries folded into the live contigs)"), (3, "remove_chimeras_and_clean"), (4, "print_records (with its room)")):
    print(f"    {part}: " + spread([t[i] for t in p_ms]))
print("  join: fgpu_stage3_join of the print records over the build where it lies (a call of its own): " + spread([t[0] for t in j_ms]))
print("  emission: fgpu_stage3_fasta_joined + fgpu_stage3_fasta_take (calls of their own): " + spread(emit_ms))
print("    fgpu_stage3_fasta_joined: " + spread([t[1] for t in j_ms]))
print("    fgpu_stage3_fasta_take: " + spread([t[2] for t in j_ms]))
med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
parts_sum = med(s_ms) + med(plan_ms) + med([t[0] for t in j_ms]) + med(emit_ms)
print(f"  medians: {med(s_ms):.1f} + {med(plan_ms):.1f} + {med([t[0] for t in j_ms]):.1f} + {med(emit_ms):.1f} = {parts_sum:.1f} ms of the call's {med(d_ms):.1f} ms; "
      f"{med(d_ms) - parts_sum:+.1f} ms are not accounted for (the parts were timed apart from the call: the summaries' vector, the info, the order of the host's pages)")
print("\n## host, from the build: fgpu_stage3_build_take + summaries + fgpu_chimera_plan + the records joined and printed on the host (C++, one thread)")
print("wall " + spread([t[0] for t in h_ms]))
for i, part in enumerate(("fgpu_stage3_build_take", "summaries by numpy", "fgpu_chimera_plan (graph, detip, chimeras, print records)", "host join and print (sized, then written)")):
    print(f"  {part}: " + spread([t[1 + i] for t in h_ms]))
print(f"\nbyte for byte the same file; the host route's minimum over the device's: {min(t[0] for t in h_ms) / min(d_ms):.2f} x")
print("\n## the chimera step now that the graph is not made again, beside what a step that started from the build would pay first (the same host program, a clock each)")
print("  the graph of the build (of_build): " + spread([t[0] for t in p_ms]))
print("  delete_tips_and_clean: " + spread([t[1] for t in p_ms]))
print("  set_cov + remove_chimeras_and_clean (the step on the live graph): " + spread([t[2] + t[3] for t in p_ms]))
again = med([t[0] + t[1] for t in p_ms])
print(f"  medians: {med([t[2] + t[3] for t in p_ms]):.1f} ms for the step against {again:.1f} ms for the graph and the detip in front of it, "
      f"of fgpu_chimera_plan's {med([t[3] for t in h_ms]):.1f} ms")

ctx.stage3_build(MRL, take=False)
ctx.stage3_detip(MRL)
ctx.profile_enable(True)
ctx.kernel_times_reset()
t0 = now()
ctx.stage3_dechimera()
wall = 1e3 * (now() - t0)
kt = {k_: v for k_, v in ctx.kernel_times().items() if k_.startswith(("s3f_", "s3j_"))}
ctx.profile_enable(False)
total = sum(v[1] for v in kt.values())
join = sum(v[1] for k_, v in kt.items() if k_.startswith("s3j_") and k_ != "s3j_cov_calls")
emit = sum(v[1] for k_, v in kt.items() if k_.startswith("s3f_"))
summ = kt.get("s3j_cov_calls", (0, 0.0))[1]
print(f"\n## one more device call with events on: wall {wall:.1f} ms = summaries' kernel {summ:.3f} ms + join kernels {join:.3f} ms + emission kernels {emit:.3f} ms + "
      f"{wall - total:.1f} ms for the host's work and the copies, which the parts above time one by one")
for k_, (launches, t) in sorted(kt.items()):
    print(f"  {k_:18s} {launches:3d} launch(es) {t:8.3f} ms  {100 * t / total:5.1f} % of the kernels, {100 * t / wall:5.1f} % of the call")
ctx.close()
