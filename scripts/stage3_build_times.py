"""What does JunctionMap::buildContigGraph's whole contig list in one device call (fgpu_stage3_build) cost, how many rounds does its fixed point
need on a real map, and how many calls does a round walk again?  (GPU box; one GPU; measurement, no bar.)

BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31 -- loaded and scanned once; the scan's own junction map
handed to Stage 3 (the map of profiles/stage3_contigs.txt).

  build    api.Context.stage3_build(raw=True): ONE call; wall time with the arrays taken to the host, rounds, getContig evaluations per round,
           getValidJExtension evaluations, and the library's own kernel times of one more call with events on
  static   the two fgpu_stage3_contigs calls of scripts/stage3_contig_times.py on the same map (every branching start, every linear start).
           They do LESS: each answers on the map as it was set -- no kills, no claims, no destroyComplexJunctions between the two -- so their
           contigs are not the reference's list; they are here as the price of the walks alone
  serial   stage3.build_serial, the literal loop (one fgpu_stage3_contigs call per getContig, the map set again after every kill), on the
           FIRST calls of the build only, checked against the build's, and EXTRAPOLATED to all calls in proportion -- an estimate, labelled so

    python scripts/stage3_build_times.py [serial calls] > profiles/stage3_build.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from faucet_amd import api, stage3  # noqa: E402

SERIAL = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
K, MRL = 31, 100
dev = torch.device("cuda", 0)
n, E, S = 10_000_000, 100_000_000, 20_000_000
tai, nh = api.load_filter_shape(E, S)
reads = bench.make_reads(bench.make_genome(20_000_000, 2, dev), n, 100, 0.01, 1000, dev)
ctx = api.Context(K, tai, nh)
lst, sst, b2, keys, recs = bench.step_single(ctx, bench.device_batches(reads, bench.batch_bounds(n, 1_000_000, 2)))
keys, recs = np.asarray(keys), np.asarray(recs)
del reads
ctx.stage3_set_junctions(keys, recs)
paths = (recs["cov"] > 0).sum(axis=1)
print(f"config 2's scanned map: {len(keys)} junctions ({int((paths > 1).sum())} with more than one path out, {int((paths == 1).sum())} with one); "
      f"max_read_length {MRL}", flush=True)


def timed(f):
    ctx.synchronize()
    t0 = time.perf_counter()
    res = f()
    return 1e3 * (time.perf_counter() - t0), res


print("\n## build: fgpu_stage3_build + fgpu_stage3_build_take, one call")
timed(lambda: ctx.stage3_build(MRL, raw=True))                               # (warm up)
runs = [timed(lambda: ctx.stage3_build(MRL, raw=True)) for _ in range(3)]
ms = sorted(r[0] for r in runs)
out, calls, text, kmers, dist, cov, info = runs[-1][1]
print(f"wall {ms[1]:.1f} ms (median of 3; {ms[0]:.1f} .. {ms[2]:.1f}); status {info['status']}; {info['calls_possible']} time slots, {len(out)} calls made: "
      f"{[int((calls['phase'] == p).sum()) for p in range(3)]} branching / linear forward / linear backward; {int(out['n_seg'].sum())} segments, {int(out['len'].sum())} bases")
print(f"rounds {info['rounds']} (behind the last one nothing is left to evaluate); getContig evaluations {info['rewalked']}, {info['rewalked'] / max(len(out), 1):.3f} per call made; "
      f"getValidJExtension evaluations {info['probes']}; junction-map hits recorded {info['table_hits']}, their array regrown {info['regrown']} time(s)")
print(f"evaluations per round: {info['rewalked_by_round']}" + (" ... (the first rounds)" if info["rounds"] > len(info["rewalked_by_round"]) else ""))
ctx.profile_enable(True)
ctx.kernel_times_reset()
wall, _ = timed(lambda: ctx.stage3_build(MRL, raw=True))
kt = {k_: v for k_, v in ctx.kernel_times().items() if k_.startswith("s3b_")}
ctx.profile_enable(False)
total = sum(v[1] for v in kt.values())
print(f"kernels of one call with events on (wall {wall:.1f} ms, kernels {total:.1f} ms):")
for k_, (launches, t) in sorted(kt.items()):
    print(f"  {k_:12s} {launches:5d} launch(es) {t:9.2f} ms  {100 * t / total:5.1f} % of the kernels, {100 * t / wall:5.1f} % of the call")

print("\n## static: the two fgpu_stage3_contigs calls on the map as set (they do less: no kills, no claims, no destroyComplexJunctions)")
static_ms = 0.0
for name, (starts, idx) in (("buildBranchingPaths", stage3.branching_starts(keys, recs, K)), ("buildLinearRegions", stage3.linear_starts(keys, recs))):
    timed(lambda: ctx.stage3_contigs(starts[:1000], idx[:1000], MRL, raw=True))
    t = sorted(timed(lambda: ctx.stage3_contigs(starts, idx, MRL, raw=True))[0] for _ in range(3))
    static_ms += t[1]
    print(f"{name}: {len(starts)} starts, {t[1]:.1f} ms (median of 3; {t[0]:.1f} .. {t[2]:.1f})")
print(f"both: {static_ms:.1f} ms; the build takes {ms[1] / static_ms:.2f} x that")

print(f"\n## serial: stage3.build_serial, the first {SERIAL} calls")
t, (want, status, sets) = timed(lambda: stage3.build_serial(ctx, keys, recs, K, MRL, limit=SERIAL))
ctx.stage3_set_junctions(keys, recs)
chars = np.frombuffer(b"ACTG", dtype=np.uint8)
for i, w in enumerate(want):
    g, h = out[i], calls[i]
    s, ns, v = int(g["seg_first"]), int(g["n_seg"]), int(g["cov_first"])
    words = text[int(g["text_word"]):int(g["text_word"]) + (int(g["len"]) + 31) // 32]
    string = chars[((words[:, None] >> (2 * np.arange(32, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)].reshape(-1)[:int(g["len"])].tobytes().decode()
    got = dict(phase=int(h["phase"]), start=int(h["start_kmer"]), ind1=int(g["ind1"]), ind2=int(g["ind2"]), end_kmer=int(g["end_kmer"]), end_node=int(g["end_node"]),
               string=string, distances=dist[s:s + ns].tolist(), coverages=cov[v:v + int(g["n_cov"])].tolist(), kills=kmers[s:s + max(ns - 1, 0)].tolist(),
               far_kmer=int(h["far_kmer"]), far_is_junction=int(h["far_is_junction"]), far_is_start=int(h["far_is_start"]))
    assert got == w, (i, got, w)
print(f"{len(want)} calls, call for call equal to the build's first {len(want)}: {t:.0f} ms, the map set {sets} times; {t / max(len(want), 1):.1f} ms per call")
print(f"EXTRAPOLATED to the build's {len(out)} calls in proportion: {t / max(len(want), 1) * len(out) / 1e3:.0f} s -- an estimate, not a measurement; "
      f"the build's one call: {ms[1] / 1e3:.3f} s")
ctx.close()
