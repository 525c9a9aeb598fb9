"""What do whole getContig chains on the device (fgpu_stage3_contigs) cost beside chaining fgpu_stage3_find_neighbors on the host, the only way
before?  (GPU box; one GPU; measurement, no bar.)

BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31 -- loaded and scanned once; the scan's own junction map
handed to Stage 3.  Then the two batches a graph build asks for: every start of buildBranchingPaths, every start of buildLinearRegions
(faucet_amd/stage3.py; on the map as it stands -- the reference kills the complex junctions in between, which is the caller's business).

  device   api.Context.stage3_contigs(raw=True): ONE call per batch; wall time with the arrays taken to the host, and the library's own kernel
           times of one more call with events on (the follower's share of the call says whether pointer doubling would be worth having)
  host     stage3.NeighborWalker.contigs over Context.stage3_find_neighbors(contigs=True): one device call per chain segment, the strings down
           and the bookkeeping in Python, on a SAMPLE of the starts (it is per-chain Python; the whole batch would take minutes), and the
           device's call on the same sample, chain for chain equal

    python scripts/stage3_contig_times.py [sample] > profiles/stage3_contigs.txt"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from faucet_amd import api, stage3  # noqa: E402

SAMPLE = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
K, MRL = 31, 100
dev = torch.device("cuda", 0)
n, E, S = 10_000_000, 100_000_000, 20_000_000
tai, nh = api.load_filter_shape(E, S)
reads = bench.make_reads(bench.make_genome(20_000_000, 2, dev), n, 100, 0.01, 1000, dev)
ctx = api.Context(K, tai, nh)
lst, sst, b2, keys, recs = bench.step_single(ctx, bench.device_batches(reads, bench.batch_bounds(n, 1_000_000, 2)))
keys, recs = np.asarray(keys), np.asarray(recs)
del reads
t0 = time.perf_counter()
ctx.stage3_set_junctions(keys, recs)
paths = (recs["cov"] > 0).sum(axis=1)
print(f"config 2's scanned map: {len(keys)} junctions ({int((paths > 1).sum())} with more than one path out, {int((paths == 1).sum())} with one), "
      f"set in {1e3 * (time.perf_counter() - t0):.1f} ms; max_read_length {MRL}", flush=True)
walker = stage3.NeighborWalker(ctx, keys, recs, K, MRL)
rng = np.random.default_rng(5)


def device(starts, idx):
    ctx.synchronize()
    t0 = time.perf_counter()
    res = ctx.stage3_contigs(starts, idx, MRL, raw=True)
    return 1e3 * (time.perf_counter() - t0), res


def host_find(km, ix):
    got, _, strings = ctx.stage3_find_neighbors(km, ix, MRL, contigs=True)
    return got, strings


for name, (starts, idx) in (("buildBranchingPaths", stage3.branching_starts(keys, recs, K)), ("buildLinearRegions", stage3.linear_starts(keys, recs))):
    print(f"\n## {name}: {len(starts)} starts")
    if not len(starts):
        continue
    device(starts[:1000], idx[:1000])                                          # (warm up)
    runs = [device(starts, idx) for _ in range(3)]
    ms = sorted(r[0] for r in runs)
    out, text, kmers, dist, cov, probes = runs[-1][1]
    st = out["status"]
    print(f"device, one call: {ms[1]:.1f} ms (median of 3; {ms[0]:.1f} .. {ms[2]:.1f}), {len(starts) / ms[1] * 1e3:.3g} chains/s; "
          f"{int(out['n_seg'].sum())} segments, {int(out['len'].sum())} bases, {probes} getValidJExtension evaluations")
    print(f"status 0 / 1 / 2 / 3: {[int((st == v).sum()) for v in range(4)]}; longest chain {int(out['n_seg'].max())} segments, longest string {int(out['len'].max())} bases; "
          f"chains of 2 or more segments: {int((out['n_seg'] >= 2).sum())}")
    ctx.profile_enable(True)
    ctx.kernel_times_reset()
    wall, _ = device(starts, idx)
    kt = {k_: v for k_, v in ctx.kernel_times().items() if k_.startswith("s3c_")}
    ctx.profile_enable(False)
    total = sum(v[1] for v in kt.values())
    print(f"kernels of one call with events on (wall {wall:.1f} ms, kernels {total:.1f} ms):")
    for k_, (launches, t) in sorted(kt.items()):
        print(f"  {k_:14s} {launches} launch(es) {t:9.2f} ms  {100 * t / total:5.1f} % of the kernels, {100 * t / wall:5.1f} % of the call")
    share = kt.get("s3c_follow", (0, 0.0))[1] / wall
    print(f"the follower (both passes) takes {100 * share:.1f} % of the call: " + ("MORE than half -- pointer doubling is worth building" if share > 0.5 else
          "less than half -- a sequential follower is enough here, pointer doubling is not built"))
    pick = np.sort(rng.choice(len(starts), size=min(SAMPLE, len(starts)), replace=False))
    ctx.synchronize()
    t0 = time.perf_counter()
    want = walker.contigs(starts[pick], idx[pick], find=host_find)
    host_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    got = ctx.stage3_contigs(starts[pick], idx[pick], MRL)
    dev_ms = 1e3 * (time.perf_counter() - t0)
    for i, w in enumerate(want):
        g = got[0][i]
        assert int(g["status"]) == w["status"], (i, w)
        assert (int(g["ind1"]), int(g["ind2"]), int(g["end_kmer"]), int(g["end_node"]), got[1][i], got[2][i].tolist(), got[3][i].tolist(), got[4][i].tolist()) == \
            (w["ind1"], w["ind2"], w["end_kmer"], w["end_node"], w["string"], w["distances"], w["coverages"], w["kills"]), (i, w)
    print(f"sample of {len(pick)} starts, chain for chain equal: host chaining over fgpu_stage3_find_neighbors {host_ms:.1f} ms in {walker.rounds} rounds of calls; "
          f"stage3_contigs with the strings decoded {dev_ms:.1f} ms ({host_ms / dev_ms:.1f} x)")
ctx.close()
