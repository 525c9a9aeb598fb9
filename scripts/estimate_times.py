"""What does pass 0 (fgpu_estimate_*: the sketch -estimated_kmers and -singletons are made from) cost beside pass 1?  (GPU box; one GPU;
measurement, no bar.)

BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31, resident in HBM, batches of 1 M reads -- through ONE context:
the estimate pass at the default 2^30 cells per level (begin to end: 1 GiB of planes allocated, cleared, filled, counted and freed) and pass 1
on the filters the command line would size (fgpu_load_begin to fgpu_load_end), in turn in the same process, three of each after one of each to
warm up; wall time per pass with the device synchronised, median of 3 (min .. max).  The expectation -- one hash and at most two atomics per
k-mer cost no more than pass 1's n_hash loads and atomics -- is what this measures.
    python scripts/estimate_times.py [r_bits] > profiles/estimate_times.txt"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from faucet_amd import api  # noqa: E402

R_BITS = int(sys.argv[1]) if len(sys.argv) > 1 else 0
dev = torch.device("cuda", 0)
n, E, S = 10_000_000, 100_000_000, 20_000_000
tai, nh = api.load_filter_shape(E, S)
reads = bench.make_reads(bench.make_genome(20_000_000, 2, dev), n, 100, 0.01, 1000, dev)
batches = bench.device_batches(reads, bench.batch_bounds(n, 1_000_000, 2))
ctx = api.Context(31, tai, nh)


def estimate():
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.estimate_begin(R_BITS)
    for b in batches:
        ctx.estimate_batch(b)
    e = ctx.estimate_end()
    return 1e3 * (time.perf_counter() - t0), e


def load():
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.load_begin()
    for b in batches:
        ctx.load_batch(b)
    st = ctx.load_end()
    return 1e3 * (time.perf_counter() - t0), st


estimate()
load()
rows = {"pass 0 (estimate)": [], "pass 1 (load)": []}
for i in range(3):
    ms, e = estimate()
    rows["pass 0 (estimate)"].append(ms)
    ms1, st = load()
    rows["pass 1 (load)"].append(ms1)
    assert e["kmers"] == st["kmers"]
    print(f"run {i}: pass 0 {ms:8.2f} ms, pass 1 {ms1:8.2f} ms", flush=True)
print(f"config 2's reads: {n} reads in {len(batches)} batches, {e['kmers']} k-mers; sketch of 2^{e['r_bits']} cells per level, solved from level {e['level']}: "
      f"F0 = {e['f0']:.0f}, f1 = {e['f1']:.0f}; filters 2^{tai.bit_length() - 1} bits x {nh} hash functions")
print("\n| pass | wall, ms (median of 3; min .. max) | k-mers/s |")
print("|---|---|---|")
for name, v in rows.items():
    v = sorted(v)
    print(f"| {name} | {v[1]:.2f} ({v[0]:.2f} .. {v[2]:.2f}) | {e['kmers'] / v[1] * 1e3:.3g} |")
ctx.close()
