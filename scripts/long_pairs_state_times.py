"""What does the sparse state of the long pair filter cost beside the dense one?  (GPU box; one GPU; measurement, no bar.)

BASELINE config 3's shape -- 2.5 M pairs of 100-base reads of a 4.6 Mb genome with planted repeats, k = 31, both pair filters sized as the
command line sizes them -- scanned through ONE context, the long pair filter's first-set times dense (4 bytes per filter bit,
FGPU_LONG_PAIRS_FILTER) and sparse (a table per batch, FGPU_LONG_PAIRS_FILTER_SPARSE) in turn in the same process, three scans each.  Per scan:
the `long_pairs` kernel time from fgpu_kernel_times (HIP events around every launch of csrc/pairs.hip) and the wall time of the scan, from
scan_begin to the downloaded filter.  Both forms must give the same filter and fgpu_diag_long_pairs figures.
    python scripts/long_pairs_state_times.py [batch_reads]"""
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from faucet_amd import api  # noqa: E402
from faucet_amd import synth_det as sd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "fullsize.json")) as f:
    c = json.load(f)["config3"]["params"]
BATCH = int(sys.argv[1]) if len(sys.argv) > 1 else 625_000
dev = torch.device("cuda", 0)
g = sd.make_genome(c["genome"], c["genome_seed"], dev)
sd.plant_repeats(g, c["genome_seed"] + 100, *c["repeats"])
reads = sd.make_pairs(g, c["pairs"], c["read_len"], c["insert"][0], c["insert"][1], c["err"], c["read_seed"], dev)
tai, nh = api.load_filter_shape(c["E"], c["S"])
_, stai, snh = api.size_optimal(c["E"] // 20, np.float32(0.01))      # src/Faucet.cpp:266-283
_, ltai, lnh = api.size_optimal(c["E"] // 10, np.float32(0.01))
ctx = api.Context(c["k"], tai, nh, record_stops=True, profile=True)
batches = bench.device_batches(reads, BATCH)
ctx.load_begin()
for b in batches:
    ctx.load_batch(b)
ctx.load_end()
print(f"config 3's shape: {reads.shape[0]} reads in {len(batches)} batches of {BATCH}; long pair filter 2^{ltai.bit_length() - 1} bits x {lnh} hash functions "
      f"(dense first-set times: {4 * ltai / 2**20:.0f} MiB)")
ctx.scan_short_pairs(stai, snh, False)


def scan(mode):
    ctx.scan_long_pairs(ltai, lnh, mode)
    ctx.synchronize()
    ctx.kernel_times_reset()
    t0 = time.perf_counter()
    ctx.scan_begin()
    for b in batches:
        ctx.scan_batch(b)
    ctx.scan_end()
    bits, empty, not_empty = ctx.scan_long_pairs_download(ltai)
    wall = time.perf_counter() - t0
    launches, ms = ctx.kernel_times().get("long_pairs", (0, 0.0))
    return dict(wall_ms=1e3 * wall, kernel_ms=ms, launches=launches, digest=hashlib.sha256(bits.tobytes()).hexdigest(), counts=(empty, not_empty),
                diag=ctx.diag_long_pairs(), state=ctx.diag_long_pairs_state())


scan(2)                                   # the first use of a context: windows calibrated, the junction table grown
rows = {"dense": [], "sparse": []}
for i in range(3):
    for name, mode in (("dense", 2), ("sparse", 3)):
        r = scan(mode)
        assert r["state"]["form"] == name and r["state"]["error"] == 0, r["state"]
        rows[name].append(r)
        print(f"run {i} {name:6s}: long_pairs kernels {r['kernel_ms']:8.2f} ms in {r['launches']} launches, scan wall {r['wall_ms']:8.1f} ms; "
              f"working bytes beyond the bits {r['state']['working_bytes'] / 2**20:.1f} MiB, table slots at most {r['state']['table_slots_high']}", flush=True)
first = rows["dense"][0]
for name in rows:
    for r in rows[name]:
        assert (r["digest"], r["counts"], r["diag"]) == (first["digest"], first["counts"], first["diag"]), (name, r, first)
print(f"same filter ({first['digest'][:16]}...), pair counts {first['counts']} and diagnostics {first['diag']} in all six scans")
print("\n| first-set times | long_pairs kernels, ms (median of 3; min .. max) | scan wall, ms (median of 3; min .. max) | working bytes beyond the bits |")
print("|---|---|---|---|")
for name in ("dense", "sparse"):
    km, wm = sorted(r["kernel_ms"] for r in rows[name]), sorted(r["wall_ms"] for r in rows[name])
    print(f"| {name} | {km[1]:.2f} ({km[0]:.2f} .. {km[2]:.2f}) | {wm[1]:.1f} ({wm[0]:.1f} .. {wm[2]:.1f}) | {rows[name][-1]['state']['working_bytes'] / 2**20:.1f} MiB |")
ctx.close()
