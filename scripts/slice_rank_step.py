"""One rank of pass 1 by filter slices on its own, for profilers: rank R of N over BASELINE config 4's whole stream, slice_load + commit (on its own
fail planes: without the other ranks' the commit sets more bits than in the protocol), twice.
    rocprofv3 --kernel-trace --stats ... -- python3 scripts/slice_rank_step.py [N [R]]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from faucet_amd import api, sharded  # noqa: E402
from faucet_amd import synth_det as sd  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8
R = int(sys.argv[2]) if len(sys.argv) > 2 else N // 2
fx = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "fullsize.json")))["config4"]
c = fx["params"]
dev = torch.device("cuda", 0)
tai, nh = api.load_filter_shape(c["E"], c["S"])
genome = sd.make_genome(c["genome"], c["genome_seed"], dev)
reads = sd.make_reads(genome, c["reads"], c["read_len"], c["err"], c["read_seed"], dev)
del genome
stream = bench.device_batches(reads, bench.batch_bounds(c["reads"], 2_500_000, 2))
lo, hi = sharded._slices(tai // 8, N, 64)[R]
b = sharded.GpuShard(api.Context(c["k"], tai, nh), dev, stream_ordered=False)
out = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.slice_load(stream, lo * 8, hi * 8)
    b.ctx.synchronize()
    t1 = time.perf_counter()
    b.slice_commit()
    st = b.slice_end()
    out.append({"slice_load_ms": 1e3 * (t1 - t0), "commit_ms": 1e3 * (time.perf_counter() - t1), "kmers": st["kmers"]})
print(json.dumps({"N": N, "rank": R, "runs": out}))
