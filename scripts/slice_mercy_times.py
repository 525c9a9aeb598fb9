"""What --mercy costs under filter slices, per rank, on ONE MI355X: BASELINE config 2's shape (tests/golden/fullsize.json: k, filter size, hash
count, genome, read generator) with every THIN-th read kept -- low coverage, where --mercy has work to do -- on N slices side by side.

Sliced pass (the five-step protocol of faucet_gpu.h): the N contexts in lockstep -- batch, OR of its fail plane across the contexts, probe --
then the OR of the miss planes, commit, end.  Yardstick: the plain one-context --mercy pass over the same batches.  The two alternate in one
process, one warm-up and REPS repetitions; the kernel times are the library's own (HIP events around every launch, fgpu_kernel_times), summed
over the batches of a pass, the minimum over the repetitions printed beside all of them.  The concatenated slices are compared with the plain
pass' filters in the same run.  This is ranks IN TURN on one device -- what one rank's kernels cost -- not a scaling number: no link is crossed.

    timeout -k 10 600 python scripts/slice_mercy_times.py [N]        (default 4; THIN=10 REPS=3 BATCH_READS=250000)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from faucet_amd import _lib as L  # noqa: E402
from faucet_amd import api, sharded  # noqa: E402
from faucet_amd import synth_det as sd  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4
THIN = int(os.environ.get("THIN", "10"))
REPS = int(os.environ.get("REPS", "3"))
BATCH_READS = int(os.environ.get("BATCH_READS", "250000"))
fx = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "fullsize.json")))["config2"]
c = fx["params"]
dev = torch.device("cuda", 0)
tai, nh = fx["tai"], fx["n_hash"]
genome = sd.make_genome(c["genome"], c["genome_seed"], dev)
reads = sd.make_reads(genome, c["reads"], c["read_len"], c["err"], c["read_seed"], dev)[::THIN].contiguous()
del genome
n_reads = reads.shape[0]
batches = bench.device_batches(reads, BATCH_READS)
coverage = n_reads * c["read_len"] / c["genome"]

SLICED = ["slice_mark", "slice_resolve", "slice_mercy_probe", "slice_commit", "slice_mercy_commit", "slice_carry_update"]
PLAIN = ["load_mark", "load_resolve", "load_mercy", "carry_update"]


def or_across(ctxs, planes):
    for p, nb in planes[1:]:
        ctxs[0].bitmap_or(planes[0][0], p, nb)
    ctxs[0].synchronize()
    for ctx, (p, nb) in zip(ctxs[1:], planes[1:]):
        ctx.bitmap_or(p, planes[0][0], nb)
        ctx.synchronize()


def sliced_pass(ctxs, bounds):
    for ctx, (lo, hi) in zip(ctxs, bounds):
        ctx.kernel_times_reset()
        ctx.load_slice_mercy_begin(lo, hi)
    for b in batches:
        for ctx in ctxs:
            ctx.load_slice_batch(b)
        for ctx in ctxs:
            ctx.synchronize()
        or_across(ctxs, [ctx.load_slice_plane(ctx.load_slice_state()[2] - 1) for ctx in ctxs])
        for ctx in ctxs:
            ctx.load_slice_mercy_probe()
    for ctx in ctxs:
        ctx.synchronize()
    for i in range(ctxs[0].load_slice_state()[2]):
        or_across(ctxs, [ctx.load_slice_mercy_planes(i) for ctx in ctxs])
    stats = []
    for ctx in ctxs:
        ctx.load_slice_commit()
        stats.append(ctx.load_slice_end())
        ctx.synchronize()
    return stats, [{k: ctx.kernel_times().get(k, (0, 0.0))[1] for k in SLICED} for ctx in ctxs]


def plain_pass(ctx):
    ctx.kernel_times_reset()
    ctx.load_begin()
    for b in batches:
        ctx.load_batch(b)
    st = ctx.load_end()
    ctx.synchronize()
    return st, {k: ctx.kernel_times().get(k, (0, 0.0))[1] for k in PLAIN}


bounds = [(lo * 8, hi * 8) for lo, hi in sharded._slices(tai // 8, N, 64)]
ctxs = [api.Context(c["k"], tai, nh, mercy=True, profile=True) for _ in range(N)]
plain = api.Context(c["k"], tai, nh, mercy=True, profile=True)
runs_s, runs_p = [], []
ok = None
for rep in range(1 + REPS):                      # rep 0: the warm-up, which also compares the filters
    stats, ts = sliced_pass(ctxs, bounds)
    st, tp = plain_pass(plain)
    if rep == 0:
        ok = all(s["to_bloo2"] == st["to_bloo2"] and s["kmers"] == st["kmers"] for s in stats)
        for which in (L.BLOO1, L.BLOO2):
            want = torch.as_tensor(sharded._DevView(*plain.bloom_devptr(which)), device=dev)
            for ctx, (lo, hi) in zip(ctxs, bounds):
                got = torch.as_tensor(sharded._DevView(*ctx.bloom_devptr(which)), device=dev)
                ok = ok and bool(torch.equal(got[lo // 8:hi // 8], want[lo // 8:hi // 8]))
        diag = [ctx.diag_slice_mercy() for ctx in ctxs]
    else:
        runs_s.append(ts)
        runs_p.append(tp)

best = lambda v: min(v)      # noqa: E731
fmt = lambda v: " ".join(f"{x:.2f}" for x in v)      # noqa: E731
print(f"config 2's shape, every {THIN}th read: {n_reads} reads x {c['read_len']} bp ({coverage:.1f}x), {len(batches)} batches, 2^{tai.bit_length() - 1} bits, "
      f"{nh} hash functions; {st['kmers']} windows, {diag[0][0]} probed ({100.0 * diag[0][0] / st['kmers']:.0f} %), tests and runs {diag[0][1:]}; "
      f"filters and counts {'EQUAL' if ok else 'DIFFER FROM'} the plain --mercy pass'", flush=True)
print(f"kernel ms per pass, minimum of {REPS} (all repetitions in brackets); N = {N} contexts side by side, ranks in turn on one device")
rows = []
for r in range(N):
    per = {k: [run[r][k] for run in runs_s] for k in SLICED}
    mr = [a + b for a, b in zip(per["slice_mark"], per["slice_resolve"])]
    cm = [a + b for a, b in zip(per["slice_commit"], per["slice_mercy_commit"])]
    rows.append((best(mr), best(per["slice_mercy_probe"]), best(per["slice_commit"]), best(per["slice_mercy_commit"])))
    print(f"  rank {r}: mark + resolve {best(mr):.2f} [{fmt(mr)}] | probe {best(per['slice_mercy_probe']):.2f} [{fmt(per['slice_mercy_probe'])}] | "
          f"commit {best(per['slice_commit']):.2f} + mercy commit {best(per['slice_mercy_commit']):.2f} [{fmt(cm)}] | carry update {best(per['slice_carry_update']):.2f}")
pm = [run["load_mark"] + run["load_resolve"] for run in runs_p]
pl = [run["load_mercy"] for run in runs_p]
print(f"  plain pass, one context: mark + resolve {best(pm):.2f} [{fmt(pm)}] | load_mercy {best(pl):.2f} [{fmt(pl)}] | carry update "
      f"{best([run['carry_update'] for run in runs_p]):.2f}")
for ctx in ctxs + [plain]:
    ctx.close()
