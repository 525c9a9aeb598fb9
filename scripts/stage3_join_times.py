"""What does joining the contigs of a build on the device cost (fgpu_stage3_join: the build's fgpu_contig records to the host, the lists
checked and three running sums per piece made there, the sums' way to the device, three kernels), and how far are the kernels from a plain
device copy of the bytes they move?  (GPU box; one GPU; measurement, no bar.)

Config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31 -- loaded and scanned once; the scan's own junction map handed to
Stage 3 and built (the build of profiles/stage3_build.txt), left on the device.  Two sets of lists over it:

  graph    the contigs as the reference's graph holds them when JunctionMap::buildContigGraph returns: every branching call a list of one
           piece, every linear region the list of two that utils/JunctionMap.cpp:120 joins (the backward chain reversed, then the forward one)
  chains   lists of eight consecutive contigs of at least k bases, every second one flipped: the shape collapseNode leaves behind (the pieces
           do not overlap here; the join does not ask for it)

Per set: the wall time of fgpu_stage3_join (host clock around a call that ends synchronised, no events; fgpu_stage3_join_take apart), then the
library's own kernel times of one more call with events on, and per kernel the payload it moves (output bytes, read once and written once)
against fgpu_diag_stream_copy of as many bytes.  The device's results are compared with numpy's for the `graph` set's coverages and lengths.
There is no host way to compare with that does not first take the build (fgpu_stage3_build_take, timed here as the floor under any).

    python scripts/stage3_join_times.py > profiles/stage3_join.txt"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from faucet_amd import api  # noqa: E402

REPS = 7
K, MRL = 31, 100
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
    return f"min {v[0]:.2f} ms, median {v[len(v) // 2]:.2f}, max {v[-1]:.2f} ({len(v)} repetitions)"


contigs, calls = ctx.stage3_build(MRL, raw=True)[:2]                # (only to make the lists: which calls are linear, which are long enough)
built = ctx.stage3_build(MRL, take=False)
assert built["status"] == 0 and built["totals"][0] == len(contigs)
nc = len(contigs)
print(f"the build: {nc} calls, {built['totals'][1]} text words, {built['totals'][2]} distances, {built['totals'][3]} coverages", flush=True)


def csr(sizes, call, flip):
    first = np.zeros(len(sizes) + 1, dtype=np.uint64)
    first[1:] = np.cumsum(sizes, dtype=np.uint64)
    pieces = np.zeros(len(call), dtype=api.JOIN_PIECE_DTYPE)
    pieces["call"], pieces["flip"] = call, flip
    return first, pieces


phase = calls["phase"]
backward = phase == api.BUILD_LINEAR_BACKWARD
fwd = np.flatnonzero(phase == api.BUILD_LINEAR_FORWARD)
assert len(fwd) == int(backward.sum()) and (not len(fwd) or (fwd[-1] + 1 < nc and backward[fwd + 1].all()))      # forward, then its backward
head = ~backward                                                    # a list per call that is not the backward half of a region
sizes = np.where(phase[head] == api.BUILD_LINEAR_FORWARD, 2, 1)
call = np.arange(nc, dtype=np.int64)
order = call.copy()                                                 # pieces in list order: (backward, forward) per region
order[fwd], order[fwd + 1] = fwd + 1, fwd
sets = {"graph": csr(sizes, order, backward[order].astype(np.uint32))}
long_enough = np.flatnonzero(contigs["len"] >= K)
long_enough = long_enough[:len(long_enough) // 8 * 8]
sets["chains"] = csr(np.full(len(long_enough) // 8, 8), long_enough, (np.arange(len(long_enough)) & 1).astype(np.uint32))


def join(first, pieces):
    out = np.zeros(len(first) - 1, dtype=api.JOINED_DTYPE)
    totals = (C.c_uint64 * 3)()
    t0 = now()
    ctx._c(ctx.lib.fgpu_stage3_join(ctx.h, first.ctypes.data, len(first) - 1, pieces.ctypes.data, len(pieces), None, 0, None, 0, None, 0, None, 0, out.ctypes.data, totals))
    t1 = now()
    return 1e3 * (t1 - t0), out, [int(v) for v in totals]


def take(totals):
    text, dist, cov = np.empty(totals[0], dtype=np.uint64), np.empty(totals[1], dtype=np.uint8), np.empty(totals[2], dtype=np.uint8)
    t0 = now()
    ctx._c(ctx.lib.fgpu_stage3_join_take(ctx.h, text.ctypes.data, len(text), dist.ctypes.data, len(dist), cov.ctypes.data, len(cov)))
    return 1e3 * (now() - t0), text, dist, cov


for name, (first, pieces) in sets.items():
    join(first, pieces)                                             # (warm up: code objects, the host's pages)
    ms, take_ms = [], []
    for _ in range(REPS):
        t, out, totals = join(first, pieces)
        ms.append(t)
        t, text, dist, cov = take(totals)
        take_ms.append(t)
    print(f"\n## {name}: {len(first) - 1} lists of {len(pieces)} pieces -> {totals[0]} text words, {totals[1]} distances, {totals[2]} coverages")
    print("fgpu_stage3_join       wall " + spread(ms))
    print("fgpu_stage3_join_take  wall " + spread(take_ms))
    if name == "graph":                                             # the lists of one piece and of two, against numpy
        c = contigs[order]
        at = first[:-1].astype(np.int64)
        two = sizes == 2
        want_len = c["len"][at].astype(np.int64)
        want_len[two] += c["len"][at[two] + 1].astype(np.int64) - K
        want_cov = c["n_cov"][at].astype(np.int64)
        want_cov[two] += c["n_cov"][at[two] + 1].astype(np.int64) - 1
        assert (out["len"] == want_len).all() and (out["n_cov"] == want_cov).all()
        ends = np.cumsum(out["n_cov"].astype(np.int64))
        sums = np.diff(np.concatenate([[0], np.cumsum(cov.astype(np.int64))[ends - 1]]))
        assert (sums == out["cov_sum"].astype(np.int64)).all()
        print(f"lengths, coverage counts and coverage sums equal numpy's; longest joined contig {int(out['len'].max())} bases, mean coverage of all {float(out['cov_sum'].sum()) / float(out['n_cov'].sum()):.3f}")
    ctx.profile_enable(True)
    ctx.kernel_times_reset()
    wall = join(first, pieces)[0]
    kt = {k_: v for k_, v in ctx.kernel_times().items() if k_.startswith("s3j_")}
    ctx.profile_enable(False)
    total = sum(v[1] for v in kt.values())
    print(f"kernels of one more call with events on (wall {wall:.2f} ms, the three kernels {total:.3f} ms; the rest is the contig records' way to the host, the host's check and sums, their way back)")
    payload = {"s3j_text": 8 * totals[0], "s3j_dist": totals[1], "s3j_cov": totals[2]}
    for k_, (launches, t) in sorted(kt.items()):
        rate = ctx.diag_stream_copy(max(payload[k_], 1 << 16), 20)
        copy_ms = 2 * payload[k_] / (rate * 1e9) * 1e3
        print(f"  {k_:9s} {launches:2d} launch(es) {t:7.3f} ms for {payload[k_]:9d} bytes of output; a device copy of as many bytes: {copy_ms:.3f} ms ({rate:.0f} GB/s read + write): {t / copy_ms:.1f} x")

nt, ns, nv = built["totals"][1:]
t0 = now()
o, cl = np.empty(nc, dtype=api.CONTIG_DTYPE), np.empty(nc, dtype=api.BUILD_DTYPE)
text, kmers, dist, cov = np.empty(nt, dtype=np.uint64), np.empty(ns, dtype=np.uint64), np.empty(ns, dtype=np.uint8), np.empty(nv, dtype=np.uint8)
ctx._c(ctx.lib.fgpu_stage3_build_take(ctx.h, o.ctypes.data, cl.ctypes.data, nc, text.ctypes.data, nt, kmers.ctypes.data, dist.ctypes.data, ns, cov.ctypes.data, nv))
print(f"\nfgpu_stage3_build_take, which any join on the host has to pay first: {1e3 * (now() - t0):.2f} ms (once, after everything above: the joins left the build as it was)")
assert o.tobytes() == contigs.tobytes()
ctx.close()
