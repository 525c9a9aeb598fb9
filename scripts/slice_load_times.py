"""Pass 1 by filter slices against the read-shard protocols, per rank, on ONE MI355X: BASELINE config 4 (tests/golden/fullsize.json), N = 2, 4, 8.

Sliced pass (sharded.load_sliced's phases): the N contexts side by side on the device, every rank loading the WHOLE stream into its slice of the
filter bits.  Each rank's slice_load and commit are timed on their own -- host clock around work that ends in a synchronise -- one warm-up and
three repetitions, all printed; the commits run on the planes ORed over all ranks, as in the protocol.  The exchanges are priced, not measured
(LINK_GBPS per xGMI link and direction, every rank on its own link to every other): the OR-allreduce of the fail planes (one bit per stream
position: reduce-scatter + all-gather by slices) and the gather of the bloo1 / bloo2 byte ranges.  The concatenated slices and to_bloo2 are
compared with the fixture's digests in the same run.

Read-shard protocol (what sharded.load_sharded takes for the shape; scripts/project_strong.py's pass-1 part), alternating with the above for the same
N in the same process: every rank's own load + fix-up (or presence pass + load on the prefix), the same one warm-up + three repetitions, all
printed, the minimum taken on both sides; the slowest rank + the two priced exchanges.

    timeout -k 10 900 python scripts/slice_load_times.py [N ...]        (default 2 4 8)"""
import hashlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from faucet_amd import _lib as L  # noqa: E402
from faucet_amd import api, sharded  # noqa: E402
from faucet_amd import synth_det as sd  # noqa: E402

LINK = float(os.environ.get("LINK_GBPS", "50"))
REPS = int(os.environ.get("REPS", "3"))
Ns = [int(a) for a in sys.argv[1:]] or [2, 4, 8]
fx = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "fullsize.json")))[os.environ.get("FIXTURE", "config4")]
c = fx["params"]
dev = torch.device("cuda", 0)
tai, nh = api.load_filter_shape(c["E"], c["S"])
genome = sd.make_genome(c["genome"], c["genome_seed"], dev)
reads = sd.make_reads(genome, c["reads"], c["read_len"], c["err"], c["read_seed"], dev)
del genome


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def sha(t):
    h = hashlib.sha256()
    for lo in range(0, t.numel(), 1 << 28):
        h.update(t[lo:lo + (1 << 28)].cpu().numpy().tobytes())
    return h.hexdigest()


def fmt(v):
    return " ".join(f"{x:.0f}" for x in v)


def sliced(N):
    stream = bench.device_batches(reads, bench.batch_bounds(c["reads"], 2_500_000, 2))
    sl = sharded._slices(tai // 8, N, 64)
    backs = [sharded.GpuShard(api.Context(c["k"], tai, nh), dev, stream_ordered=False) for _ in range(N)]
    t_load, t_commit = [[] for _ in range(N)], [[] for _ in range(N)]
    acc, stats = None, None
    for rep in range(1 + REPS):                  # rep 0: the warm-up, which also makes the ORed planes and checks the result
        if rep == 0:
            for r, b in enumerate(backs):
                _, ms = timed(lambda: b.slice_load(stream, sl[r][0] * 8, sl[r][1] * 8))
                t_load[r].append(ms)
            for b in backs:
                planes = b.slice_planes()
                if acc is None:
                    acc = [p.clone() for p in planes]
                    torch.cuda.synchronize()
                else:
                    for a, p in zip(acc, planes):
                        b.or_tensor(a, p)
                    b.ctx.synchronize()
        b1, b2 = (torch.zeros(tai // 8, dtype=torch.uint8, device=dev) for _ in range(2)) if rep == 0 else (None, None)
        for r, b in enumerate(backs):
            if rep > 0:
                _, ms = timed(lambda: b.slice_load(stream, sl[r][0] * 8, sl[r][1] * 8))
                t_load[r].append(ms)
            for a, p in zip(acc, b.slice_planes()):
                p.copy_(a)
            (stats), ms = timed(lambda: (b.slice_commit(), b.slice_end())[1])
            t_commit[r].append(ms)
            if rep == 0:
                lo, hi = sl[r]
                b1[lo:hi].copy_(b.bloom_tensor(L.BLOO1)[lo:hi])
                b2[lo:hi].copy_(b.bloom_tensor(L.BLOO2)[lo:hi])
        if rep == 0:
            torch.cuda.synchronize()
            ok = (sha(b1) == fx.get("bloo1_sha256") and sha(b2) == fx.get("bloo2_sha256") and stats["to_bloo2"] == fx.get("to_bloo2") and
                  stats["kmers"] == fx.get("kmers"))
            del b1, b2
    state = [b.ctx.load_slice_state()[1] for b in backs]
    plane_bytes = sum(a.numel() for a in acc)
    for b in backs:
        b.close()
    del acc
    torch.cuda.empty_cache()
    fail_or = 2 * (plane_bytes / N) / (LINK * 1e9) * 1e3 * (N > 1)          # reduce-scatter + all-gather: plane bytes / N per link and phase
    gather = 2 * (tai / 8 / N) / (LINK * 1e9) * 1e3 * (N > 1)               # bloo1 and bloo2: every rank's byte range over each of its links
    for r in range(N):
        print(f"  slices N={N} rank {r}: slice_load {fmt(t_load[r])} ms | commit {fmt(t_commit[r])} ms   (warm-up first)", flush=True)
    best_load = max(min(t[1:]) for t in t_load)
    best_commit = max(min(t[1:]) for t in t_commit)
    p1 = best_load + fail_or + best_commit + gather
    print(f"slices N={N}: slowest rank slice_load {best_load:.0f} ms + fail-plane OR ({plane_bytes / 1e9:.2f} GB of planes) {fail_or:.1f} ms + commit "
          f"{best_commit:.0f} ms + gather {gather:.1f} ms = pass 1 {p1:.0f} ms | slice state per rank {max(state) / 2**30:.2f} GiB, {N} contexts side by side | "
          f"bloo1, bloo2, kmers, to_bloo2 {'EQUAL' if ok else 'DIFFER FROM'} the oracle's digests", flush=True)
    return p1


def shards_protocol(N):
    per = c["reads"] // N
    ctx = api.Context(c["k"], tai, nh)
    b = sharded.GpuShard(ctx, dev, stream_ordered=False)
    shard = lambda r: bench.device_batches(reads[r * per:(r + 1) * per], bench.batch_bounds(per, 2_500_000, 2))      # noqa: E731
    fixup = os.environ.get("FAUCET_SHARD_PROTOCOL", "auto") != "presence" and b.fixup_possible(shard(0))
    t_first, t_second = [], []
    running = torch.zeros(tai // 8, dtype=torch.uint8, device=dev)
    if fixup:
        for r in range(N):
            batches = shard(r)
            runs = []
            for _ in range(1 + REPS):
                b.clear_filters()
                _, ms = timed(lambda: b.load(batches, keep_carry=False, shard_times=True))
                runs.append(ms)
            t_first.append(runs)
            ms = 0.0
            if r > 0:                        # (once per pass: the fix-up consumes the pass' state)
                _, ms = timed(lambda: b.load_fixup(running))
            t_second.append([ms])
            running |= b.bloom_tensor(L.BLOO1)
    else:
        pres = []
        for r in range(N):
            batches = shard(r)
            runs = []
            for _ in range(1 + REPS):
                b.clear_filters()
                _, ms = timed(lambda: [b.presence(x) for x in batches])
                ctx.synchronize()
                runs.append(ms)
            t_first.append(runs)
            pres.append(b.bloom_tensor(L.BLOO1).clone())
        for r in range(N):
            batches = shard(r)
            runs = []
            for _ in range(1 + REPS):
                b.clear_filters()
                b.bloom_tensor(L.BLOO1).copy_(running)
                ctx.synchronize()
                _, ms = timed(lambda: b.load(batches, keep_carry=True))
                runs.append(ms)
            t_second.append(runs)
            running |= pres[r]
        del pres
    ctx.close()
    del running
    torch.cuda.empty_cache()
    exch = 2 * 2 * (tai / 8 / N) / (LINK * 1e9) * 1e3
    best = lambda v: min(v[1:]) if len(v) > 1 else v[0]      # noqa: E731   (warm-up first, as on the sliced side)
    for r in range(N):
        print(f"  shards N={N} rank {r}: {'own load' if fixup else 'presence'} {fmt(t_first[r])} ms | {'fix-up (one run)' if fixup else 'load on the prefix'} "
              f"{fmt(t_second[r])} ms   (warm-up first)", flush=True)
    slowest = max(best(p) + best(q) for p, q in zip(t_first, t_second))
    p1 = slowest + exch
    print(f"shards N={N} ({'own load + fix-up' if fixup else 'presence + load'}): slowest rank {slowest:.0f} ms + exchanges {exch:.0f} ms = pass 1 {p1:.0f} ms", flush=True)
    return p1


rows = []
for N in Ns:
    a = sliced(N)
    z = shards_protocol(N)
    rows.append((N, a, z))
print(f"\npass 1 of config 4, ms (links priced at {LINK:.0f} GB/s per direction)\n   N   slices   shards")
for N, a, z in rows:
    print(f"{N:4d} {a:8.0f} {z:8.0f}")
