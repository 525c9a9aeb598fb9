"""What does pass 0 over N read shards (ShardedRun::estimate, fgpu_group_estimate_end) cost a rank, beside today's pass on one device?  (GPU box;
one GPU; measurement, no bar: what it gives for N devices is a PROJECTION and is labelled as one.)

BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31, resident in HBM, batches of at most 1 M reads -- and N = 2, 4, 8.
One rank's stages in turn, on one device, wall time with the device synchronised, median of 3 (min .. max) after one round to warm up:
  sketch    fgpu_estimate_begin (2^r_bits bytes of planes allocated and cleared) and the batches of the first 1/N of the reads
  merge     the rank's slice (1/N of the planes) of each of the N - 1 peers copied into the staging buffer and merged (fgpu_estimate_merge), in the
            chunks the collective uses (at most 128 MiB of staging); the peer is a second context that sketched the next 1/N of the reads, the
            same one N - 1 times.  On one device the copy runs at HBM speed; between devices the (N - 1)/N of a sketch a rank takes in crosses xGMI
  end       fgpu_estimate_end: counts the WHOLE planes (the collective counts the rank's slice, 1/N of them: an upper bound) and frees them
beside the one-device pass over all reads (begin to end), in the same process on the same resident reads.
Then the command line: `faucet --estimate -gpus 2 --just_load_bloom` on the same reads as a FASTA file in /dev/shm, both shards on this one device,
with FAUCET_ESTIMATE_SHARDS=0 (pass 0 on the first device alone) against the default, FGPU_CLI_TIMES=1: what the shards add on ONE device --
overhead (a second placeholder context, two sketches' planes, the exchange, and the record cuts of the file, which the first pass over the
shards finds and the later ones reuse: pass 1's column shows them moving), not speed-up.
    python scripts/estimate_shard_times.py [r_bits] > profiles/estimate_shard_times.txt"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from faucet_amd import _lib as L  # noqa: E402
from faucet_amd import api  # noqa: E402

R_BITS = int(sys.argv[1]) if len(sys.argv) > 1 else 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = torch.device("cuda", 0)
n, LEN = 10_000_000, 100
reads = bench.make_reads(bench.make_genome(20_000_000, 2, dev), n, LEN, 0.01, 1000, dev)
lib = L.load()
ctx, peer = api.Context(31, 128, 1), api.Context(31, 128, 1)


def batches(lo, hi):
    return bench.device_batches(reads, [(a, min(a + 1_000_000, hi)) for a in range(lo, hi, 1_000_000)])


def med(v):
    v = sorted(v)
    return f"{v[1]:8.2f} ({v[0]:.2f} .. {v[2]:.2f})"


def one_device(all_reads):
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.estimate_begin(R_BITS)
    for b in all_reads:
        ctx.estimate_batch(b)
    e = ctx.estimate_end()
    return 1e3 * (time.perf_counter() - t0), e


def rank_stages(N, mine, stage, peer_planes, nbytes):
    step = ((nbytes + N - 1) // N + 15) & ~15               # the slices of fgpu_group_or_allreduce; this rank's is the first
    chunk = min(((128 << 20) // (N - 1)) & ~15, step)
    ctx.synchronize()
    t = [time.perf_counter()]
    ctx.estimate_begin(R_BITS)
    for b in mine:
        ctx.estimate_batch(b)
    ctx.synchronize()
    t.append(time.perf_counter())
    for at in range(0, step, chunk):
        ln = min(chunk, step - at)
        for i in range(N - 1):
            assert lib.fgpu_device_copy(ctx.h, stage.data_ptr() + i * chunk, peer_planes + at, ln) == 0
        for i in range(N - 1):
            ctx.estimate_merge(stage.data_ptr() + i * chunk, at, ln)
    ctx.synchronize()
    t.append(time.perf_counter())
    ctx.estimate_end()
    t.append(time.perf_counter())
    return [1e3 * (b - a) for a, b in zip(t[:-1], t[1:])]


everything = batches(0, n)
one_device(everything)
base = []
for i in range(3):
    ms, whole = one_device(everything)
    base.append(ms)
nbytes = 1 << whole["r_bits"]
print(f"config 2's reads: {n} reads, {whole['kmers']} k-mers; sketch of 2^{whole['r_bits']} cells per level ({nbytes >> 20} MiB of planes), solved from level "
      f"{whole['level']}: F0 = {whole['f0']:.0f}, f1 = {whole['f1']:.0f}")
print("\n| what, on ONE device | wall, ms (median of 3; min .. max) |")
print("|---|---|")
print(f"| one-device pass 0 over all reads (today's path) | {med(base)} |")
rows = {}
for N in (2, 4, 8):
    share = n // N
    mine, theirs = batches(0, share), batches(share, 2 * share)
    peer.estimate_begin(R_BITS)
    for b in theirs:
        peer.estimate_batch(b)
    peer_planes, _ = peer.estimate_planes_devptr()
    peer.synchronize()
    step = ((nbytes + N - 1) // N + 15) & ~15
    stage = torch.empty(min(((128 << 20) // (N - 1)) & ~15, step) * (N - 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    rank_stages(N, mine, stage, peer_planes, nbytes)
    runs = [rank_stages(N, mine, stage, peer_planes, nbytes) for _ in range(3)]
    peer.estimate_end()
    del stage
    rows[N] = [[r[i] for r in runs] for i in range(3)]
    print(f"| N = {N}: sketch of 1/{N} of the reads | {med(rows[N][0])} |")
    print(f"| N = {N}: merge of the slice of {N - 1} peer{'s' if N > 2 else ''} ({(N - 1) * step >> 20} MiB copied and merged) | {med(rows[N][1])} |")
    print(f"| N = {N}: end (count of the whole planes, an upper bound for the slice's; free) | {med(rows[N][2])} |", flush=True)
print("\nPROJECTION (not a measurement of N devices): a rank's pass 0 = sketch + merge + end as measured above, on a device of its own, the N - 1 slices"
      " it takes in crossing xGMI instead of HBM; reading and splitting its share of a file is not in these figures (the reads are resident).")
print("| N | a rank's stages in turn, ms (medians) | of the one-device pass |")
print("|---|---|---|")
b = sorted(base)[1]
for N, r in rows.items():
    tot = sum(sorted(v)[1] for v in r)
    print(f"| {N} | {tot:.2f} | {tot / b:.2f} |")
ctx.close()
peer.close()

# ---- the command line: -gpus 2 on this one device, pass 0 on the first device alone against pass 0 over the shards
host_reads = reads.cpu().numpy()
del reads, everything
d = tempfile.mkdtemp(prefix="faucet_est_", dir="/dev/shm")
try:
    rec = np.empty((n, 10 + LEN + 1), dtype=np.uint8)
    rec[:, 0] = ord(">")
    idx = np.arange(n, dtype=np.int64)
    for dgt in range(8):
        rec[:, 8 - dgt] = ord("0") + (idx // 10 ** dgt) % 10
    rec[:, 9] = ord("\n")
    rec[:, 10:10 + LEN] = host_reads
    rec[:, 10 + LEN] = ord("\n")
    path = os.path.join(d, "reads.fa")
    rec.tofile(path)
    del rec
    cmd = [os.path.join(ROOT, "faucet_amd", "faucet"), "-read_load_file", path, "-read_scan_file", path, "-size_kmer", "31", "-max_read_length", "100",
           "--no_cleaning", "--just_load_bloom", "--estimate", "-gpus", "2", "-file_prefix", os.path.join(d, "out")] + (["-estimate_bits", str(R_BITS)] if R_BITS else [])
    print("\n`faucet --estimate -gpus 2 --just_load_bloom` on the same reads as a FASTA file, both shards on ONE device (overhead, not speed-up); phase clock, ms:")
    print("| pass 0 | run | placeholder context(s) | pass 0 | pass 1 | process |")
    print("|---|---|---|---|---|---|")
    heads, notes = {}, []
    for i in range(3):
        for name, env in (("first device alone (FAUCET_ESTIMATE_SHARDS=0)", {"FAUCET_ESTIMATE_SHARDS": "0"}), ("over the 2 shards (default)", {})):
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, FGPU_CLI_TIMES="1", **env))
            dt = 1e3 * (time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr[-2000:]
            ph = dict(re.findall(r"^\[cli\] (arguments, placeholder contexts?|pass 0 \([a-z +]+\)) +([0-9.]+) ms", r.stderr, re.M))
            setup = [v for k, v in ph.items() if k.startswith("arguments")][0]
            pass0 = [v for k, v in ph.items() if k.startswith("pass 0")][0]
            heads.setdefault(name, r.stdout.split("\n")[:2])
            load = re.search(r"^\[cli\] (pass 1 \([a-z ,+-]+\)) +([0-9.]+) ms", r.stderr, re.M)
            print(f"| {name} | {i} | {setup} | {pass0} | {load.group(2) if load else '?'} | {dt:.0f} |", flush=True)
            if i == 2:
                notes += [ln.strip() for ln in r.stderr.splitlines() if "pass 0:" in ln]
    a, b2 = heads.values()
    assert a == b2, (a, b2)
    print("both print: " + " / ".join(a))
    print("the last run over the shards, as the command line tells it:")
    for ln in notes:
        print("    " + ln)
finally:
    shutil.rmtree(d, ignore_errors=True)
