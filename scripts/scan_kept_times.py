"""What does `faucet --scan_kept` gain when pass 2 scans the batches pass 1 kept on the device, against the default, in which pass 2 reads,
splits, packs and compares the file a second time?  (GPU box; one GPU; measurement, no bar: the flag is opt-in, and whether it pays on a file
the page cache holds is what this table says.)

Two shapes through the command line, FGPU_CLI_TIMES=1, each mode in turn, three runs of each after one of each to warm up; pass 1, pass 2 and
the whole process (wall clock around it) as median of 3 (min .. max), the bytes pass 1 kept per base, and every output file of the modes
compared byte for byte:
  config 2   BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31 -- as a FASTA file in /dev/shm, `--no_cleaning`
  config 3   config 3's shape at its real size -- 2.5 M pairs, interleaved FASTQ, `--fastq --paired_ends` with cleaning: read offsets, stop
             lists and both pair filters are live (the reads of tests/golden/fullsize.json; the files' digests are the compiled reference's)
With FAUCET_AB_OLD=<tree of the parent commit, built> (scripts/ab_worktree.sh says how to make one) a third leg runs that tree's command line in
the default mode, in turn with the other two: has the flag's plumbing slowed the run that does not use it?
    python scripts/scan_kept_times.py > profiles/scan_kept_times.txt"""
import filecmp
import json
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
from faucet_amd import synth_det as sd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = torch.device("cuda", 0)
AB_OLD = os.environ.get("FAUCET_AB_OLD")
MODES = [("default (pass 2 reads the file again)", "default", [], ROOT), ("--scan_kept", "kept", ["--scan_kept"], ROOT)]
if AB_OLD:
    MODES.append(("parent commit, default", "parent", [], os.path.abspath(AB_OLD)))


def med(v):
    v = sorted(v)
    return f"{v[1]:8.2f} ({v[0]:.2f} .. {v[2]:.2f})"


def config2_text(path):
    n, length = 10_000_000, 100
    host_reads = bench.make_reads(bench.make_genome(20_000_000, 2, dev), n, length, 0.01, 1000, dev).cpu().numpy()
    torch.cuda.empty_cache()
    rec = np.empty((n, 10 + length + 1), dtype=np.uint8)
    rec[:, 0] = ord(">")
    idx = np.arange(n, dtype=np.int64)
    for dgt in range(8):
        rec[:, 8 - dgt] = ord("0") + (idx // 10 ** dgt) % 10
    rec[:, 9] = ord("\n")
    rec[:, 10:10 + length] = host_reads
    rec[:, 10 + length] = ord("\n")
    rec.tofile(path)
    return n * length, ["-size_kmer", "31", "-max_read_length", "100", "-estimated_kmers", "100000000", "-singletons", "20000000", "--no_cleaning"], 0


def config3_text(path):
    with open(os.path.join(ROOT, "tests", "golden", "fullsize.json")) as f:
        fx = json.load(f)["config3"]
    c = fx["params"]
    g = sd.make_genome(c["genome"], c["genome_seed"], dev)
    sd.plant_repeats(g, c["genome_seed"] + 100, *c["repeats"])
    reads = sd.make_pairs(g, c["pairs"], c["read_len"], c["insert"][0], c["insert"][1], c["err"], c["read_seed"], dev)
    sd.fasta_bytes(reads, fastq=True).cpu().numpy().tofile(path)
    bases = int(reads.shape[0]) * c["read_len"]
    del reads, g
    torch.cuda.empty_cache()
    return bases, fx["args"], 3


def measure(title, make_text, suffix):
    d = tempfile.mkdtemp(prefix="faucet_scan_kept_", dir="/dev/shm")
    try:
        path = os.path.join(d, "reads." + suffix)
        bases, args, ok = make_text(path)

        def run(tag, flags, tree):
            cmd = [os.path.join(tree, "faucet_amd", "faucet"), "-read_load_file", path] + ([] if flags else ["-read_scan_file", path]) + \
                  ["-file_prefix", os.path.join(d, tag)] + args + flags
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, FGPU_CLI_TIMES="1"))
            whole = (time.perf_counter() - t0) * 1e3
            assert r.returncode == ok, r.stderr[-2000:]
            ph = dict(re.findall(r"^\[cli\] (pass [12] \([a-z0-9 ,+]+\)) +([0-9.]+) ms", r.stderr, re.M))
            p1 = [float(v) for k, v in ph.items() if k.startswith("pass 1")][0]
            p2 = [float(v) for k, v in ph.items() if k.startswith("pass 2")][0]
            assert ("pass 2 (scan of kept reads)" in ph) == bool(flags), r.stderr[-2000:]
            return p1, p2, whole, r.stderr

        for _, tag, flags, tree in MODES:
            run(tag, flags, tree)
        rows = {mode: [] for mode, _, _, _ in MODES}
        print(f"## {title}: {os.path.getsize(path)} bytes of text, {bases} bases\n")
        print("| mode | run | pass 1, ms | pass 2, ms | whole run, ms |")
        print("|---|---|---|---|---|")
        kept_err = ""
        for i in range(3):
            for mode, tag, flags, tree in MODES:
                p1, p2, whole, err = run(tag, flags, tree)
                rows[mode].append((p1, p2, whole))
                kept_err = err if flags else kept_err
                print(f"| {mode} | {i} | {p1:.2f} | {p2:.2f} | {whole:.2f} |", flush=True)
        files = sorted(f[len("default."):] for f in os.listdir(d) if f.startswith("default."))
        for ext in files:
            for _, tag, _, _ in MODES[1:]:
                assert filecmp.cmp(os.path.join(d, "default." + ext), os.path.join(d, tag + "." + ext), shallow=False), (tag, ext)
        print("\nall modes write byte-identical files: " + ", ".join("." + e for e in files))
        m = re.search(r"([0-9]+) bytes kept on the device in ([0-9]+) batches", kept_err)
        if m:
            print(f"pass 1 kept {m.group(1)} bytes in {m.group(2)} batches: {int(m.group(1)) / bases:.4f} bytes per base")
        print("\n| mode | pass 1, ms (median of 3; min .. max) | pass 2, ms | whole run, ms |")
        print("|---|---|---|---|")
        for mode, v in rows.items():
            print(f"| {mode} | " + " | ".join(med([r[c] for r in v]) for c in range(3)) + " |")
        print(flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


which = sys.argv[1] if len(sys.argv) > 1 else "both"
if which in ("both", "config2"):
    measure("config 2 (FASTA, --no_cleaning)", config2_text, "fa")
if which in ("both", "config3"):
    measure("config 3's shape (--fastq --paired_ends, cleaning)", config3_text, "fq")
