"""What does `faucet --estimate` gain when pass 0 keeps the batches it packs and pass 1 loads from them (FAUCET_ESTIMATE_KEEP=1), against
the default, in which pass 1 reads, splits and packs the file a second time?  (GPU box; one GPU; measurement, no bar: whether the kept path
becomes the default for regular files is decided from this table, not here.)

BASELINE config 2's reads -- 10 M x 100 bases of a 20 Mb genome, 1 % errors, k = 31 -- as a FASTA file in /dev/shm through the command line:
`faucet --estimate --no_cleaning`, both passes and the scan, the two modes in turn, three runs of each after one of each to warm up; the
phases from the command line's own clock (FGPU_CLI_TIMES=1): pass 0, pass 1 and their sum per mode as median of 3 (min .. max), the bytes
pass 0 kept, and both modes' .bloom / .junctions compared byte for byte.  With FAUCET_AB_OLD=<tree of the parent commit, built> (scripts/ab_worktree.sh
says how to make one) a third leg runs that tree's command line in the default mode, in turn with the other two: has keeping slowed the
pass 0 that does not keep?
    python scripts/estimate_keep_times.py [r_bits] > profiles/estimate_keep_times.txt"""
import filecmp
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

R_BITS = int(sys.argv[1]) if len(sys.argv) > 1 else 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dev = torch.device("cuda", 0)
n, LEN = 10_000_000, 100
host_reads = bench.make_reads(bench.make_genome(20_000_000, 2, dev), n, LEN, 0.01, 1000, dev).cpu().numpy()
torch.cuda.empty_cache()
AB_OLD = os.environ.get("FAUCET_AB_OLD")
MODES = [("default (pass 1 reads the file again)", {}, ROOT), ("kept (FAUCET_ESTIMATE_KEEP=1)", {"FAUCET_ESTIMATE_KEEP": "1"}, ROOT)]
if AB_OLD:
    MODES.append(("parent commit, default", {}, os.path.abspath(AB_OLD)))


def med(v):
    v = sorted(v)
    return f"{v[1]:8.2f} ({v[0]:.2f} .. {v[2]:.2f})"


d = tempfile.mkdtemp(prefix="faucet_keep_", dir="/dev/shm")
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
    del rec, host_reads

    def run(mode, env, tree):
        prefix = os.path.join(d, "kept" if env else "default" if tree == ROOT else "parent")
        cmd = [os.path.join(tree, "faucet_amd", "faucet"), "-read_load_file", path, "-read_scan_file", path, "-size_kmer", "31", "-max_read_length", "100",
               "--no_cleaning", "--estimate", "-file_prefix", prefix] + (["-estimate_bits", str(R_BITS)] if R_BITS else [])
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, FGPU_CLI_TIMES="1", **env))
        assert r.returncode == 0, r.stderr[-2000:]
        ph = dict(re.findall(r"^\[cli\] (pass [012] \([a-z0-9 ,+]+\)) +([0-9.]+) ms", r.stderr, re.M))
        p0 = [float(v) for k, v in ph.items() if k.startswith("pass 0")][0]
        p1 = [float(v) for k, v in ph.items() if k.startswith("pass 1")][0]
        p2 = [float(v) for k, v in ph.items() if k.startswith("pass 2")][0]
        kept = re.search(r"([0-9]+) bytes of packed reads kept in ([0-9]+) blocks \(budget ([0-9]+) bytes\)", r.stderr)
        assert bool(kept) == bool(env) and ("pass 1 (load from kept reads)" in ph) == bool(env), r.stderr[-2000:]
        return p0, p1, p2, kept, r.stdout.split("\n")[:2]

    for mode, env, tree in MODES:
        run(mode, env, tree)
    rows = {mode: [] for mode, _, _ in MODES}
    heads, kept_note = set(), None
    print("| mode | run | pass 0, ms | pass 1, ms | pass 0 + pass 1, ms | pass 2, ms |")
    print("|---|---|---|---|---|---|")
    for i in range(3):
        for mode, env, tree in MODES:
            p0, p1, p2, kept, head = run(mode, env, tree)
            rows[mode].append((p0, p1, p0 + p1, p2))
            heads.add(tuple(head))
            kept_note = kept or kept_note
            print(f"| {mode} | {i} | {p0:.2f} | {p1:.2f} | {p0 + p1:.2f} | {p2:.2f} |", flush=True)
    assert len(heads) == 1, heads
    for ext in ("bloom", "junctions"):
        for other in ["kept"] + (["parent"] if AB_OLD else []):
            assert filecmp.cmp(os.path.join(d, "default." + ext), os.path.join(d, other + "." + ext), shallow=False), (other, ext)
    print("\nall modes print: " + " / ".join(heads.pop()) + "; their .bloom and .junctions are byte-identical")
    print(f"pass 0 kept {kept_note.group(1)} bytes of packed reads (4 bits per stream position) in {kept_note.group(2)} blocks, of a budget of {kept_note.group(3)} bytes; "
          f"the file is {os.path.getsize(path)} bytes")
    print("\n| mode | pass 0, ms (median of 3; min .. max) | pass 1, ms | pass 0 + pass 1, ms | pass 2, ms |")
    print("|---|---|---|---|---|")
    for mode, v in rows.items():
        print(f"| {mode} | " + " | ".join(med([r[c] for r in v]) for c in range(4)) + " |")
finally:
    shutil.rmtree(d, ignore_errors=True)
