"""`faucet -gpus 2` under FAUCET_SHARD_PROTOCOL=slices on config 2's reads as a FASTA file in /dev/shm, through the command line, both ranks on
this box's ONE device: what --scan_kept (pass 1 keeps the reads, pass 2 scans them: the file is read once) costs or saves against the sliced
run that reads the file twice, and that run against the parent commit's.

    slices              this build, the file given twice                      (the default of the protocol)
    slices+scan_kept    this build, -read_load_file only, --scan_kept
    parent slices       the build of the parent commit under ab_old/ (scripts/ab_worktree.sh says how it is made); left out where there is none

Alternating, `runs` runs each; the times are the FGPU_CLI_TIMES phase clock's pass 1 and pass 2 marks and the process' wall clock: median with
minimum and maximum.  .bloom and .junctions of every run against the compiled reference's digests (tests/golden/fullsize.json, config2_cli).
Ranks that share one device show OVERHEAD, not speed-up.  Not measured here: a pipe fed by a decompressor, runs on N real devices, config 4's size.
    python scripts/multi_scan_kept_times.py [runs = 3] [gpus = 2]"""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from faucet_amd import synth_det as sd  # noqa: E402


def sha_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def spread(v):
    s = sorted(v)
    return f"{s[len(s) // 2]:8.1f} ({s[0]:.1f} .. {s[-1]:.1f})"


runs = int(sys.argv[1]) if len(sys.argv) > 1 else 3
gpus = sys.argv[2] if len(sys.argv) > 2 else "2"
with open(os.path.join(ROOT, "tests", "golden", "fullsize.json")) as f:
    fx = json.load(f)["config2_cli"]
c = fx["params"]
dev = torch.device("cuda", 0)
reads = sd.make_reads(sd.make_genome(c["genome"], c["genome_seed"], dev), c["reads"], c["read_len"], c["err"], c["read_seed"], dev)
text = sd.fasta_bytes(reads, fastq=False).cpu().numpy()
del reads
torch.cuda.empty_cache()
assert hashlib.sha256(text.tobytes()).hexdigest() == fx["text_sha256"], "the generator gives another text here than the fixture's"
d = tempfile.mkdtemp(prefix="faucet_multi_kept_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    path = os.path.join(d, "reads.fa")
    text.tofile(path)
    print(f"config 2 as FASTA: {text.size} bytes, -gpus {gpus} on one device, FAUCET_SHARD_PROTOCOL=slices, {runs} runs per mode, alternating", flush=True)
    del text
    here, parent = os.path.join(ROOT, "faucet_amd", "faucet"), os.path.join(ROOT, "ab_old", "faucet_amd", "faucet")
    twice, once = ["-read_load_file", path, "-read_scan_file", path], ["-read_load_file", path, "--scan_kept"]
    modes = [("slices", here, twice), ("slices+scan_kept", here, once)] + ([("parent slices", parent, twice)] if os.path.exists(parent) else [])
    if len(modes) == 2:
        print("(no build of the parent commit under ab_old/: that mode is left out)", flush=True)
    times = {name: {"pass 1": [], "pass 2": [], "process": []} for name, _, _ in modes}
    for i in range(runs):
        for name, exe, inputs in modes:
            prefix = os.path.join(d, f"out_{i}")
            t0 = time.perf_counter()
            r = subprocess.run([exe] + inputs + ["-file_prefix", prefix, "-gpus", gpus] + fx["args"], capture_output=True, text=True, timeout=900,
                               env=dict(os.environ, FGPU_CLI_TIMES="1", FAUCET_SHARD_PROTOCOL="slices"))
            dt = 1e3 * (time.perf_counter() - t0)
            if r.returncode != 0:
                print(name, "exit", r.returncode, r.stderr[-1500:], flush=True)
                sys.exit(1)
            marks = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[cli\] (pass [12] \([^)]*\))\s+([0-9.]+) ms", r.stderr)}
            ok = sha_file(prefix + ".bloom") == fx["bloom_sha256"] and sha_file(prefix + ".junctions") == fx["junctions_sha256"]
            for ext in ("bloom", "junctions"):
                os.remove(prefix + "." + ext)
            p1 = [v for k, v in marks.items() if k.startswith("pass 1")]
            p2 = [v for k, v in marks.items() if k.startswith("pass 2")]
            if not ok or len(p1) != 1 or len(p2) != 1:
                print(name, "files DIFFER from the reference digests" if not ok else "marks not parsed: " + str(marks), flush=True)
                sys.exit(2)
            kept = ("reads kept" in r.stderr, "scan of kept reads" in r.stderr)
            assert kept == ((True, True) if name == "slices+scan_kept" else (False, False)), (name, kept)
            times[name]["pass 1"].append(p1[0])
            times[name]["pass 2"].append(p2[0])
            times[name]["process"].append(dt)
            print(f"{name:17s} run {i}: process {dt:.0f} ms | " + " | ".join(f"{k} {v:.1f} ms" for k, v in marks.items()) + " | files equal the reference digests",
                  flush=True)
    print(f"\nms, median (min .. max) of {runs}; -gpus {gpus}, both ranks on one MI355X")
    print(f"{'mode':17s} {'pass 1':>28s} {'pass 2':>28s} {'process':>28s}")
    for name, _, _ in modes:
        t = times[name]
        print(f"{name:17s} {spread(t['pass 1']):>28s} {spread(t['pass 2']):>28s} {spread(t['process']):>28s}")
finally:
    shutil.rmtree(d, ignore_errors=True)
