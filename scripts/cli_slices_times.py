"""Pass 1 of `faucet -gpus N` on config 2's reads as a FASTA file at full size, FAUCET_SHARD_PROTOCOL=slices against the default protocol: the
same build, alternating, `runs` runs each, the times from the FGPU_CLI_TIMES marks; .bloom and .junctions of every run against the compiled
reference's digests (tests/golden/fullsize.json, config2_cli).  All contexts share this box's one device: not a scaling number.
    python scripts/cli_slices_times.py [gpus = 4] [runs = 3]"""
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


gpus = sys.argv[1] if len(sys.argv) > 1 else "4"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
with open(os.path.join(ROOT, "tests", "golden", "fullsize.json")) as f:
    fx = json.load(f)["config2_cli"]
c = fx["params"]
dev = torch.device("cuda", 0)
reads = sd.make_reads(sd.make_genome(c["genome"], c["genome_seed"], dev), c["reads"], c["read_len"], c["err"], c["read_seed"], dev)
text = sd.fasta_bytes(reads, fastq=False).cpu().numpy()
del reads
assert hashlib.sha256(text.tobytes()).hexdigest() == fx["text_sha256"], "the generator gives another text here than the fixture's"
d = tempfile.mkdtemp(prefix="faucet_slices_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    path = os.path.join(d, "reads.fa")
    text.tofile(path)
    print(f"config 2 as FASTA: {text.size} bytes, -gpus {gpus}, {runs} runs per protocol, alternating", flush=True)
    del text
    exe = os.path.join(ROOT, "faucet_amd", "faucet")
    times = {"default": [], "slices": []}
    for i in range(runs):
        for name, env in (("default", {}), ("slices", {"FAUCET_SHARD_PROTOCOL": "slices"})):
            prefix = os.path.join(d, f"out_{name}_{i}")
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-read_load_file", path, "-read_scan_file", path, "-file_prefix", prefix, "-gpus", gpus] + fx["args"],
                               capture_output=True, text=True, timeout=900,
                               env=dict({k: v for k, v in os.environ.items() if k != "FAUCET_SHARD_PROTOCOL"}, FGPU_CLI_TIMES="1", **env))
            dt = time.perf_counter() - t0
            if r.returncode != 0:
                print(name, "exit", r.returncode, r.stderr[-1500:], flush=True)
                sys.exit(1)
            marks = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[cli\] (pass [12] \([^)]*\))\s+([0-9.]+) ms", r.stderr)}
            ok = sha_file(prefix + ".bloom") == fx["bloom_sha256"] and sha_file(prefix + ".junctions") == fx["junctions_sha256"]
            p1 = [v for k, v in marks.items() if k.startswith("pass 1")]
            p2 = [v for k, v in marks.items() if k.startswith("pass 2")]
            times[name].append(p1[0] if p1 else float("nan"))
            print(f"{name:8s} run {i}: process {dt * 1e3:.0f} ms | " + " | ".join(f"{k} {v:.1f} ms" for k, v in marks.items()) +
                  f" | files {'equal the reference digests' if ok else 'DIFFER from the reference digests'}", flush=True)
            for ln in r.stderr.splitlines():
                if "rank" in ln and "pass 1" in ln:
                    print("    " + ln.strip()[:230], flush=True)
            if not p1 or not p2:
                print("    (marks not parsed) " + " / ".join(ln.strip() for ln in r.stderr.splitlines() if "pass" in ln)[:600], flush=True)
            for ext in ("bloom", "junctions"):
                os.remove(prefix + "." + ext)
            if not ok:
                sys.exit(2)
    for name, v in times.items():
        print(f"pass 1, {name}: " + ", ".join(f"{x:.1f}" for x in v) + f" ms (median {sorted(v)[len(v) // 2]:.1f})")
finally:
    shutil.rmtree(d, ignore_errors=True)
