"""Two builds of the host side against each other on the CPU: exit code, stdout, stderr and every output file, run by run.

    python scripts/host_ab.py --old OLD/faucet --new NEW/faucet [--old-ref OLD/faucet_ref_stub --new-ref NEW/faucet_ref_stub]

--old / --new: faucet_amd/host/faucet_main.cpp of two trees, each built against the tests' CPU stand-in of the C ABI with the command of
tests/test_host_sanitizers.py minus the sanitizer flags; --old-ref / --new-ref: `make -C oracle ref_stub` of the same two trees (the compiled
reference with integration/faucet_binding.cpp linked in).  Both programs of a pair run with the same paths, one after the other, so that the
log lines that name files are the same; the two `Time ...` lines are blanked.  profiles/host_unify_ab.txt is this script's output."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.golden_util import Case  # noqa: E402

CASES = ["se_cleaning_k21", "c1_k21", "mercy_k21", "pe_fastq_k21", "pe_repeats_k25", "pe_fasta_highcov_k31"]


def run(exe, argv, env, d):
    out = os.path.join(d, "out")
    os.makedirs(out)
    r = subprocess.run([exe] + argv, capture_output=True, text=True, errors="replace", timeout=900, env=dict(os.environ, **env))
    files = {}
    for f in sorted(os.listdir(out)):
        data = open(os.path.join(out, f), "rb").read()
        if f.endswith(".fastg"):          # the reference names nodes by heap address
            seen = {}
            data = re.sub(rb"0x[0-9a-f]+", lambda m: seen.setdefault(m.group(0), b"n%d" % len(seen)), data)
        files[f] = data
    shutil.rmtree(out)
    stdout = re.sub(r"^(Time [^:]*:).*$", r"\1", r.stdout, flags=re.M)
    return r.returncode, stdout, r.stderr, files


def compare(label, old, new, argv, env, d, keep=None):
    a = run(old, argv, env, d)
    b = run(new, argv, env, d)
    if keep is not None:
        keep.update(b[3])
    cols = ["same" if x == y else "DIFFERS" for x, y in zip(a, b)]
    err = ""
    if a[2] != b[2]:
        la, lb = a[2].splitlines(), b[2].splitlines()
        err = "   stderr: " + " | ".join(f"old {x!r} new {y!r}" for x, y in zip(la, lb) if x != y)[:400] if len(la) == len(lb) else "   stderr: other line count"
    print(f"{label:<58} exit {a[0]}/{b[0]} {cols[0]:<8} stdout {cols[1]:<8} stderr {cols[2]:<8} files({len(a[3])}/{len(b[3])}) {cols[3]}{err}")
    return all(c == "same" for c in cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", required=True)
    ap.add_argument("--new", required=True)
    ap.add_argument("--old-ref")
    ap.add_argument("--new-ref")
    args = ap.parse_args()
    d = tempfile.mkdtemp(prefix="host_ab_")
    same = 0
    total = 0
    try:
        for name in CASES:
            c = Case(name)
            inp = os.path.join(d, "reads.fq" if c.fastq else "reads.fa")
            with open(inp, "wb") as f:
                f.write(c.reads_text())
            base = ["-read_load_file", inp, "-read_scan_file", inp, "-file_prefix", os.path.join(d, "out", "out")] + c.meta["args"]
            made = {}
            runs = [("plain", base, {}), ("-batch_reads 333", base + ["-batch_reads", "333"], {})]
            if c.paired:
                runs.append(("FGPU_DEBUG_LONG_PAIRS_NOMEM=1", base, {"FGPU_DEBUG_LONG_PAIRS_NOMEM": "1"}))
            runs.append(("-gpus 3 FAUCET_SHARD_PROTOCOL=presence", base + ["-gpus", "3"], {"FAUCET_SHARD_PROTOCOL": "presence"}))
            runs.append(("--just_load_bloom", base + ["--just_load_bloom"], {}))
            for i, (what, argv, env) in enumerate(runs):
                total += 1
                same += compare(f"{name}: {what}", args.old, args.new, argv, env, d, made if i == 0 else None)
            bloom = os.path.join(d, "restart.bloom")
            with open(bloom, "wb") as f:
                f.write(made["out.bloom"])
            for what, argv, env in [("-bloom_file restart", base + ["-bloom_file", bloom], {}),
                                    ("-bloom_file restart, -gpus 3", base + ["-bloom_file", bloom, "-gpus", "3"], {"FAUCET_SHARD_PROTOCOL": "presence"})]:
                total += 1
                same += compare(f"{name}: {what}", args.old, args.new, argv, env, d)
            if name == CASES[0]:
                missing = [x if x != inp else inp + ".missing" for x in base]
                unwritable = [x if x != os.path.join(d, "out", "out") else os.path.join(d, "no_such_folder", "out") for x in base]
                for what, argv in [("error: missing input file", missing), ("error: missing input file, -gpus 2", missing + ["-gpus", "2"]),
                                   ("error: unwritable prefix", unwritable), ("error: unwritable prefix, -gpus 2", unwritable + ["-gpus", "2"]),
                                   ("error: -batch_reads with -gpus 2", base + ["-batch_reads", "333", "-gpus", "2"])]:
                    total += 1
                    same += compare(f"{name}: {what}", args.old, args.new, argv, {"FAUCET_SHARD_PROTOCOL": "presence"}, d)
            if c.paired and args.old_ref and args.new_ref:
                for what, env in [("plain", {}), ("FGPU_DEBUG_LONG_PAIRS_NOMEM=1", {"FGPU_DEBUG_LONG_PAIRS_NOMEM": "1"}),
                                  ("FAUCET_GPUS=2", {"FAUCET_GPUS": "2", "FAUCET_SHARD_PROTOCOL": "presence"})]:
                    total += 1
                    same += compare(f"{name}: reference + binding, {what}", args.old_ref, args.new_ref, base, env, d)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(f"{same} of {total} runs the same in exit code, stdout, stderr and files")


if __name__ == "__main__":
    main()
