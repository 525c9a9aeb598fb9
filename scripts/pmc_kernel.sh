#!/bin/bash
# Runs ON THE GPU BOX: SQ counters of one kernel (regex $2) of a short bench run; env assignments after that are exported first.
#   gpurun -- 'bash scripts/pmc_kernel.sh tag k_walk [VAR=val ...]'
tag=$1; regex=$2; shift 2
for kv in "$@"; do export "$kv"; done
root=${GRAFT_REPO_ROOT:-$(pwd)}
out=$root/gpurun_out/pmc_$tag
mkdir -p "$out"
export TMPDIR=/tmp
cd /tmp
rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU --kernel-include-regex "$regex" --output-format csv -d "$out/sq1" -o run -- python3 "$root/bench.py" --full --steps 1 --warmup 0 --no-cpu --no-ceilings > "$out/b1.json" 2> "$out/b1.err"
rocprofv3 --pmc SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM SQ_INSTS_FLAT SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_THREAD_CYCLES_VALU SQ_INSTS_LDS --kernel-include-regex "$regex" --output-format csv -d "$out/sq2" -o run -- python3 "$root/bench.py" --full --steps 1 --warmup 0 --no-cpu --no-ceilings > "$out/b2.json" 2> "$out/b2.err"
find "$out" \( -name "*.db" \) -delete
python3 - "$out" <<'PY'
import csv, glob, os, sys
acc = {}
for f in glob.glob(os.path.join(sys.argv[1], "**", "*counter_collection.csv"), recursive=True):
    for row in csv.DictReader(open(f)):
        k = row["Kernel_Name"].split("(")[0][-40:]
        a = acc.setdefault((k, row["Counter_Name"]), [0, 0.0])
        a[0] += 1; a[1] += float(row["Counter_Value"])
for (k, c), (n, v) in sorted(acc.items()):
    print(f"{k:42s} {c:24s} launches {n:5d} total {v:.4g} per-launch {v/n:.4g}")
PY
