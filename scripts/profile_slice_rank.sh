#!/bin/bash
# rocprofv3 kernel statistics of ONE rank of pass 1 by filter slices (scripts/slice_rank_step.py: rank N/2 of N over config 4's whole stream), in a
# run of its own (on an MI355X):   bash scripts/profile_slice_rank.sh [N]   -> $OUT_DIR/slice_rank_kernel_stats.csv  (default profiles/out/prof_slice)
n=${1:-8}
root=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
out=${OUT_DIR:-$root/profiles/out/prof_slice}
mkdir -p "$out"
export TMPDIR=/tmp
cd /tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/stats" -o run -- python3 "$root/scripts/slice_rank_step.py" "$n" > "$out/step.json" 2> "$out/step.err"
rc=$?
echo "rc=$rc"
[ $rc -eq 0 ] || exit $rc
find "$out" \( -name "*kernel_trace.csv" -o -name "*.db" \) -delete
cat "$out/step.json"
python3 - <<PY
import csv, glob
f = glob.glob("$out/**/*kernel_stats.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if "k_" in r["Name"] and "at::" not in r["Name"] and "rocprim" not in r["Name"]]
w = csv.writer(open("$out/slice_rank_kernel_stats.csv", "w"))
w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs"])
for r in rows:
    n = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
    w.writerow([n, r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["Percentage"], r["MinNs"], r["MaxNs"]])
    print(f"{n[:40]:40s} x{r['Calls']:>6s} {int(r['TotalDurationNs'])/1e6:10.1f} ms")
PY
