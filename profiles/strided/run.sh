#!/bin/bash
# The two GPU steps of profiles/strided/README.md, from the repository root: the timing run, then -- only if it succeeded -- the
# kernel trace in a run of its own.  Each step under its own time limit; output under $1 (default ./strided_out).
set -o pipefail
out=${1:-strided_out}
mkdir -p "$out"
timeout -k 10 420 python profiles/strided/measure.py --out "$out" 2>&1 | tee "$out/measure.log" &&
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/trace" -- python profiles/strided/measure.py --profile > "$out/rocprof.log" 2>&1 &&
python - "$out" <<'PY'
import csv, glob, sys
f = sorted(glob.glob(sys.argv[1] + "/trace/**/*kernel_stats.csv", recursive=True))[0]
rows = list(csv.DictReader(open(f)))
with open(sys.argv[1] + "/kernel_stats.txt", "w") as fh:
    for r in rows[:28]:
        line = " | ".join((r["Name"][:110], r["Calls"], r["TotalDurationNs"], r["AverageNs"], r["Percentage"]))
        print(line)
        fh.write(line + "\n")
PY
