#!/bin/bash
# Kernel-trace cost of the initial-state sensitivities (levels 0, 1, 2) at the headline shape, one job:
#   bash scripts/sens_cost.sh [OUT]    -> OUT/{level0,level1,level2}/ + OUT/summary.txt  (OUT: a new temporary directory if not given)
# Each level is one rocprofv3 --kernel-trace --stats run of scripts/sens_cost.py (200 steps); the summary is the control-step kernel's
# mean / median duration over the last 150 launches.  Stops at the first failing run.
set -u
R=$PWD
O=${1:-$(mktemp -d)}; O=$(mkdir -p "$O" && cd "$O" && pwd)
for L in 0 1 2; do
  (cd "$O" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/level$L -- python3 $R/scripts/sens_cost.py --level $L > $O/level$L.log 2>&1) || { echo "level $L failed ($?)"; tail -20 $O/level$L.log; exit 1; }
done
python3 - $O <<'PY' | tee $O/summary.txt
import csv, glob, statistics as S, sys
base = None
for L in (0, 1, 2):
    d = []
    for f in glob.glob(f"{sys.argv[1]}/level{L}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "rti_kernel" in r["Kernel_Name"] or "rti_sens_kernel" in r["Kernel_Name"]:
                d.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    d = [x for _, x in sorted(d)][-150:]
    m = S.mean(d)
    base = base or m
    print(f"level {L}: {len(d)} launches, mean {m / 1e3:.2f} us, median {S.median(d) / 1e3:.2f} us, min {min(d) / 1e3:.2f} us  ({100 * (m / base - 1):+.1f} % vs level 0)")
PY
