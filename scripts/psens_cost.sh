#!/bin/bash
# Kernel-trace cost of the parameter sensitivities at the headline shape, one job:
#   bash scripts/psens_cost.sh [OUT]    -> OUT/{off,level1,params}/ + OUT/summary.txt  (OUT: a new temporary directory if not given)
# Each setting (sensitivities off; level 1; level 1 + parameters) is one rocprofv3 --kernel-trace --stats run of scripts/psens_cost.py
# (200 steps); the summary is the control-step kernel's mean / median duration over the last 150 launches.  Stops at the first failing run.
set -u
R=$PWD
O=${1:-$(mktemp -d)}; O=$(mkdir -p "$O" && cd "$O" && pwd)
for S in off level1 params; do
  (cd "$O" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$S -- python3 $R/scripts/psens_cost.py --setting $S > $O/$S.log 2>&1) || { echo "$S failed ($?)"; tail -20 $O/$S.log; exit 1; }
done
python3 - $O <<'PY' | tee $O/summary.txt
import csv, glob, statistics as S, sys
base = None
for s in ("off", "level1", "params"):
    d = []
    for f in glob.glob(f"{sys.argv[1]}/{s}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if any(k in r["Kernel_Name"] for k in ("rti_kernel", "rti_sens_kernel", "rti_psens_kernel")):
                d.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    d = [x for _, x in sorted(d)][-150:]
    m = S.mean(d)
    base = base or m
    print(f"{s}: {len(d)} launches, mean {m / 1e3:.2f} us, median {S.median(d) / 1e3:.2f} us, min {min(d) / 1e3:.2f} us  ({100 * (m / base - 1):+.1f} % vs off)")
PY
