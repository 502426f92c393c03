#!/bin/bash
# Kernel-trace cost of the downwash network's forward mode next to its forward and its backward pass at B = 1024, N = 20, all gates open:
#   bash scripts/mlp_jvp_cost.sh [OUT]    -> OUT/trace/ + OUT/summary.txt  (OUT: a new temporary directory if not given)
# One rocprofv3 --kernel-trace --stats run of scripts/mlp_jvp_cost.py; the summary is each kernel's mean / median / min duration over its
# last 25 launches of 30, mlp_jvp_kernel's four blocks (T = 1 and T = 8, without and with a direction of the weights) told apart by their
# order in time.
set -u
R=$PWD
O=${1:-$(mktemp -d)}; O=$(mkdir -p "$O" && cd "$O" && pwd)
(cd "$O" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -- python3 $R/scripts/mlp_jvp_cost.py > $O/run.log 2>&1) || { echo "run failed ($?)"; tail -20 $O/run.log; exit 1; }
python3 - $O <<'PY' | tee $O/summary.txt
import csv, glob, statistics as S, sys
per = {}
for f in glob.glob(f"{sys.argv[1]}/trace/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        for k in ("mlp_kernel", "mlp_vjp_kernel", "mlp_vjp_reduce_kernel", "mlp_jvp_kernel"):
            if "::" + k + "(" in r["Kernel_Name"]:
                per.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
def line(name, d):
    d = d[5:]
    print(f"{name}: {len(d)} launches, mean {S.mean(d) / 1e3:.2f} us, median {S.median(d) / 1e3:.2f} us, min {min(d) / 1e3:.2f} us")
for k in ("mlp_kernel", "mlp_vjp_kernel", "mlp_vjp_reduce_kernel"):
    line(k, [x for _, x in sorted(per[k])])
j = [x for _, x in sorted(per["mlp_jvp_kernel"])]
assert len(j) == 120, len(j)
for i, name in enumerate(("T = 1", "T = 1 with d_tw", "T = 8", "T = 8 with d_tw")):
    line("mlp_jvp_kernel " + name, j[30 * i:30 * i + 30])
PY
