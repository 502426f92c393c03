#!/bin/bash
# Kernel-trace cost of the model gradient (rti_wvjp_kernel) beside the plain adjoint (rti_vjp_kernel) at the headline shape, one job:
#   bash scripts/model_grad_cost.sh [OUT]    -> OUT/trace/ + OUT/summary.txt  (OUT: a new temporary directory if not given)
# One rocprofv3 --kernel-trace --stats run of scripts/model_grad_cost.py (200 steps, both adjoint kernels behind every step, on the same
# tape); the summary is each kernel's mean / median duration over its last 150 launches IN THAT ONE TRACE.
set -u
R=$PWD
O=${1:-$(mktemp -d)}; O=$(mkdir -p "$O" && cd "$O" && pwd)
(cd "$O" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -- python3 $R/scripts/model_grad_cost.py > $O/trace.log 2>&1) || { echo "trace failed ($?)"; tail -20 $O/trace.log; exit 1; }
python3 - $O <<'PY' | tee $O/summary.txt
import csv, glob, statistics as S, sys
per = {}
for f in glob.glob(f"{sys.argv[1]}/trace/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        for k in ("rti_kernel", "rti_vjp_kernel", "rti_wvjp_kernel"):
            if k + "I" in r["Kernel_Name"] or k + "<" in r["Kernel_Name"]:
                per.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
mean = {}
for k, d in sorted(per.items()):
    d = [x for _, x in sorted(d)][-150:]
    mean[k] = S.mean(d)
    print(f"{k}: {len(d)} launches, mean {mean[k] / 1e3:.2f} us, median {S.median(d) / 1e3:.2f} us, min {min(d) / 1e3:.2f} us")
print(f"rti_wvjp_kernel / rti_vjp_kernel: {mean['rti_wvjp_kernel'] / mean['rti_vjp_kernel']:.3f}")
PY
