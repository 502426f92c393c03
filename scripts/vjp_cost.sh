#!/bin/bash
# Kernel-trace cost of the adjoint against the parameter sensitivities at the headline shape, one job:
#   bash scripts/vjp_cost.sh [OUT]    -> OUT/{params,vjp}/ + OUT/summary.txt  (OUT: a new temporary directory if not given)
# Each setting (level 1 + parameter sensitivities; the plain step + tape + adjoint) is one rocprofv3 --kernel-trace --stats run of
# scripts/vjp_cost.py (200 steps); the summary is each kernel's mean / median duration over the last 150 launches and the per-step total of
# the setting.  Stops at the first failing run.
set -u
R=$PWD
O=${1:-$(mktemp -d)}; O=$(mkdir -p "$O" && cd "$O" && pwd)
for S in params vjp; do
  (cd "$O" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$S -- python3 $R/scripts/vjp_cost.py --setting $S > $O/$S.log 2>&1) || { echo "$S failed ($?)"; tail -20 $O/$S.log; exit 1; }
done
python3 - $O <<'PY' | tee $O/summary.txt
import csv, glob, statistics as S, sys
tot = {}
for s in ("params", "vjp"):
    per = {}
    for f in glob.glob(f"{sys.argv[1]}/{s}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for k in ("rti_kernel", "rti_psens_kernel", "rti_vjp_kernel"):
                if k in r["Kernel_Name"]:
                    per.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    tot[s] = 0.0
    for k, d in sorted(per.items()):
        d = [x for _, x in sorted(d)][-150:]
        m = S.mean(d)
        tot[s] += m
        print(f"{s} {k}: {len(d)} launches, mean {m / 1e3:.2f} us, median {S.median(d) / 1e3:.2f} us, min {min(d) / 1e3:.2f} us")
    print(f"{s}: {tot[s] / 1e3:.2f} us per step")
print(f"vjp / params: {tot['vjp'] / tot['params']:.2f}")
PY
