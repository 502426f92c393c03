#!/bin/bash
# Kernel-trace cost of the downwash network's backward pass next to its forward at B = 1024, N = 20, one job:
#   bash scripts/mlp_vjp_cost.sh [OUT]    -> OUT/{open,part}/ + OUT/summary.txt  (OUT: a new temporary directory if not given)
# Each gate setting (all open; the benchmark's ~36 % open) is one rocprofv3 --kernel-trace --stats run of scripts/mlp_vjp_cost.py; the
# summary is each kernel's mean / median duration over its last 50 launches, the ratio (backward + reduction) / forward from that same
# run, and the driver's HIP-event times of the two layers' backward passes.  Stops at the first failing run.
set -u
R=$PWD
O=${1:-$(mktemp -d)}; O=$(mkdir -p "$O" && cd "$O" && pwd)
for S in open part; do
  (cd "$O" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$S -- python3 $R/scripts/mlp_vjp_cost.py --gate $S > $O/$S.log 2>&1) || { echo "$S failed ($?)"; tail -20 $O/$S.log; exit 1; }
done
python3 - $O <<'PY' | tee $O/summary.txt
import csv, glob, statistics as S, sys
for s in ("open", "part"):
    per = {}
    for f in glob.glob(f"{sys.argv[1]}/{s}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for k in ("mlp_kernel", "mlp_vjp_kernel", "mlp_vjp_reduce_kernel"):
                if "::" + k + "(" in r["Kernel_Name"]:
                    per.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    m = {}
    for k, d in sorted(per.items()):
        d = [x for _, x in sorted(d)][5:55]               # the stand-alone launches behind the warm-up, not the layers' at the end
        m[k] = S.mean(d)
        print(f"{s} {k}: {len(d)} launches, mean {m[k] / 1e3:.2f} us, median {S.median(d) / 1e3:.2f} us, min {min(d) / 1e3:.2f} us")
    print(f"{s}: (mlp_vjp_kernel + mlp_vjp_reduce_kernel) / mlp_kernel = {(m['mlp_vjp_kernel'] + m['mlp_vjp_reduce_kernel']) / m['mlp_kernel']:.2f}")
    print("".join(l for l in open(f"{sys.argv[1]}/{s}.log") if l.startswith("gate ")), end="")
PY
