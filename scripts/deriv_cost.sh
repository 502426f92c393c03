#!/bin/bash
# Kernel-trace cost of the control step's derivatives at the headline shape, one job:
#   bash scripts/deriv_cost.sh SETTING... [-o OUT]   -> OUT/SETTING/ each + OUT/summary.txt  (OUT: a new temporary directory if not given)
# SETTING: off level1 level2 params vjp model jvp1 jvp8 (scripts/deriv_cost.py).  Each is one rocprofv3 --kernel-trace --stats run of
# scripts/deriv_cost.py (200 steps); the summary is, per setting, each control-step kernel's mean / median / minimum duration over its last
# 150 launches and their sum per step; then each sensitivity setting against `off`, vjp / params, jvp1 and jvp8 against vjp and params, and
# rti_wvjp_kernel / rti_vjp_kernel IN THE ONE `model` TRACE, for the settings that were run.  Stops at the first failing run.
set -u
R=$PWD
O=; SETTINGS=
while [ $# -gt 0 ]; do
  case $1 in -o) O=$2; shift 2;; *) SETTINGS="$SETTINGS $1"; shift;; esac
done
[ -n "$SETTINGS" ] || { echo "usage: bash scripts/deriv_cost.sh SETTING... [-o OUT]"; exit 2; }
O=${O:-$(mktemp -d)}; O=$(mkdir -p "$O" && cd "$O" && pwd)
for S in $SETTINGS; do
  (cd "$O" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$S -- python3 $R/scripts/deriv_cost.py --setting $S > $O/$S.log 2>&1) || { echo "$S failed ($?)"; tail -20 $O/$S.log; exit 1; }
done
python3 - $O $SETTINGS <<'PY' | tee $O/summary.txt
import csv, glob, statistics as S, sys
tot, mean = {}, {}
for s in sys.argv[2:]:
    per = {}
    for f in glob.glob(f"{sys.argv[1]}/{s}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for k in ("rti_kernel", "rti_sens_kernel", "rti_psens_kernel", "rti_vjp_kernel", "rti_wvjp_kernel", "rti_jvp_kernel"):
                if k + "I" in r["Kernel_Name"] or k + "<" in r["Kernel_Name"]:       # (mangled or demangled: rti_kernel alone, not the others)
                    per.setdefault(k, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    tot[s] = 0.0
    for k, d in sorted(per.items()):
        d = [x for _, x in sorted(d)][-150:]
        mean[s, k] = S.mean(d)
        tot[s] += mean[s, k]
        print(f"{s} {k}: {len(d)} launches, mean {mean[s, k] / 1e3:.2f} us, median {S.median(d) / 1e3:.2f} us, min {min(d) / 1e3:.2f} us")
    print(f"{s}: {tot[s] / 1e3:.2f} us per step")
for s in ("level1", "level2", "params"):
    if s in tot and "off" in tot:
        print(f"{s}: {100 * (tot[s] / tot['off'] - 1):+.1f} % vs off")
if "vjp" in tot and "params" in tot:
    print(f"vjp / params: {tot['vjp'] / tot['params']:.2f}")
for s in ("jvp1", "jvp8"):
    for o in ("vjp", "params"):
        if s in tot and o in tot:
            print(f"{s} / {o}: {tot[s] / tot[o]:.2f}")
if "model" in tot:
    print(f"rti_wvjp_kernel / rti_vjp_kernel: {mean['model', 'rti_wvjp_kernel'] / mean['model', 'rti_vjp_kernel']:.3f}")
PY
