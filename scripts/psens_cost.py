#!/usr/bin/env python3
"""The cost of the parameter sensitivities: K control steps of the headline shape (B = 1024, N = 20, fused downwash, device pointers) with
sensitivities off, at level 1, or at level 1 with parameter sensitivities.  Run under rocprofv3 by scripts/psens_cost.sh, which compares
the control-step kernels' durations (rti_kernel, rti_sens_kernel, rti_psens_kernel)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setting", choices=("off", "level1", "params"), default="off")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    a = ap.parse_args()
    import torch

    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import synth
    b = synth.make_batch(a.batch, seed=synth.SEED0, downwash=True)
    eng = ndp.BatchedNMPC(a.batch, disturbance=True)
    eng.reset(b["xr"], b["ur"])
    if a.setting != "off":
        eng.enable_sensitivity(1)
    if a.setting == "params":
        eng.enable_param_sensitivity()
    dev = torch.device("cuda", 0)
    t = {k: torch.tensor(b[k], device=dev) for k in ("x0", "xr", "ur", "other", "ego_xy")}
    u0 = torch.empty(a.batch, 4, dtype=torch.float64, device=dev)
    step = eng.bind_update_device(t["x0"], t["xr"], t["ur"], u0, other=t["other"], ego_xy=t["ego_xy"])
    for _ in range(a.steps):
        step()
    eng.synchronize()
    st, it = eng.status()
    print(f"{a.setting}: {a.steps} steps, status nonzero {int((st != 0).sum())}, interior point {int((it > 0).sum())}")


if __name__ == "__main__":
    main()
