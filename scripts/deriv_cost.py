#!/usr/bin/env python3
"""The cost of the control step's derivatives: K control steps of the headline shape (B = 1024, N = 20, fused downwash, device pointers) on
one side stream, in one of these settings:
  off      the plain step (rti_kernel)
  level1   initial-state sensitivities at level 1 (rti_sens_kernel);  level2: at level 2
  params   level 1 plus parameter sensitivities (rti_psens_kernel): what the torch layer's control_step needs
  vjp      the plain step with one tape recorded before it and one adjoint launch behind it (rti_vjp_kernel): what control_step_trajectory
           does for a backward through every step
  model    as vjp, with BOTH adjoint launches behind every step on the same tape and upstream gradient -- ndp_step_vjp_device
           (rti_vjp_kernel) and ndp_step_vjp_model_device (rti_wvjp_kernel)
  jvp1     the plain step with one tape recorded before it and one forward-mode launch behind it (rti_jvp_kernel) along ONE direction
           (tx0, txr, tur and tf all given); jvp8: along eight directions in the one launch
Run under rocprofv3 by scripts/deriv_cost.sh, which compares the kernels' durations."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setting", choices=("off", "level1", "level2", "params", "vjp", "model", "jvp1", "jvp8"), default="off")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    a = ap.parse_args()
    import torch

    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import synth
    b = synth.make_batch(a.batch, seed=synth.SEED0, downwash=True)
    eng = ndp.BatchedNMPC(a.batch, disturbance=True)
    eng.reset(b["xr"], b["ur"])
    if a.setting in ("level1", "level2", "params"):
        eng.enable_sensitivity(2 if a.setting == "level2" else 1)
    if a.setting == "params":
        eng.enable_param_sensitivity()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    t = {k: torch.tensor(b[k], device=dev) for k in ("x0", "xr", "ur", "other", "ego_xy")}
    u0 = torch.empty(a.batch, 4, dtype=torch.float64, device=dev)
    g = torch.randn(a.batch, 4, dtype=torch.float64, device=dev)
    out = [torch.empty(*shape, dtype=torch.float64, device=dev) for shape in
           ((a.batch, 10), (a.batch, 21, 10), (a.batch, 20, 4), (a.batch, 21, 3), (a.batch, 16))]
    gmodels = {"vjp": (None,), "model": (None, out[4])}.get(a.setting, ())      # one adjoint launch behind the step for each
    T = {"jvp1": 1, "jvp8": 8}.get(a.setting, 0)
    tan = [torch.randn(a.batch, T, *shape, dtype=torch.float64, device=dev) for shape in ((10,), (21, 10), (20, 4), (21, 3))] if T else []
    dout = [torch.empty(a.batch, T, *shape, dtype=torch.float64, device=dev) for shape in ((4,), (21, 10), (20, 4))] if T else []
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        step = eng.bind_update_device(t["x0"], t["xr"], t["ur"], u0, other=t["other"], ego_xy=t["ego_xy"], stream=s)
        for _ in range(a.steps):
            tape = eng.record_tape(s) if gmodels or T else None
            step()
            for gm in gmodels:
                eng.step_vjp_device(t["x0"], t["xr"], t["ur"], tape, gu0=g, f=eng.device_force(), gx0=out[0], gxr=out[1], gur=out[2],
                                    gf=out[3], gmodel=gm, stream=s)
            if T:
                eng.step_jvp_device(t["x0"], t["xr"], t["ur"], tape, *tan, f=eng.device_force(), du0=dout[0], dX=dout[1], dU=dout[2], stream=s)
    s.synchronize()
    eng.synchronize()
    st, it = eng.status()
    print(f"{a.setting}: {a.steps} steps, status nonzero {int((st != 0).sum())}, interior point {int((it > 0).sum())}")


if __name__ == "__main__":
    main()
