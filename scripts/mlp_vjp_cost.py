"""Driver of scripts/mlp_vjp_cost.sh: at B = 1024, N = 20 launches the downwash network's forward (mlp_kernel) and its backward pass
(mlp_vjp_kernel + mlp_vjp_reduce_kernel) 60 times each for one gate setting, then times the backward of control_step_ndp next to the
backward of control_step_trajectory with HIP events (20 rounds each, medians).  Prints one line per figure."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ndp_nmpc_qd_amd as ndp  # noqa: E402
from ndp_nmpc_qd_amd import _lib, synth  # noqa: E402
from ndp_nmpc_qd_amd.torch_layer import control_step_ndp, control_step_trajectory  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--gate", choices=["open", "part"], default="open")
a = ap.parse_args()
B, N = 1024, 20
dev = torch.device("cuda", 0)
t = lambda x, dt=None: torch.tensor(np.ascontiguousarray(x), device=dev, dtype=dt)  # noqa: E731
b = synth.make_batch(B, seed=synth.SEED0, downwash=True)
ego_xy = b["ego_xy"] if a.gate == "part" else None          # the benchmark's batch: about 36 % of the gates open
e = ndp.BatchedNMPC(B, N=N, disturbance=True)
e.reset(b["xr"], b["ur"])
T = {k: t(b[k]) for k in ("x0", "xr", "ur", "other")}
exy = None if ego_xy is None else t(ego_xy)
if exy is not None:
    d = b["other"][:, 0, :2] - b["ego_xy"]
    print(f"gate {a.gate}: {float(((d ** 2).sum(axis=1) < e.cfg.r_horiz ** 2).mean()):.3f} of the instances open")
f = torch.empty(B, N + 1, 3, dtype=torch.float32, device=dev)
gf = t(np.random.default_rng(0).normal(size=(B, N + 1, 3)))
gz = torch.empty(B, N + 1, 6, dtype=torch.float64, device=dev)
gw = torch.empty(_lib.MLP_NPARAM, dtype=torch.float32, device=dev)
s = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
with torch.cuda.stream(s):
    for _ in range(60):
        e.downwash_device(T["other"], T["xr"], f, ego_xy=exy, stream=s)
        e.downwash_vjp_device(T["other"], T["xr"], gf, ego_xy=exy, gz=gz, gw=gw, stream=s)
    s.synchronize()
    w = t(_lib.load_weights()).requires_grad_(True)
    up = (torch.randn(B, 4, device=dev, dtype=torch.float64), torch.randn(B, N + 1, 10, device=dev, dtype=torch.float64),
          torch.randn(B, N, 4, device=dev, dtype=torch.float64))
    for name in ("trajectory", "ndp"):
        ms = []
        for _ in range(25):
            leaf = {k: T[k].clone().requires_grad_(True) for k in ("x0", "xr", "ur")}
            if name == "ndp":
                oth = T["other"].clone().requires_grad_(True)
                out = control_step_ndp(e, leaf["x0"], leaf["xr"], leaf["ur"], oth, ego_xy=exy, weights=w)
                wrt = (leaf["x0"], leaf["xr"], leaf["ur"], oth, w)
            else:
                out = control_step_trajectory(e, leaf["x0"], leaf["xr"], leaf["ur"], other=T["other"], ego_xy=exy)
                wrt = (leaf["x0"], leaf["xr"], leaf["ur"])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            torch.autograd.grad(out, wrt, up)
            e1.record(s)
            s.synchronize()
            ms.append(e0.elapsed_time(e1))
        print(f"gate {a.gate}: backward of control_step_{name}: median {statistics.median(ms[5:]) * 1e3:.1f} us over {len(ms) - 5} rounds")
e.close()
