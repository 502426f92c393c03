"""Driver of scripts/mlp_jvp_cost.sh: at B = 1024, N = 20, all gates open, launches the downwash network's forward (mlp_kernel), its backward
pass (mlp_vjp_kernel + mlp_vjp_reduce_kernel) and its forward mode (mlp_jvp_kernel) 30 times each, the forward mode in four blocks in this
order: T = 1 without and with a direction of the weights, T = 8 without and with one."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ndp_nmpc_qd_amd as ndp  # noqa: E402
from ndp_nmpc_qd_amd import _lib, synth  # noqa: E402

B, N, REPS = 1024, 20, 30
dev = torch.device("cuda", 0)
t = lambda x, dt=None: torch.tensor(np.ascontiguousarray(x), device=dev, dtype=dt)  # noqa: E731
b = synth.make_batch(B, seed=synth.SEED0, downwash=True)
e = ndp.BatchedNMPC(B, N=N, disturbance=True)
T = {k: t(b[k]) for k in ("xr", "other")}
rng = np.random.default_rng(0)
f = torch.empty(B, N + 1, 3, dtype=torch.float32, device=dev)
gf = t(rng.normal(size=(B, N + 1, 3)))
gz = torch.empty(B, N + 1, 6, dtype=torch.float64, device=dev)
gw = torch.empty(_lib.MLP_NPARAM, dtype=torch.float32, device=dev)
tz = t(rng.normal(size=(B, 8, N + 1, 6)))
tw = t((_lib.load_weights()[None] * 0.1 * rng.normal(size=(8, _lib.MLP_NPARAM))).astype(np.float32))
df = torch.empty(B, 8, N + 1, 3, dtype=torch.float64, device=dev)
s = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()
with torch.cuda.stream(s):
    for _ in range(REPS):
        e.downwash_device(T["other"], T["xr"], f, stream=s)
    for _ in range(REPS):
        e.downwash_vjp_device(T["other"], T["xr"], gf, gz=gz, gw=gw, stream=s)
    for nt in (1, 8):
        z, w, d = (tz, tw, df) if nt == 8 else (tz[:, 0].contiguous(), tw[0].contiguous(), df[:, 0].contiguous())
        for with_w in (False, True):
            for _ in range(REPS):
                e.downwash_jvp_device(T["other"], T["xr"], tz=z, tw=w if with_w else None, n_tan=nt, df=d, stream=s)
    s.synchronize()
print(f"launched {REPS} x (mlp_kernel, mlp_vjp_kernel, mlp_jvp_kernel T=1, T=1 + tw, T=8, T=8 + tw)")
e.close()
