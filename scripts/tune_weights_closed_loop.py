#!/usr/bin/env python3
"""Tunes the controller's cost weights on a CLOSED-LOOP tracking loss: a few Adam steps on Qd [10], Rd [4] through
torch_layer.closed_loop -- one call forward, one call back per iteration -- and the loss printed per iteration.

    python scripts/tune_weights_closed_loop.py [--batch 256] [--ticks 20] [--iters 10] [--lr 0.05] [--horizon 20]

The flight: the mixed workload (bench.py's: perturbed starts, 0.5 m / 1 m/s / 0.15) sliding along its figure-eights, `ticks` control
periods, a seeded force on the plant the controller does not see (the model mismatch that makes the weights matter).  The loss: the
mean squared distance of the plant's position and velocity after tick k from the reference at that time (node 0 of tick k + 1's window).
The weights are optimised as Qd0 exp(s), Rd0 exp(r): positive whatever Adam does, a weight that is 0 stays 0.  Every iteration restarts the
engine from tick 0's window, so the iterations differ in the weights alone.  A vehicle whose step fails contributes nothing to the
gradient (torch_layer.closed_loop's convention); the last tick's are counted."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIXED = dict(pos_sigma=0.5, vel_sigma=1.0, quat_sigma=0.15)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--force", type=float, default=1.0, help="sigma of the force on the plant, N")
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import synth
    from ndp_nmpc_qd_amd import torch_layer as TL
    from ndp_nmpc_qd_amd.params import nmpc_params as CP
    dev = torch.device("cuda:0")
    B, K, N, dt = a.batch, a.ticks, a.horizon, CP.ts_nmpc
    b = [synth.make_batch(B, N=N, seed=synth.SEED0 + 40, t0=k * dt, **MIXED) for k in range(K + 1)]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)      # noqa: E731
    x0, xr, ur = t(b[0]["x0"]), t(np.stack([v["xr"] for v in b[:K]])), t(np.stack([v["ur"] for v in b[:K]]))
    target = t(np.stack([v["xr"][:, 0, :6] for v in b[1:]]))                # [K,B,6]: the reference at the time x_{k+1} is reached
    fp = t(np.random.default_rng(7).normal(0.0, a.force, (K, B, 3)))
    eng = ndp.BatchedNMPC(B, N=N)
    Qd0 = torch.tensor(list(eng.cfg.Qd), dtype=torch.float64)
    Rd0 = torch.tensor(list(eng.cfg.Rd), dtype=torch.float64)
    s = torch.zeros(10, dtype=torch.float64, requires_grad=True)
    r = torch.zeros(4, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([s, r], lr=a.lr)
    for it in range(a.iters):
        opt.zero_grad()
        eng.reset(b[0]["xr"], b[0]["ur"])
        Qd, Rd = Qd0 * torch.exp(s), Rd0 * torch.exp(r)
        xs, us, Xs = TL.closed_loop(eng, x0, xr, ur, fp=fp, Qd=Qd, Rd=Rd, dt=dt)
        loss = ((xs[:, :, :6] - target) ** 2).sum(dim=2).mean()
        loss.backward()
        opt.step()
        failed = int((eng.status()[0] != 0).sum())                          # (the last tick's status words)
        print(f"iteration {it}: loss {float(loss):.6e}  |dL/ds| {float(s.grad.abs().max()):.2e}  |dL/dr| {float(r.grad.abs().max()):.2e}  "
              f"failed steps in the last tick {failed}", flush=True)
    print("Qd", (Qd0 * torch.exp(s)).tolist())
    print("Rd", (Rd0 * torch.exp(r)).tolist())
    eng.close()


if __name__ == "__main__":
    main()
