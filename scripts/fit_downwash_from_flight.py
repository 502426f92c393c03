#!/usr/bin/env python3
"""A plumbing demonstration of the plant-side gradient (torch_layer.plant_force -> plant_step): fit the downwash network to logged STATES
of stacked pairs, with no force labels.

    python scripts/fit_downwash_from_flight.py [--pairs 32] [--ticks 40] [--epochs 200]

Stacked pairs (the lower vehicle hears the upper one, dz above it, and the upper one hears the lower) fly `ticks` ticks at hover thrust under
the SHIPPED weights: per tick f = plant_force(x), x = plant_step(x, u, f), every state logged.  Then a copy of the weights is perturbed
(every parameter by 2 % of its own size, relative, N(0, 1)) and fitted with DownwashAdamSN to the logged states alone: every logged tick
is one row of a batch of pairs x 2 x ticks vehicles, the model steps each one tick ahead from its logged state (plant_force -> plant_step,
one call each), and the loss is the mean square of mass x (velocity after the tick, predicted minus logged) / dt -- the force error in
N^2 as the states show it.  Prints the loss per epoch (every --every epochs) and a JSON line at the end.

What this is: synthetic data made by the very network that is fitted -- it shows that a gradient reaches the weights through the plant
and that a loss on states goes down, and says nothing about real flights."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--dz", type=float, default=0.5)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import _lib
    from ndp_nmpc_qd_amd.params import nmpc_params as CP
    from ndp_nmpc_qd_amd.torch_layer import DownwashAdamSN, plant_force, plant_step
    dev = torch.device("cuda:0")
    t = lambda v, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(v)).to(dev, dt)  # noqa: E731
    rng = np.random.default_rng(1)
    B, K, dt = 2 * a.pairs, a.ticks, CP.ts_nmpc
    # ---- the flight under the shipped weights: vehicle 2 i below vehicle 2 i + 1, a few centimetres and cm/s apart in xy
    x0 = np.zeros((B, 10))
    x0[:, 6] = 1.0
    x0[:, :2] = np.repeat(rng.uniform(-3.0, 3.0, (a.pairs, 2)), 2, axis=0) + rng.normal(0.0, 0.05, (B, 2))
    x0[1::2, 2] = a.dz
    x0[:, 3:6] = rng.normal(0.0, 0.1, (B, 3))
    idx = (np.arange(B) ^ 1).astype(np.int32)
    u = np.zeros((B, 4))
    u[:, 3] = CP.gravity                                        # hover thrust, no body rates
    blob = _lib.load_weights()
    fly = ndp.BatchedNMPC(B, N=CP.N_node, disturbance=True)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream), torch.no_grad():
        x, ut, it, log = t(x0), t(u), t(idx, torch.int32), [t(x0)]
        for _ in range(K):
            x = plant_step(fly, x, ut, plant_force(fly, x, it), dt=dt)
            log.append(x)
        stream.synchronize()
    fly.close()
    log = torch.stack(log)                                      # [K+1,B,10]
    # ---- the data set: row k B + v is vehicle v at tick k; its neighbour is row k B + idx[v]
    before, after = log[:-1].reshape(K * B, 10).contiguous(), log[1:].reshape(K * B, 10).contiguous()
    rows = t((np.arange(K)[:, None] * B + idx[None]).reshape(-1), torch.int32)
    uu = ut.repeat(K, 1).contiguous()
    eng = ndp.BatchedNMPC(K * B, N=CP.N_node, disturbance=True)
    w = torch.nn.Parameter(t(blob * (1.0 + 0.02 * rng.normal(size=blob.shape)), torch.float32))
    opt = DownwashAdamSN(w, eng, lr=a.lr)
    mass = float(eng.cfg.mass)

    def loss_of(weights):
        pred = plant_step(eng, before, uu, plant_force(eng, before, rows, weights=weights), dt=dt)
        return ((mass / dt * (pred[:, 3:6] - after[:, 3:6])) ** 2).mean()

    losses = []
    with torch.cuda.stream(stream):
        with torch.no_grad():
            shipped = float(loss_of(t(blob, torch.float32)))
        for epoch in range(a.epochs):
            opt.zero_grad()
            loss = loss_of(w)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            if epoch % a.every == 0 or epoch + 1 == a.epochs:
                print(f"epoch {epoch + 1}: loss {losses[-1]:.6e} N^2", flush=True)
        with torch.no_grad():
            losses.append(float(loss_of(w.detach())))
        stream.synchronize()
    eng.close()
    print(json.dumps({"experiment": "fit of the downwash weights to logged STATES of stacked pairs through plant_force -> plant_step, no force "
                                    "labels (synthetic data from the same network: a plumbing demonstration, not evidence about real flights)",
                      "pairs": a.pairs, "ticks": K, "dz": a.dz, "rows": K * B, "adam": {"epochs": a.epochs, "lr": a.lr},
                      "loss_shipped_weights_N2": shipped, "loss_before_N2": losses[0], "loss_after_N2": losses[-1],
                      "loss_every": losses[::a.every]}))


if __name__ == "__main__":
    main()
