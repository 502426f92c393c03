#!/usr/bin/env python3
"""A plumbing demonstration of the K-neighbour gradient (torch_layer.downwash_multi): fit the downwash network to the force recorded on
the lowest vehicle of stacked triples.

    python scripts/fit_downwash_multi.py [--triples 16] [--ticks 210] [--steps 300]

scripts/formation_rollout.py's stacked triples fly blind (ndp_rollout_formation_multi_device, no compensation); the plant force on every
vehicle and the states are logged.  The lowest vehicle of a triple hears the two above it, so its recorded force is the SUM of two network
rows -- data the single-neighbour gradient cannot be fitted to.  A copy of the shipped weights is perturbed (every parameter by 2 % of its
own size, relative, N(0, 1)) and fitted by SGD through downwash_multi: 21 consecutive ticks of a vehicle lie on the 21 nodes of an
instance, the two neighbours' states on two rows of `other`, the gates open.  Prints the loss before and after as one JSON line.

What this is: synthetic data made by the very network that is fitted, under the superposition the plant itself assumes -- it shows that the
gradient arrives and that a loss goes down, and says nothing about whether superposing pair forces describes real stacked flight."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triples", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=210)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--lr", type=float, default=3e-4)      # (with momentum 0.9; 1e-3 overshoots on this data: the loss rises first)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--dz", type=float, default=0.5)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from formation_rollout import set_trajectory, stacked_triples
    from ndp_nmpc_qd_amd import _lib
    from ndp_nmpc_qd_amd.params import nmpc_params as CP
    from ndp_nmpc_qd_amd.torch_layer import downwash_multi
    dev = torch.device("cuda:0")
    N = CP.N_node
    B, K = 3 * a.triples, a.ticks - a.ticks % (N + 1)
    # ---- the flight: blind controllers, the summed force on the plant
    tr, idx = stacked_triples(a.triples, a.dz, n_seg=int(np.ceil((K * CP.ts_nmpc + 2.5) / 0.5)))
    fly = ndp.BatchedNMPC(B, load_mlp=True)
    set_trajectory(fly, tr)
    x0 = fly.ref_window(np.zeros(B))[0][:, 0].copy()
    x = torch.from_numpy(x0).to(dev)
    log = torch.empty(K, B, 10, dtype=torch.float64, device=dev)
    log_f = torch.empty(K, B, 3, dtype=torch.float64, device=dev)
    ws = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fly.rollout_formation_multi_device(K, x, torch.from_numpy(idx).to(dev), log=log, log_f=log_f, worst_status=ws)
    fly.synchronize()
    before = np.concatenate([x0[None], log.cpu().numpy()[:-1]])          # the states the force of tick k was made from
    force = log_f.cpu().numpy()
    fly.close()
    # ---- the data set: instance = (lowest vehicle, block of N + 1 ticks), node = tick, slot k on row 2 i + k of `other`
    low = np.arange(0, B, 3)
    blocks = K // (N + 1)
    win = lambda v: before[:, v].reshape(blocks, N + 1, len(v), 10).transpose(0, 2, 1, 3).reshape(-1, N + 1, 10)  # noqa: E731
    ego = win(low)
    Bf = ego.shape[0]
    other = np.stack([win(idx[low, 0]), win(idx[low, 1])], axis=1).reshape(2 * Bf, N + 1, 10)
    target = force[:, low].reshape(blocks, N + 1, len(low), 3).transpose(0, 2, 1, 3).reshape(Bf, N + 1, 3)
    t = lambda v, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(v)).to(dev, dt)  # noqa: E731
    ego_t, other_t, target_t = t(ego), t(other), t(target, torch.float32)
    idx_t = torch.arange(2 * Bf, dtype=torch.int32, device=dev).reshape(Bf, 2)
    # ---- the fit
    eng = ndp.BatchedNMPC(Bf, N=N, disturbance=True)
    blob = _lib.load_weights()
    rng = np.random.default_rng(3)
    w = torch.nn.Parameter(t(blob * (1.0 + 0.02 * rng.normal(size=blob.shape)), torch.float32))
    opt = torch.optim.SGD([w], lr=a.lr, momentum=a.momentum)
    stream = torch.cuda.Stream(device=dev)
    losses = []
    with torch.cuda.stream(stream):
        loss_of = lambda: ((downwash_multi(eng, other_t, idx_t, ego_t, weights=w) - target_t) ** 2).mean()  # noqa: E731
        shipped = float(((downwash_multi(eng, other_t, idx_t, ego_t, weights=t(blob, torch.float32)) - target_t) ** 2).mean())
        for _ in range(a.steps):
            opt.zero_grad()
            loss = loss_of()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        losses.append(float(loss_of().detach()))
        stream.synchronize()
    eng.close()
    print(json.dumps({"experiment": "fit of the downwash weights to the summed force recorded on the lowest vehicle of stacked triples, "
                                    "through downwash_multi (synthetic data: a plumbing demonstration, not evidence about superposition)",
                      "triples": a.triples, "ticks": K, "dz": a.dz, "instances": Bf, "samples": Bf * (N + 1), "worst_status": int(ws.max()),
                      "mean_square_force_N2": float((target ** 2).mean()), "sgd": {"steps": a.steps, "lr": a.lr, "momentum": a.momentum},
                      "loss_shipped_weights": shipped, "loss_before": losses[0], "loss_after": losses[-1],
                      "loss_every_50": losses[::50]}))


if __name__ == "__main__":
    main()
