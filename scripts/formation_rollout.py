#!/usr/bin/env python3
"""The closed-loop formation experiment on the device (formation form): pairs of vehicles on figure-eights, the
neighbour flying the same path dz above (dz < 0: below) the ego vehicle, the shipped downwash network acting on the plant at the
vehicles' actual relative state.  Both controllers -- NMPC (blind) and NDP (predicts the force from the neighbour's reference window) --
for dz in {0.5, 1.0, -0.5} and plant_scale in {1.0, 0.7, 1.3} (the model-mismatch knob), one ndp_rollout_formation_device call each.

    python scripts/formation_rollout.py [--pairs 8] [--ticks 250] [--skip 50]

Prints one JSON line: per (dz, plant_scale, controller) the z-RMSE over ticks skip.. of the lower and the upper vehicle of the pairs
(mean and max over the pairs), the peak |force| and the worst status."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stacked_pairs(pairs, dz, seed=7, n_seg=16, t_seg=0.5):
    """(trajectory dict for ref_set_trajectory, other_index int32[2 pairs]): vehicle 2k + 1 flies vehicle 2k's figure-eight (omega in
    [0.5, 1] rad/s) dz above it; other_index = i ^ 1."""
    from ndp_nmpc_qd_amd import synth
    B = 2 * pairs
    tr = synth.figure_eight_traj(B, seed=seed, n_seg=n_seg, t_seg=t_seg, omega_range=(0.5, 1.0))
    for k in ("coeff_x", "coeff_y", "coeff_z", "coeff_yaw", "time_cum", "time_seg", "final_pt"):
        tr[k][1::2] = tr[k][0::2]
    tr["coeff_z"][1::2, 0::8] += dz
    tr["final_pt"][1::2, 2] += dz
    return tr, (np.arange(B, dtype=np.int32) ^ 1).astype(np.int32)


def set_trajectory(eng, tr):
    eng.ref_set_trajectory(tr["coeff_x"], tr["coeff_y"], tr["coeff_z"], tr["coeff_yaw"], tr["time_cum"], tr["time_seg"], tr["final_pt"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=250)
    ap.add_argument("--skip", type=int, default=50)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd.params import nmpc_params as CP
    dev = torch.device("cuda:0")
    B, K = 2 * a.pairs, a.ticks
    n_seg = int(np.ceil((K * CP.ts_nmpc + 2.5) / 0.5))
    rows = []
    for dz in (0.5, 1.0, -0.5):
        tr, idx = stacked_pairs(a.pairs, dz, n_seg=n_seg)
        low, up = (slice(0, B, 2), slice(1, B, 2)) if dz > 0 else (slice(1, B, 2), slice(0, B, 2))
        engs = {"nmpc": ndp.BatchedNMPC(B, load_mlp=True), "ndp": ndp.BatchedNMPC(B, disturbance=True)}
        for e in engs.values():
            set_trajectory(e, tr)
        ref = np.stack([engs["nmpc"].ref_window(np.full(B, (k + 1) * CP.ts_nmpc))[0][:, 0, 0:3] for k in range(K)])
        x0 = engs["nmpc"].ref_window(np.zeros(B))[0][:, 0].copy()
        idx_t = torch.from_numpy(idx).to(dev)
        for scale in (1.0, 0.7, 1.3):
            for name, eng in engs.items():
                x = torch.from_numpy(x0).to(dev)
                log = torch.empty(K, B, 10, dtype=torch.float64, device=dev)
                log_f = torch.empty(K, B, 3, dtype=torch.float64, device=dev)
                worst = torch.zeros(B, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                eng.rollout_formation_device(K, x, idx_t, log=log, log_f=log_f, worst_status=worst, plant_scale=scale)
                eng.synchronize()
                ez = log.cpu().numpy()[a.skip:, :, 2] - ref[a.skip:, :, 2]
                rm = np.sqrt(np.mean(ez * ez, axis=0))
                rows.append({"dz": dz, "plant_scale": scale, "controller": name,
                             "z_rmse_lower_m": {"mean": float(rm[low].mean()), "max": float(rm[low].max())},
                             "z_rmse_upper_m": {"mean": float(rm[up].mean()), "max": float(rm[up].max())},
                             "peak_force_N": float(log_f.abs().max()), "worst_status": int(worst.max())})
    print(json.dumps({"experiment": "closed-loop formation rollout, downwash on the plant", "pairs": a.pairs, "ticks": K,
                      "rmse_over_ticks": [a.skip, K - 1], "dt_tick": CP.ts_nmpc, "substeps": 4, "rows": rows}))


if __name__ == "__main__":
    main()
