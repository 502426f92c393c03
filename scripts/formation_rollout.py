#!/usr/bin/env python3
"""The closed-loop formation experiment on the device (formation form): pairs of vehicles on figure-eights, the
neighbour flying the same path dz above (dz < 0: below) the ego vehicle, the shipped downwash network acting on the plant at the
vehicles' actual relative state.  Both controllers -- NMPC (blind) and NDP (predicts the force from the neighbour's reference window) --
for dz in {0.5, 1.0, -0.5} and plant_scale in {1.0, 0.7, 1.3} (the model-mismatch knob), one ndp_rollout_formation_device call each.

    python scripts/formation_rollout.py [--pairs 8] [--ticks 250] [--skip 50]
    python scripts/formation_rollout.py --triples 2 [--ticks 200] [--skip 50]

--triples: stacked TRIPLES instead (three vehicles on one figure-eight, dz apart, every vehicle hears the two others, forces superposed --
a modelling assumption: the network was trained on pairs), dz in {0.5, 0.75}, three legs: blind, the controller hearing slot 0 only (all a
single-neighbour entry point can do; the plant still feels both -- composed tick by tick from the host), hearing all slots
(ndp_rollout_formation_multi_device).  Per (dz, leg) the z-RMSE of the lowest, middle and top vehicle of the triples.

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


def stacked_triples(triples, dz, seed=7, n_seg=16, t_seg=0.5):
    """(trajectory dict, other_index int32[3 triples, 2]): vehicle 3t + m flies vehicle 3t's figure-eight m * dz above it; slot 0 = the
    next one up of the triple, cyclically, slot 1 the remaining one."""
    from ndp_nmpc_qd_amd import synth
    B = 3 * triples
    tr = synth.figure_eight_traj(B, seed=seed, n_seg=n_seg, t_seg=t_seg, omega_range=(0.5, 1.0))
    for m in (1, 2):
        for k in ("coeff_x", "coeff_y", "coeff_z", "coeff_yaw", "time_cum", "time_seg", "final_pt"):
            tr[k][m::3] = tr[k][0::3]
        tr["coeff_z"][m::3, 0::8] += m * dz
        tr["final_pt"][m::3, 2] += m * dz
    v = np.arange(B)
    return tr, np.stack([v // 3 * 3 + (v % 3 + 1) % 3, v // 3 * 3 + (v % 3 + 2) % 3], axis=1).astype(np.int32)


def slot0_leg(eng, idx, x0, K, dt):
    """The plant feels every slot, the controller hears slot 0: plant_force_multi -> downwash_multi_device (one slot) + update_device(f)
    -> plant_step, tick by tick from the host.  -> (states [K, B, 10], peak |force|, worst status)."""
    import torch
    B, N, dev = eng.B, eng.N, torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    u0_t, f_t = torch.empty(B, 4, dtype=torch.float64, device=dev), torch.empty(B, N + 1, 3, dtype=torch.float32, device=dev)
    p_t = t(idx[:, :1])
    eng.reset(*eng.ref_window(np.zeros(B)))
    xs, log, peak, worst = x0.copy(), [], 0.0, 0
    for k in range(K):
        xr, ur = eng.ref_window(np.full(B, k * dt))
        f = eng.plant_force_multi(xs, idx)
        xrt = t(xr)
        torch.cuda.synchronize()
        eng.downwash_multi_device(xrt, p_t, xrt, f_t, ego_xy=t(xs[:, 0:2]))
        eng.update_device(t(xs), xrt, t(ur), u0_t, f=f_t)
        eng.synchronize()
        worst = max(worst, int(eng.status()[0].max()))
        xs = eng.plant_step(xs, u0_t.cpu().numpy(), f, dt, 4)
        log.append(xs.copy())
        peak = max(peak, float(np.abs(f).max()))
    return np.stack(log), peak, worst


def main_triples(a):
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd.params import nmpc_params as CP
    dev = torch.device("cuda:0")
    B, K = 3 * a.triples, a.ticks
    n_seg = int(np.ceil((K * CP.ts_nmpc + 2.5) / 0.5))
    rows = []
    for dz in (0.5, 0.75):
        tr, idx = stacked_triples(a.triples, dz, n_seg=n_seg)
        idx_t = torch.from_numpy(idx).to(dev)
        engs = {"blind": ndp.BatchedNMPC(B, load_mlp=True), "slot0": ndp.BatchedNMPC(B, disturbance=True), "all": ndp.BatchedNMPC(B, disturbance=True)}
        for e in engs.values():
            set_trajectory(e, tr)
        ref = np.stack([engs["blind"].ref_window(np.full(B, (k + 1) * CP.ts_nmpc))[0][:, 0, 0:3] for k in range(K)])
        x0 = engs["blind"].ref_window(np.zeros(B))[0][:, 0].copy()
        for leg, eng in engs.items():
            if leg == "slot0":
                states, peak, worst = slot0_leg(eng, idx, x0, K, CP.ts_nmpc)
            else:
                x = torch.from_numpy(x0).to(dev)
                log = torch.empty(K, B, 10, dtype=torch.float64, device=dev)
                log_f = torch.empty(K, B, 3, dtype=torch.float64, device=dev)
                ws = torch.zeros(B, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                eng.rollout_formation_multi_device(K, x, idx_t, log=log, log_f=log_f, worst_status=ws)
                eng.synchronize()
                states, peak, worst = log.cpu().numpy(), float(log_f.abs().max()), int(ws.max())
            ez = states[a.skip:, :, 2] - ref[a.skip:, :, 2]
            rm = np.sqrt(np.mean(ez * ez, axis=0))
            d = states[:, idx, 0:2] - states[:, :, None, 0:2]
            rows.append({"dz": dz, "leg": leg, "z_rmse_m": {n: [float(v) for v in rm[m::3]] for m, n in enumerate(("lowest", "middle", "top"))},
                         "peak_force_N": peak, "worst_status": worst, "max_slot_distance_m": float(np.sqrt((d * d).sum(-1)).max())})
    print(json.dumps({"experiment": "closed-loop formation rollout on stacked triples, two neighbours per vehicle, forces superposed",
                      "triples": a.triples, "ticks": K, "rmse_over_ticks": [a.skip, K - 1], "dt_tick": CP.ts_nmpc, "substeps": 4, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triples", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=250)
    ap.add_argument("--skip", type=int, default=50)
    a = ap.parse_args()
    if a.triples:
        return main_triples(a)
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
