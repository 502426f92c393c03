"""The closed-loop formation experiment (SURVEY 8 row f4 with the downwash acting on the plant) on the CPU, from the oracle's pieces:
ref_window -> the true force at the actual relative state -> step_batch (blind, or with downwash_batch's prediction) -> plant_step.
tests/test_formation_rollout.py holds it to the paper's effect; tests/test_formation_rollout_gpu.py holds the device rollout to it.

The workload: `pairs` pairs on figure-eights (omega in [0.5, 1] rad/s), vehicle 2k + 1 flies vehicle 2k's path dz above it
(other_index = i ^ 1), so the pairs stay stacked -- horizontal distance << r_horiz -- and no gate flips.  The trajectories are the
TrajCoefficients arrays ndp_ref_set_trajectory takes, the z offset added to the neighbour's constant coefficient and final_pt."""
import functools
import os

import numpy as np

from ndp_nmpc_qd_amd import synth
from ndp_nmpc_qd_amd.params import downwash_params as DP
from ndp_nmpc_qd_amd.params import nmpc_params as CP
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS, TICKS, SKIP = 4, 200, 50          # the acceptance workload: z-RMSE over ticks SKIP..TICKS-1
N_SEG, T_SEG = 16, 0.5                   # 8 s of trajectory: TICKS * ts_nmpc + the 2 s horizon fit


def workload(pairs=PAIRS, dz=0.5, seed=7):
    """dict: the trajectory arrays (coeff_x .. final_pt), other_index int32[B], B = 2 pairs."""
    B = 2 * pairs
    tr = synth.figure_eight_traj(B, seed=seed, n_seg=N_SEG, t_seg=T_SEG, omega_range=(0.5, 1.0))
    for k in ("coeff_x", "coeff_y", "coeff_z", "coeff_yaw", "time_cum", "time_seg", "final_pt"):
        tr[k][1::2] = tr[k][0::2]
    tr["coeff_z"][1::2, 0::8] += dz
    tr["final_pt"][1::2, 2] += dz
    tr["other_index"] = (np.arange(B, dtype=np.int32) ^ 1).astype(np.int32)
    return tr


def set_trajectory(eng, tr):
    eng.ref_set_trajectory(tr["coeff_x"], tr["coeff_y"], tr["coeff_z"], tr["coeff_yaw"], tr["time_cum"], tr["time_seg"], tr["final_pt"])


def _model(cfg):
    """cfg (an OrcCfg or None: the oracle's default) with the force off, a copy."""
    c = O.default_cfg() if cfg is None else type(cfg).from_buffer_copy(cfg)
    c.use_fd = 0
    return c


def windows(tr, ticks, t0=0.0, dt=CP.ts_nmpc, cfg=None):
    """The oracle's reference windows at t0 + k dt, k = 0 .. ticks (one more than the ticks: node 0 of window k + 1 is where the vehicle
    should be after tick k): xr [ticks+1, B, N+1, 10], ur [ticks+1, B, N, 4].  cfg: the model (the flatness map reads mass and g)."""
    B = tr["coeff_x"].shape[0]
    c = _model(cfg)
    coeff = np.concatenate([tr["coeff_" + a].reshape(B, N_SEG, -1) for a in ("x", "y", "z", "yaw")], axis=2)
    out = [O.ref_window(coeff, tr["time_cum"], tr["time_seg"], tr["final_pt"], np.full(B, t0 + k * dt), N=c.N, dt=c.dt, mass=c.mass, g=c.g)
           for k in range(ticks + 1)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def true_force(blob, x, idx, gate=True, scale=1.0, r_horiz=DP.r_horiz):
    """The force on the plant: the network at the actual relative state (fp64 difference rounded to fp32), strict gate on the actual xy
    at r_horiz.  idx < 0 or >= B: an empty slot (the device's rule)."""
    has = (idx >= 0) & (idx < len(idx))
    o = np.where(has, idx, np.arange(len(idx)))
    d = x[o] - x
    f = O.mlp_forward(blob, d[:, 0:6].astype(np.float32)).astype(np.float64) * scale
    open_ = has & ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < r_horiz ** 2) if gate else True)
    return np.where(open_[:, None], f, 0.0)


def cpu_rollout(blob, tr, xr_all, ur_all, compensate, ticks=TICKS, gate=True, scale=1.0, dt=CP.ts_nmpc, substeps=4, cfg=None,
                r_horiz=DP.r_horiz, x_init=None):
    """-> (states [ticks, B, 10], u0 [ticks, B, 4], force [ticks, B, 3], status [ticks, B]) from x = x_init (None: xr[0][:, 0]).  cfg: the model of
    controller and plant (None: the oracle's default), r_horiz: the radius of both gates."""
    idx = tr["other_index"]
    cfg = _model(cfg)
    cfg.use_fd = int(bool(compensate))
    X, U = xr_all[0].copy(), ur_all[0].copy()
    x = xr_all[0][:, 0].copy() if x_init is None else np.array(x_init, dtype=np.float64)
    log, log_u, log_f, log_s = [], [], [], []
    for k in range(ticks):
        xr, ur = xr_all[k], ur_all[k]
        f = true_force(blob, x, idx, gate, scale, r_horiz)
        fp = None
        if compensate:      # the reference's rule: the neighbour's window against the ego odometry (ndp_nmpc_leader_node.py:60-76)
            fp = O.downwash_batch(blob, xr[idx].copy(), xr, x[:, 0:2].copy() if gate else None, r_horiz=r_horiz)
        u0, st, _ = O.step_batch(cfg, x, xr, ur, fp, X, U)
        x = O.plant_step(cfg, x.copy(), u0, f, dt, substeps)
        log.append(x.copy()); log_u.append(u0); log_f.append(f); log_s.append(st)
    return np.stack(log), np.stack(log_u), np.stack(log_f), np.stack(log_s)


def z_rmse(states, xr_all, skip=SKIP):
    """Per vehicle: RMS of z - z_ref over ticks skip .. (state k against node 0 of window k + 1)."""
    e = states[skip:, :, 2] - xr_all[skip + 1:states.shape[0] + 1, :, 0, 2]
    return np.sqrt(np.mean(e * e, axis=0))


@functools.lru_cache(maxsize=None)
def reference(dz):
    """The acceptance workload at one dz, computed once per session: dict tr, xr, ur, and per controller ('nmpc', 'ndp') the rollout.
    (The oracle library must have been built: the tests' `oracle` fixture does.)"""
    blob = np.fromfile(os.path.join(ROOT, "ndp_nmpc_qd_amd", "weights", "downwash_sn4.bin"), dtype="<f4")
    tr = workload(PAIRS, dz)
    xr, ur = windows(tr, TICKS)
    return dict(tr=tr, xr=xr, ur=ur, nmpc=cpu_rollout(blob, tr, xr, ur, False), ndp=cpu_rollout(blob, tr, xr, ur, True))
