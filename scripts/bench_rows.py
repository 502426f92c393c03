#!/usr/bin/env python3
"""Measurement of the widened rows -- separate from bench.py, whose line is the headline metric.

    python scripts/bench_rows.py --row throttle --batch 4194304

throttle (f3): one KF + differentiator update + actuator command per vehicle and tick.  Elementwise, HBM-bound:
algorithmic bytes per vehicle = read vz 8 + throttle 8 + state 64, write state 64 + k 8 (152 B) for the estimator,
read u0 32 + k 8, write cmd 32 (72 B) for the actuator command.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events(torch, fn, steps, warmup):
    """fn(i) `steps` times behind `warmup` untimed calls; returns seconds per call by HIP events on the current stream."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / steps


def _trajectories(B, M=4, seed=7):
    import numpy as np
    from ndp_nmpc_qd_amd.pt_pub import TrajCoefficients
    rng = np.random.default_rng(seed)
    wp = np.zeros((B, 4, M + 1))
    wp[:, 0:2] = np.cumsum(rng.uniform(-1.0, 1.0, (B, 2, M + 1)), axis=2)
    wp[:, 2] = 1.0 + 0.2 * rng.uniform(-1, 1, (B, M + 1))
    wp[:, 3] = np.cumsum(rng.uniform(-0.3, 0.3, (B, M + 1)), axis=1)
    return TrajCoefficients.from_waypoints(wp, rng.uniform(3.0, 5.0, (B, M)))


def rows_block(torch, ndp, dev, B=1 << 18):
    """The widened rows in bench.py's line (`rows`): each on device buffers at batch B, ~0.2 s per row.  value = vehicles per second,
    frac = algorithmic bytes (the docstrings below) / kernel time / 8 TB/s."""
    import ctypes as C
    import numpy as np
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    out = {"batch": B}
    tc = _trajectories(B)
    eng = ndp.BatchedNMPC(B, load_mlp=False)
    eng.ref_set_trajectory(tc.coeff_x, tc.coeff_y, tc.coeff_z, tc.coeff_yaw, tc.traj_time_cum, tc.traj_time_seg, tc.final_pt)
    ts = [torch.full((B,), 0.02 * i, dtype=torch.float64, device=dev) for i in range(8)]
    xr = torch.empty(B, 21, 10, dtype=torch.float64, device=dev)
    ur = torch.empty(B, 20, 4, dtype=torch.float64, device=dev)
    dt = _events(torch, lambda i: eng.ref_window_device(ts[i % 8], xr, ur, stream=st), 30, 5)
    out["f1_window"] = {"value": B / dt, "frac": (8 + 224 + 72 + 1680 + 640) * B / dt / 8e12}
    eng.ref_list_reset()

    def list_tick(i):
        eng.ref_list_advance_device(ts[i % 8], stream=st)
        eng.ref_list_window_device(xr, ur, stream=st)
    dt = _events(torch, list_tick, 30, 5)
    out["f1_list"] = {"value": B / dt, "frac": ((8 + 224 + 72 + 2 * 112) + 2 * (1680 + 640)) * B / dt / 8e12}
    del eng, xr, ur
    B3 = 1 << 22                                          # (224 B per vehicle: a device-filling batch is a few million vehicles)
    e3 = ndp.BatchedNMPC(B3, N=2, load_mlp=False)         # tiny horizon: only the estimator state matters here
    vz = torch.randn(B3, dtype=torch.float64, device=dev) * 0.1
    th = torch.rand(B3, dtype=torch.float64, device=dev) * 0.8 + 0.15
    k = torch.empty(B3, dtype=torch.float64, device=dev)
    u0 = torch.randn(B3, 4, dtype=torch.float64, device=dev)
    cmd = torch.empty(B3, 4, dtype=torch.float64, device=dev)
    lib, h, s = e3._lib, e3._h, C.c_void_p(st.cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def f3(i):
        lib.ndp_throttle_update_device(h, p(vz), p(th), p(k), s)
        lib.ndp_actuator_cmd_device(h, p(u0), p(k), p(cmd), s)
    dt = _events(torch, f3, 50, 5)
    out["f3"] = {"value": B3 / dt, "frac": (152 + 72) * B3 / dt / 8e12, "batch": B3}
    del e3
    Br = 1024
    tcr = _trajectories(Br)
    er = ndp.BatchedNMPC(Br)
    er.ref_set_trajectory(tcr.coeff_x, tcr.coeff_y, tcr.coeff_z, tcr.coeff_yaw, tcr.traj_time_cum, tcr.traj_time_seg, tcr.final_pt)
    x = torch.from_numpy(er.ref_window(np.zeros(Br))[0][:, 0].copy()).to(dev)
    er.rollout_device(20, x)
    er.synchronize()
    t0 = time.perf_counter()
    er.rollout_device(200, x, t0=0.4)
    er.synchronize()
    el = time.perf_counter() - t0
    out["rollout"] = {"value": Br * 200 / el, "us_per_tick": el / 200 * 1e6, "batch": Br}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", default="throttle")
    ap.add_argument("--batch", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    B = a.batch
    dev = torch.device("cuda:0")
    if a.row == "ref_window":
        return bench_ref_window(a, torch, ndp, dev)
    if a.row == "rollout":
        return bench_rollout(a, torch, ndp, dev)
    if a.row == "rollout_formation":
        return bench_rollout_formation(a, torch, ndp, dev)
    if a.row == "ref_list":
        return bench_ref_list(a, torch, ndp, dev)
    if a.row == "downwash_multi":
        return bench_downwash_multi(a, torch, ndp, dev)
    if a.row == "downwash_multi_vjp":
        return bench_downwash_multi_vjp(a, torch, ndp, dev)
    if a.row == "rollout_formation_multi":
        return bench_rollout_formation_multi(a, torch, ndp, dev)
    eng =ndp.BatchedNMPC(B, N=2, load_mlp=False)       # tiny horizon: only the estimator state matters here
    vz = torch.randn(B, dtype=torch.float64, device=dev) * 0.1
    th = torch.rand(B, dtype=torch.float64, device=dev) * 0.8 + 0.15
    k = torch.empty(B, dtype=torch.float64, device=dev)
    u0 = torch.randn(B, 4, dtype=torch.float64, device=dev)
    cmd = torch.empty(B, 4, dtype=torch.float64, device=dev)
    import ctypes as C
    lib, h = eng._lib, eng._h
    st = torch.cuda.Stream(device=dev)       # non-default: handle 0 would mean "the library's own stream"
    torch.cuda.set_stream(st)
    s = C.c_void_p(st.cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def step():
        assert lib.ndp_throttle_update_device(h, p(vz), p(th), p(k), s) == 0
        assert lib.ndp_actuator_cmd_device(h, p(u0), p(k), p(cmd), s) == 0

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    dev_s = e0.elapsed_time(e1) * 1e-3 / a.steps
    bytes_per = 152 + 72
    print(json.dumps({"row": "f3 hover-throttle estimator + actuator command", "metric": "vehicle updates/s",
                      "value": B * a.steps / el, "batch": B, "ms_per_step": el / a.steps * 1e3, "dtype": "f64",
                      "roofline": {"bound": "hbm", "achieved": bytes_per * B / dev_s / 1e9, "peak": 8000.0, "unit": "GB/s",
                                   "frac": bytes_per * B / dev_s / 1e9 / 8000.0, "algorithmic_bytes_per_vehicle": bytes_per}}))


def bench_ref_window(a, torch, ndp, dev):
    """f1: reference windows of B vehicles per tick (4-segment minimum-snap trajectories, N = 20).  Algorithmic bytes
    per vehicle: read t 8 + the coefficients of the segments the window touches (one or two: 224..448, counted as 224)
    + 5 time_cum + 4 time_seg doubles 72, write xr 1680 + ur 640 = 2624 B."""
    import numpy as np
    from ndp_nmpc_qd_amd.pt_pub import TrajCoefficients
    B, M = a.batch, 4
    rng = np.random.default_rng(7)
    wp = np.zeros((B, 4, M + 1))
    wp[:, 0:2] = np.cumsum(rng.uniform(-1.0, 1.0, (B, 2, M + 1)), axis=2)
    wp[:, 2] = 1.0 + 0.2 * rng.uniform(-1, 1, (B, M + 1))
    wp[:, 3] = np.cumsum(rng.uniform(-0.3, 0.3, (B, M + 1)), axis=1)
    tc = TrajCoefficients.from_waypoints(wp, rng.uniform(3.0, 5.0, (B, M)))
    eng = ndp.BatchedNMPC(B, load_mlp=False)
    eng.ref_set_trajectory(tc.coeff_x, tc.coeff_y, tc.coeff_z, tc.coeff_yaw, tc.traj_time_cum, tc.traj_time_seg, tc.final_pt)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ts = [torch.full((B,), 0.02 * i, dtype=torch.float64, device=dev) for i in range(8)]
    xr = torch.empty(B, 21, 10, dtype=torch.float64, device=dev)
    ur = torch.empty(B, 20, 4, dtype=torch.float64, device=dev)
    for i in range(a.warmup):
        eng.ref_window_device(ts[i % 8], xr, ur, stream=st)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(a.steps):
        eng.ref_window_device(ts[i % 8], xr, ur, stream=st)
    e1.record()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    dev_s = e0.elapsed_time(e1) * 1e-3 / a.steps
    bytes_per = 8 + 224 + 72 + 1680 + 640
    print(json.dumps({"row": "f1 reference window generation (polynomial trajectory + differential flatness)",
                      "metric": "vehicle windows/s", "value": B * a.steps / el, "batch": B, "ms_per_step": el / a.steps * 1e3,
                      "dtype": "f64", "kernel_us": dev_s * 1e6,
                      "roofline": {"bound": "hbm", "achieved": bytes_per * B / dev_s / 1e9, "peak": 8000.0, "unit": "GB/s",
                                   "frac": bytes_per * B / dev_s / 1e9 / 8000.0, "algorithmic_bytes_per_vehicle": bytes_per}}))


def bench_ref_list(a, torch, ndp, dev):
    """f1, the reference's own bookkeeping (NMPCRefPublisher's sliding list, pt_pub/pt_publisher.py:36-103) on the device: per
    tick ONE new reference point per vehicle into the phase-major list (ref_list_fill_kernel: every entry is stored twice so that
    every window is contiguous) and the window as a dense copy (ref_list_window_kernel).  Algorithmic bytes per vehicle and tick:
    advance = read t 8 + coefficients 224 + 72, write one entry twice 224; window = read 1680 + 640, write xr 1680 + ur 640."""
    import numpy as np
    from ndp_nmpc_qd_amd.pt_pub import TrajCoefficients
    B, M = a.batch, 4
    rng = np.random.default_rng(7)
    wp = np.zeros((B, 4, M + 1))
    wp[:, 0:2] = np.cumsum(rng.uniform(-1.0, 1.0, (B, 2, M + 1)), axis=2)
    wp[:, 2] = 1.0 + 0.2 * rng.uniform(-1, 1, (B, M + 1))
    wp[:, 3] = np.cumsum(rng.uniform(-0.3, 0.3, (B, M + 1)), axis=1)
    tc = TrajCoefficients.from_waypoints(wp, rng.uniform(3.0, 5.0, (B, M)))
    eng = ndp.BatchedNMPC(B, load_mlp=False)
    eng.ref_set_trajectory(tc.coeff_x, tc.coeff_y, tc.coeff_z, tc.coeff_yaw, tc.traj_time_cum, tc.traj_time_seg, tc.final_pt)
    eng.ref_list_reset()
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ts = [torch.full((B,), 0.02 * i, dtype=torch.float64, device=dev) for i in range(8)]
    xr = torch.empty(B, 21, 10, dtype=torch.float64, device=dev)
    ur = torch.empty(B, 20, 4, dtype=torch.float64, device=dev)

    def tick(i):
        eng.ref_list_advance_device(ts[i % 8], stream=st)
        eng.ref_list_window_device(xr, ur, stream=st)
    for i in range(a.warmup):
        tick(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(a.steps):
        tick(i)
    e1.record()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    dev_s = e0.elapsed_time(e1) * 1e-3 / a.steps
    bytes_per = (8 + 224 + 72 + 2 * 112) + 2 * (1680 + 640)      # advance: t + one segment record + one entry stored twice; window: a dense copy
    print(json.dumps({"row": "f1 reference list on the device: one new point per vehicle and tick + window = every 5th entry",
                      "metric": "vehicle windows/s", "value": B * a.steps / el, "batch": B, "ms_per_step": el / a.steps * 1e3,
                      "dtype": "f64", "kernels_us": dev_s * 1e6,
                      "roofline": {"bound": "hbm", "achieved": bytes_per * B / dev_s / 1e9, "peak": 8000.0, "unit": "GB/s",
                                   "frac": bytes_per * B / dev_s / 1e9 / 8000.0, "algorithmic_bytes_per_vehicle": bytes_per}}))


def bench_rollout(a, torch, ndp, dev):
    """f4 + f1 + the control step: closed-loop rollout of B vehicles on their minimum-snap trajectories, a.steps ticks in
    one ndp_rollout_device call (3 launches per tick: reference window, control step, plant step)."""
    import numpy as np
    from ndp_nmpc_qd_amd.pt_pub import TrajCoefficients
    B, M = a.batch, 4
    rng = np.random.default_rng(7)
    wp = np.zeros((B, 4, M + 1))
    wp[:, 0:2] = np.cumsum(rng.uniform(-1.0, 1.0, (B, 2, M + 1)), axis=2)
    wp[:, 2] = 1.0 + 0.2 * rng.uniform(-1, 1, (B, M + 1))
    wp[:, 3] = np.cumsum(rng.uniform(-0.3, 0.3, (B, M + 1)), axis=1)
    tc = TrajCoefficients.from_waypoints(wp, rng.uniform(3.0, 5.0, (B, M)))
    eng = ndp.BatchedNMPC(B)
    eng.ref_set_trajectory(tc.coeff_x, tc.coeff_y, tc.coeff_z, tc.coeff_yaw, tc.traj_time_cum, tc.traj_time_seg, tc.final_pt)
    xr0, _ = eng.ref_window(np.zeros(B))
    x = torch.from_numpy(xr0[:, 0].copy()).to(dev)
    eng.rollout_device(a.warmup, x)
    eng.synchronize()
    t0 = time.perf_counter()
    eng.rollout_device(a.steps, x, t0=a.warmup * 0.02)
    eng.synchronize()
    el = time.perf_counter() - t0
    xr_end, _ = eng.ref_window(np.full(B, (a.warmup + a.steps) * 0.02))
    err = np.linalg.norm(x.cpu().numpy()[:, 0:3] - xr_end[:, 0, 0:3], axis=1)
    print(json.dumps({"row": "closed-loop rollout: reference window + control step (N=20, 1 RTI) + plant step per tick",
                      "metric": "vehicle ticks/s", "value": B * a.steps / el, "batch": B, "ticks": a.steps,
                      "us_per_tick": el / a.steps * 1e6, "simulated_seconds_per_vehicle": a.steps * 0.02,
                      "tracking_error_at_end_m": {"median": float(np.median(err)), "max": float(err.max())}}))


def bench_rollout_formation(a, torch, ndp, dev):
    """The rollout row with the downwash acting on the plant: B vehicles in stacked pairs (scripts/formation_rollout.py: the neighbour
    0.5 m above), a.steps ticks in one ndp_rollout_formation_device call per controller -- NDP (the fused step predicts the force) and
    NMPC (blind).  4 launches per tick: reference window, plant force, control step, plant step."""
    import numpy as np
    from formation_rollout import set_trajectory, stacked_pairs
    B = a.batch - a.batch % 2
    tr, idx = stacked_pairs(B // 2, 0.5, n_seg=int(np.ceil(((a.warmup + a.steps) * 0.02 + 2.5) / 0.5)))
    idx_t = torch.from_numpy(idx).to(dev)
    res = {}
    for name, dist in (("ndp", True), ("nmpc", False)):
        eng = ndp.BatchedNMPC(B, disturbance=dist, load_mlp=True)
        set_trajectory(eng, tr)
        x = torch.from_numpy(eng.ref_window(np.zeros(B))[0][:, 0].copy()).to(dev)
        worst = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        eng.rollout_formation_device(a.warmup, x, idx_t)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.rollout_formation_device(a.steps, x, idx_t, worst_status=worst, t0=a.warmup * 0.02)
        eng.synchronize()
        el = time.perf_counter() - t0
        xr_end, _ = eng.ref_window(np.full(B, (a.warmup + a.steps) * 0.02))
        ez = np.abs(x.cpu().numpy()[:, 2] - xr_end[:, 0, 2])
        res[name] = {"value": B * a.steps / el, "us_per_tick": el / a.steps * 1e6, "worst_status": int(worst.max()),
                     "z_error_at_end_m": {"lower_max": float(ez[0::2].max()), "upper_max": float(ez[1::2].max())}}
    print(json.dumps({"row": "closed-loop formation rollout: reference window + plant force (downwash network, one row per vehicle) + "
                             "control step (N=20, 1 RTI) + plant step per tick, stacked pairs dz = 0.5 m",
                      "metric": "vehicle ticks/s", "batch": B, "ticks": a.steps, "controllers": res}))


def bench_downwash_multi(a, torch, ndp, dev):
    """The controller's prediction from K neighbours (B = a.batch instances, N = 20), K = 2 and 3: ONE ndp_downwash_multi_device launch
    (the weights parked in LDS once per workgroup, reused by the K slots) against what the single-neighbour library needs for the same
    sum -- K launches of ndp_downwash_device on pre-gathered windows plus torch adds -- in the same run, alternating, by device events."""
    import numpy as np
    B, N = a.batch, 20
    rng = np.random.default_rng(7)
    eng = ndp.BatchedNMPC(B, N=N, load_mlp=True)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ego = np.zeros((B, N + 1, 10))
    ego[:, :, 0:2] = rng.uniform(-0.4, 0.4, (B, 1, 2))
    ego[:, :, 2] = 1.0
    ego[:, :, 3:6] = rng.normal(0, 0.3, (B, N + 1, 3))
    other = ego.copy()
    other[:, :, 2] += rng.uniform(0.4, 0.9, (B, 1))
    ego_t, other_t = torch.from_numpy(ego).to(dev), torch.from_numpy(other).to(dev)
    xy_t = ego_t[:, 0, 0:2].contiguous()
    out = {}
    for K in (2, 3):
        idx = np.stack([rng.permutation(B) for _ in range(K)], axis=1).astype(np.int32)
        idx_t = torch.from_numpy(idx).to(dev)
        gathered = [other_t[torch.from_numpy(idx[:, k].astype(np.int64)).to(dev)].contiguous() for k in range(K)]
        f_multi = torch.empty(B, N + 1, 3, dtype=torch.float32, device=dev)
        f_k = [torch.empty_like(f_multi) for _ in range(K)]
        f_sum = torch.empty_like(f_multi)

        def multi(i):
            eng.downwash_multi_device(other_t, idx_t, ego_t, f_multi, ego_xy=xy_t, stream=st)

        def single(i):
            for k in range(K):
                eng.downwash_device(gathered[k], ego_t, f_k[k], ego_xy=xy_t, stream=st)
            torch.add(f_k[0], f_k[1], out=f_sum)
            for k in range(2, K):
                f_sum.add_(f_k[k])
        tm, ts = [], []
        for _ in range(3):                                # alternating: other people's work shares the machine
            tm.append(_events(torch, multi, a.steps, a.warmup))
            ts.append(_events(torch, single, a.steps, a.warmup))
        assert torch.equal(f_multi, f_sum)
        out[f"K{K}"] = {"one_launch_us": min(tm) * 1e6, "k_launches_plus_add_us": min(ts) * 1e6, "speedup": min(ts) / min(tm),
                        "one_launch_us_runs": [t * 1e6 for t in tm], "k_launches_plus_add_us_runs": [t * 1e6 for t in ts]}
    print(json.dumps({"row": "downwash prediction from K neighbours: one mlp_multi_kernel launch against K mlp_kernel launches + add",
                      "metric": "us per call (device events, launches included)", "batch": B, "N": N, "results": out}))


def bench_downwash_multi_vjp(a, torch, ndp, dev):
    """The derivatives of the K-neighbour prediction (B = a.batch instances, N = 20), K = 2 and 3, every gate open and about a third of the
    slots open.  Reverse mode, gz and gw both asked for: ONE ndp_downwash_multi_vjp_device call against what it replaces on the same
    inputs -- K ndp_downwash_vjp_device calls into K buffers plus the K - 1 adds of gw.  Forward mode, T = 1 and 4: one
    ndp_downwash_multi_jvp_device call against K ndp_downwash_jvp_device calls plus the K - 1 adds of df.  Alternating passes in one
    run, by device events; the figure of a pass is its mean over a.steps calls, the figure reported is the median of the passes."""
    import numpy as np
    B, N, P = a.batch, 20, 17859
    rng = np.random.default_rng(7)
    eng = ndp.BatchedNMPC(B, N=N, load_mlp=True)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    T = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x)).to(dev) if dt is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
    ego = rng.normal(0.0, 1.0, (B, N + 1, 10))
    gf_t = T(rng.normal(size=(B, N + 1, 3)))
    out = {}
    for K in (2, 3):
        z = np.empty((B, K, N + 1, 6))
        z[..., :3], z[..., 3:] = rng.uniform(-1.5, 1.5, (B, K, N + 1, 3)), rng.uniform(-3.0, 3.0, (B, K, N + 1, 3))
        for mix in ("all_open", "third_open"):
            # every slot a row of `other` of its own; node 0's xy of slot (i, k) sits rad away from ego_xy[i]
            want = np.ones((B, K), dtype=bool) if mix == "all_open" else rng.random((B, K)) < 1.0 / 3.0
            rad = np.where(want, rng.uniform(0.0, 0.9, (B, K)), rng.uniform(1.1, 3.0, (B, K)))
            ang = rng.uniform(0.0, 2.0 * np.pi, (B, K))
            zz = z.copy()
            zz[:, :, 0, 0], zz[:, :, 0, 1] = rad * np.cos(ang), rad * np.sin(ang)
            other = rng.normal(0.0, 1.0, (B * K, N + 1, 10))
            other[:, :, :6] = (ego[:, None, :, :6] + zz).reshape(B * K, N + 1, 6)
            idx = np.arange(B * K, dtype=np.int32).reshape(B, K)
            other_t, ego_t, xy_t, idx_t = T(other), T(ego), T(ego[:, 0, 0:2]), T(idx)
            idx_k = [T(idx[:, k]) for k in range(K)]
            gz_m = torch.empty(B, K, N + 1, 6, dtype=torch.float64, device=dev)
            gw_m = torch.empty(P, dtype=torch.float32, device=dev)
            gz_k = [torch.empty(B, N + 1, 6, dtype=torch.float64, device=dev) for _ in range(K)]
            gw_k = [torch.empty(P, dtype=torch.float32, device=dev) for _ in range(K)]
            gw_s = torch.empty(P, dtype=torch.float32, device=dev)

            def vjp_multi(i):
                eng.downwash_multi_vjp_device(other_t, idx_t, ego_t, gf_t, ego_xy=xy_t, gz=gz_m, gw=gw_m, stream=st)

            def vjp_single(i):
                for k in range(K):
                    eng.downwash_vjp_device(other_t, ego_t, gf_t, ego_xy=xy_t, other_index=idx_k[k], gz=gz_k[k], gw=gw_k[k], stream=st)
                torch.add(gw_k[0], gw_k[1], out=gw_s)
                for k in range(2, K):
                    gw_s.add_(gw_k[k])
            res = {"slots_open": float(want.mean())}
            tm, ts = [], []
            for _ in range(5):                            # alternating: other people's work shares the machine
                tm.append(_events(torch, vjp_multi, a.steps, a.warmup))
                ts.append(_events(torch, vjp_single, a.steps, a.warmup))
            assert all(torch.equal(gz_m[:, k], gz_k[k]) for k in range(K))
            scale = float(gw_s.abs().max())
            assert float((gw_m - gw_s).abs().max()) <= 1e-4 * max(1.0, scale)
            res["vjp"] = {"one_call_us": float(np.median(tm)) * 1e6, "k_calls_plus_adds_us": float(np.median(ts)) * 1e6,
                          "ratio_k_calls_over_one": float(np.median(ts) / np.median(tm)),
                          "one_call_us_passes": [t * 1e6 for t in tm], "k_calls_plus_adds_us_passes": [t * 1e6 for t in ts]}
            for nt in (1, 4):
                tz_t = T(rng.normal(size=(B, nt, K, N + 1, 6)))
                tz_k = [tz_t[:, :, k].contiguous() for k in range(K)]
                tw_t = T(0.01 * rng.normal(size=(nt, P)), torch.float32)
                df_m = torch.empty(B, nt, N + 1, 3, dtype=torch.float64, device=dev)
                df_k = [torch.empty_like(df_m) for _ in range(K)]
                df_s = torch.empty_like(df_m)

                def jvp_multi(i):
                    eng.downwash_multi_jvp_device(other_t, idx_t, ego_t, tz=tz_t, tw=tw_t, ego_xy=xy_t, n_tan=nt, df=df_m, stream=st)

                def jvp_single(i):
                    for k in range(K):
                        eng.downwash_jvp_device(other_t, ego_t, tz=tz_k[k], tw=tw_t, ego_xy=xy_t, other_index=idx_k[k], n_tan=nt, df=df_k[k],
                                                stream=st)
                    torch.add(df_k[0], df_k[1], out=df_s)
                    for k in range(2, K):
                        df_s.add_(df_k[k])
                tm, ts = [], []
                for _ in range(5):
                    tm.append(_events(torch, jvp_multi, a.steps, a.warmup))
                    ts.append(_events(torch, jvp_single, a.steps, a.warmup))
                assert torch.equal(df_m, df_s)
                res[f"jvp_T{nt}"] = {"one_call_us": float(np.median(tm)) * 1e6, "k_calls_plus_adds_us": float(np.median(ts)) * 1e6,
                                     "ratio_k_calls_over_one": float(np.median(ts) / np.median(tm)),
                                     "one_call_us_passes": [t * 1e6 for t in tm], "k_calls_plus_adds_us_passes": [t * 1e6 for t in ts]}
            out[f"K{K}_{mix}"] = res
    print(json.dumps({"row": "derivatives of the downwash prediction from K neighbours: one mlp_vjp_multi_kernel / mlp_jvp_multi_kernel "
                             "call against K single-neighbour calls + adds", "metric": "us per call (device events, launches included; "
                             "median of 5 alternating passes)", "batch": B, "N": N, "results": out}))


def bench_rollout_formation_multi(a, torch, ndp, dev):
    """The formation rollout row with two neighbours per vehicle: B vehicles in stacked triples (scripts/formation_rollout.py --triples,
    dz = 0.5 m), a.steps ticks in one ndp_rollout_formation_multi_device call per controller.  Compensating: 5 launches per tick
    (reference window, plant force, prediction, control step, plant step); blind: 4."""
    import numpy as np
    from formation_rollout import set_trajectory, stacked_triples
    B = a.batch - a.batch % 3
    tr, idx = stacked_triples(B // 3, 0.5, n_seg=int(np.ceil(((a.warmup + a.steps) * 0.02 + 2.5) / 0.5)))
    idx_t = torch.from_numpy(idx).to(dev)
    res = {}
    for name, dist in (("ndp_all_slots", True), ("nmpc_blind", False)):
        eng = ndp.BatchedNMPC(B, disturbance=dist, load_mlp=True)
        set_trajectory(eng, tr)
        x = torch.from_numpy(eng.ref_window(np.zeros(B))[0][:, 0].copy()).to(dev)
        worst = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        eng.rollout_formation_multi_device(a.warmup, x, idx_t)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.rollout_formation_multi_device(a.steps, x, idx_t, worst_status=worst, t0=a.warmup * 0.02)
        eng.synchronize()
        el = time.perf_counter() - t0
        xr_end, _ = eng.ref_window(np.full(B, (a.warmup + a.steps) * 0.02))
        ez = np.abs(x.cpu().numpy()[:, 2] - xr_end[:, 0, 2])
        res[name] = {"value": B * a.steps / el, "us_per_tick": el / a.steps * 1e6, "worst_status": int(worst.max()),
                     "z_error_at_end_m": {"lowest_max": float(ez[0::3].max()), "top_max": float(ez[2::3].max())}}
    print(json.dumps({"row": "closed-loop formation rollout, two neighbours per vehicle: reference window + summed plant force + "
                             "[summed prediction +] control step (N=20, 1 RTI) + plant step per tick, stacked triples dz = 0.5 m",
                      "metric": "vehicle ticks/s", "batch": B, "ticks": a.steps, "controllers": res}))


if __name__ == "__main__":
    main()
