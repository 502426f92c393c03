#!/usr/bin/env python3
"""Time of the plant over an input sequence on one device, as one JSON line: B vehicles, `ticks` ticks, `substeps` RK4 substeps, with a
force, every form producing (or differentiating) the same log xs [ticks,B,10]:

  per_tick_us   the route there was before: ticks x (ndp_plant_step_device + a device-to-device copy of the state into the log),
                enqueued from the host on one stream (the calls bound once: one ctypes call and one torch copy per tick);
  rollout_us    ndp_plant_rollout_device, one launch;
  vjp_us        ndp_plant_rollout_vjp_device (gx0, gu and gf) on that log;
  jvp1_us / jvp8_us   ndp_plant_rollout_jvp_device with T = 1 / T = 8 directions of x0, u and f;
  torch_us      for orientation: forward + backward of torch autograd through a torch-op transcription of the plant (fewer passes).

    python scripts/bench_plant_rollout.py [--batch 1024 16384] [--ticks 100] [--substeps 4] [--passes 20] [--warmup 3] [--repeats 5]

Each figure is a host clock around `passes` calls on a side stream that ends in a stream synchronise, after `warmup` calls of the same
kind; the forms are timed alternately `repeats` times and the median is reported with the spread (scripts/bench_fit_rows.py's pattern).
There is no speed bar on these numbers; they go into DESIGN section 9 as measured."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_plant(x, u, f, dt, substeps, mass, gravity):
    """The plant in torch ops: x [B,10], u [ticks,B,4], f [ticks,B,3] -> xs [ticks,B,10] (what a user would write without the call)."""
    import torch

    def rhs(x, u, acc):
        qw, qx, qy, qz = x[:, 6], x[:, 7], x[:, 8], x[:, 9]
        return torch.stack([
            x[:, 3], x[:, 4], x[:, 5],
            2.0 * (qx * qz + qw * qy) * u[:, 3] + acc[:, 0],
            2.0 * (qy * qz - qw * qx) * u[:, 3] + acc[:, 1],
            (1.0 - 2.0 * qx * qx - 2.0 * qy * qy) * u[:, 3] + acc[:, 2],
            (-u[:, 0] * qx - u[:, 1] * qy - u[:, 2] * qz) * 0.5,
            (u[:, 0] * qw + u[:, 2] * qy - u[:, 1] * qz) * 0.5,
            (u[:, 1] * qw - u[:, 2] * qx + u[:, 0] * qz) * 0.5,
            (u[:, 2] * qw + u[:, 1] * qx - u[:, 0] * qy) * 0.5], dim=1)

    h, g3, out = dt / substeps, torch.tensor([0.0, 0.0, gravity], dtype=x.dtype, device=x.device), []
    for k in range(u.shape[0]):
        acc = f[k] / mass - g3
        for _ in range(substeps):
            k1 = rhs(x, u[k], acc)
            k2 = rhs(x + 0.5 * h * k1, u[k], acc)
            k3 = rhs(x + 0.5 * h * k2, u[k], acc)
            k4 = rhs(x + h * k3, u[k], acc)
            x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        x = torch.cat([x[:, :6], x[:, 6:] / x[:, 6:].norm(dim=1, keepdim=True)], dim=1)
        out.append(x)
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--substeps", type=int, default=4)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-passes", type=int, default=2)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd.params import nmpc_params as CP
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    K, sub, dt = a.ticks, a.substeps, CP.ts_nmpc
    out = {}
    for B in a.batch:
        rng = np.random.default_rng(B)
        eng = ndp.BatchedNMPC(B, load_mlp=False)
        q = rng.normal(size=(B, 4))
        x0n = np.concatenate([rng.normal(0, 2, (B, 6)), q / np.linalg.norm(q, axis=1, keepdims=True)], axis=1)
        un = np.concatenate([rng.uniform(CP.w_min, CP.w_max, (K, B, 3)), rng.uniform(CP.c_min, CP.c_max, (K, B, 1))], axis=2)
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)      # noqa: E731
        x0, u, f = t(x0n), t(un), t(rng.normal(0, 4, (K, B, 3)))
        g = t(rng.normal(size=(K, B, 10)))
        tan = {T: (t(rng.normal(size=(B, T, 10))), t(rng.normal(size=(K, B, T, 4))), t(rng.normal(size=(K, B, T, 3)))) for T in (1, 8)}
        xs, log, x = torch.empty_like(g), torch.empty_like(g), torch.empty_like(x0)
        gx0, gu, gf = torch.empty_like(x0), torch.empty_like(u), torch.empty_like(f)
        dxs = {T: torch.empty(K, B, T, 10, dtype=torch.float64, device=dev) for T in (1, 8)}
        sp = C.c_void_p(stream.cuda_stream)
        step_args = [(eng._h, C.c_void_p(x.data_ptr()), C.c_void_p(u[k].data_ptr()), C.c_void_p(f[k].data_ptr()), C.c_double(dt), sub, sp)
                     for k in range(K)]
        step = eng._lib.ndp_plant_step_device

        def per_tick():
            x.copy_(x0, non_blocking=True)
            for k in range(K):
                if step(*step_args[k]) != 0:
                    raise RuntimeError("ndp_plant_step_device failed")
                log[k].copy_(x, non_blocking=True)

        forms = {
            "per_tick": per_tick,
            "rollout": lambda: eng.plant_rollout_device(x0, u, xs, f=f, dt=dt, substeps=sub, stream=stream),
            "vjp": lambda: eng.plant_rollout_vjp_device(x0, u, xs, g, f=f, gx0=gx0, gu=gu, gf=gf, dt=dt, substeps=sub, stream=stream),
            "jvp1": lambda: eng.plant_rollout_jvp_device(x0, u, dxs[1], f=f, tx0=tan[1][0], tu=tan[1][1], tf=tan[1][2], dt=dt, substeps=sub,
                                                         stream=stream),
            "jvp8": lambda: eng.plant_rollout_jvp_device(x0, u, dxs[8], f=f, tx0=tan[8][0], tu=tan[8][1], tf=tan[8][2], dt=dt, substeps=sub,
                                                         stream=stream),
        }

        def run(call, passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for _ in range(passes):
                    call()
                stream.synchronize()
            return (time.perf_counter() - t0) / passes * 1e6

        for call in forms.values():
            run(call, a.warmup)
        same_log = bool(torch.equal(xs, log))                   # the one-launch log against the per-tick route's: the same bits
        times = {k: [] for k in forms}
        for _ in range(a.repeats):                              # alternating: what else runs on the host moves all alike
            for k, call in forms.items():
                times[k].append(run(call, a.passes))

        # torch autograd through the transcription: forward + backward, a handful of passes
        xa, ua, fa = (v.clone().requires_grad_(True) for v in (x0, u, f))

        def torch_pass():
            for v in (xa, ua, fa):
                v.grad = None
            (torch_plant(xa, ua, fa, dt, sub, eng.cfg.mass, eng.cfg.gravity) * g).sum().backward()

        run(torch_pass, 1)
        times["torch"] = [run(torch_pass, a.torch_passes) for _ in range(3)]
        gx0_dev_vs_torch = float((gx0 - xa.grad).abs().max())
        eng.close()
        med = {k + "_us": float(np.median(v)) for k, v in times.items()}
        out[str(B)] = {"median": med, "min_max": {k + "_us": [float(min(v)), float(max(v))] for k, v in times.items()},
                       "per_tick_over_rollout": med["per_tick_us"] / med["rollout_us"], "vjp_over_rollout": med["vjp_us"] / med["rollout_us"],
                       "jvp8_over_jvp1": med["jvp8_us"] / med["jvp1_us"], "torch_over_rollout_plus_vjp": med["torch_us"] / (med["rollout_us"] + med["vjp_us"]),
                       "one_launch_log_equals_per_tick_log": same_log, "gx0_device_minus_torch_max": gx0_dev_vs_torch}
    print(json.dumps({"experiment": "the plant over an input sequence: per-tick launches + copies, one launch, reverse mode, forward mode, torch autograd",
                      "device": torch.cuda.get_device_name(0), "ticks": K, "substeps": sub, "passes": a.passes, "warmup": a.warmup,
                      "repeats": a.repeats, "torch_passes": a.torch_passes, "batch": out}))


if __name__ == "__main__":
    main()
