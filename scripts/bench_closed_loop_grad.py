#!/usr/bin/env python3
"""Forward + backward of a loss on a closed-loop flight, one call per direction against the layer's chain, as one JSON line.  B vehicles of
the mixed workload, K ticks, N = 20, a float32 force the controller sees and a force on the plant, the loss
L = sum_k <G_k, x_{k+1}> + <H_k, u0_k> + <A_k, X_k>, gradients in x_0, xr, ur, f and fp:

  chain_us      torch_layer.control_step_trajectory -> plant_step, tick by tick, and autograd's backward through it (per tick: a tape of three
                clones, the step, the plant; back: the plant's adjoint, three copies, the step's adjoint, torch's additions) -- the route
                there was before, unchanged;
  one_call_us   torch_layer.closed_loop and its backward: ndp_closed_loop_device + ndp_closed_loop_vjp_device;
  one_call_model_us   the same with Qd, Rd and the mass requiring a gradient as well (rti_wvjp_kernel instead of rti_vjp_kernel).

    python scripts/bench_closed_loop_grad.py [--batch 1024 16384] [--ticks 20 100] [--passes 2] [--warmup 1] [--repeats 5]

Each figure is a host clock around `passes` forward + backward passes on a side stream that ends in a stream synchronise, after `warmup`
passes of the same kind; every pass starts from the same iterate (reset_device to tick 0's window, then one warm-up step); the forms are
timed alternately `repeats` times and the median is reported with the spread (scripts/bench_plant_rollout.py's pattern).  The windows are
those of 1024 vehicles, tiled over the batch."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIXED = dict(pos_sigma=0.5, vel_sigma=1.0, quat_sigma=0.15)      # bench.py's `mixed` workload


def inputs(B, K, N, seed, dt):
    from ndp_nmpc_qd_amd import synth
    b0 = min(B, 1024)
    b = [synth.make_batch(b0, N=N, seed=seed, t0=k * dt, **MIXED) for k in range(K)]
    rng = np.random.default_rng(seed + 1)
    tile = lambda v, axis: np.concatenate([v] * (B // b0), axis=axis) if B > b0 else v  # noqa: E731
    return dict(x0=tile(b[0]["x0"], 0), xr=tile(np.stack([v["xr"] for v in b]), 1), ur=tile(np.stack([v["ur"] for v in b]), 1),
                f=rng.normal(0.0, 0.3, (K, B, N + 1, 3)).astype(np.float32), fp=rng.normal(0.0, 1.0, (K, B, 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--ticks", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import torch_layer as TL
    from ndp_nmpc_qd_amd.params import nmpc_params as CP
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    N, dt = 20, CP.ts_nmpc
    out = {}
    for B in a.batch:
        for K in a.ticks:
            v = inputs(B, K, N, 20231516, dt)
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
            x0, xr, ur, f, fp = (t(v[n]).requires_grad_(True) for n in ("x0", "xr", "ur", "f", "fp"))
            g = torch.Generator(device=dev).manual_seed(B + K)
            G, H, A = (torch.randn(s, generator=g, dtype=torch.float64, device=dev) for s in ((K, B, 10), (K, B, 4), (K, B, N + 1, 10)))
            eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
            Qd = torch.tensor(list(eng.cfg.Qd), dtype=torch.float64, requires_grad=True)
            Rd = torch.tensor(list(eng.cfg.Rd), dtype=torch.float64, requires_grad=True)
            mass = torch.tensor(float(eng.cfg.mass), dtype=torch.float64, requires_grad=True)
            xr0, ur0, f0, u0 = xr[0].detach(), ur[0].detach(), f[0].detach(), torch.empty(B, 4, dtype=torch.float64, device=dev)
            leaves = (x0, xr, ur, f, fp)
            # the chain's leaves: one tensor per tick (a select of a [K, ...] leaf would cost the chain a full-size zero fill per tick)
            per_tick = [[w[k].detach().requires_grad_(True) for k in range(K)] for w in (xr, ur, f, fp)]
            chain_leaves = [x0] + [w for ws in per_tick for w in ws]

            def prepare():
                eng.reset_device(xr0, ur0, stream=stream)
                eng.update_device(x0.detach(), xr0, ur0, u0, f=f0, stream=stream)

            def chain():
                prepare()
                x, L = x0, 0.0
                for k in range(K):
                    uk, X, _ = TL.control_step_trajectory(eng, x, per_tick[0][k], per_tick[1][k], f=per_tick[2][k])
                    x = TL.plant_step(eng, x, uk, per_tick[3][k], dt=dt)
                    L = L + (G[k] * x).sum() + (H[k] * uk).sum() + (A[k] * X).sum()
                return torch.autograd.grad(L, chain_leaves)

            def one_call(model=False):
                prepare()
                kw = dict(Qd=Qd, Rd=Rd, mass=mass) if model else {}
                xs, us, Xs = TL.closed_loop(eng, x0, xr, ur, f=f, fp=fp, dt=dt, **kw)
                return torch.autograd.grad((G * xs).sum() + (H * us).sum() + (A * Xs).sum(), leaves + ((Qd, Rd, mass) if model else ()))

            forms = {"chain": chain, "one_call": one_call, "one_call_model": lambda: one_call(True)}

            def run(call, passes):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.cuda.stream(stream):
                    for _ in range(passes):
                        res = call()
                    stream.synchronize()
                return (time.perf_counter() - t0) / passes * 1e6, res

            res = {k: run(call, a.warmup)[1] for k, call in forms.items()}
            # the two routes' gradients side by side (not bit-equal: the plant's adjoint may round differently from one kernel to the next)
            ok = torch.isfinite(res["chain"][0]).all(dim=1) & torch.isfinite(res["one_call"][0]).all(dim=1)
            dgx0 = float((res["chain"][0][ok] - res["one_call"][0][ok]).abs().max())
            times = {k: [] for k in forms}
            for _ in range(a.repeats):                          # alternating: what else runs on the host moves all alike
                for k, call in forms.items():
                    times[k].append(run(call, a.passes)[0])
            st = eng.status()[0]
            eng.close()
            med = {k + "_us": float(np.median(x)) for k, x in times.items()}
            out[f"B{B}_K{K}"] = {"median": med, "min_max": {k + "_us": [float(min(x)), float(max(x))] for k, x in times.items()},
                                 "chain_over_one_call": med["chain_us"] / med["one_call_us"],
                                 "gx0_chain_minus_one_call_max": dgx0, "vehicles_compared": int(ok.sum()),
                                 "status_nonzero_last_tick": int((st != 0).sum())}
            del x0, xr, ur, f, fp, G, H, A, res
            torch.cuda.empty_cache()
    print(json.dumps({"experiment": "gradient of a closed-loop loss: the layer's chain against one call per direction", "N": N,
                      "device": torch.cuda.get_device_name(0), "passes": a.passes, "warmup": a.warmup, "repeats": a.repeats, "shapes": out}))


if __name__ == "__main__":
    main()
