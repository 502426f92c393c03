#!/usr/bin/env python3
"""Forward and gradient of a loss on a FORMATION's closed-loop flight -- the downwash force on the plant made from the vehicles' actual states
at every tick -- one call per direction against the layer's per-tick chain, as one JSON line.  B vehicles in stacked triples (every vehicle
hears the two others of its triple, K = 2 slots; a batch that is no multiple of three ends in vehicles that hear nobody), `ticks` ticks,
N = 20, a float32 force the controller sees, the loss L = sum_k <G_k, x_{k+1}> + <H_k, u0_k> + <A_k, X_k> + <F_k, fps_k>, gradients in x_0
and the network's weights:

  chain_us      torch_layer.plant_force -> control_step_trajectory -> plant_step, tick by tick, and autograd's backward through it (back,
                per tick: the plant's adjoint, the force's adjoint and its index_add_ scatter, the step's adjoint, torch's additions);
  one_call_us   torch_layer.closed_loop_formation and its backward: ndp_closed_loop_formation_device +
                ndp_closed_loop_formation_vjp_device (the scatter is a gather inside the link's launch, g_w is summed on the device);
  *_fwd_us      the forward of each alone, under torch.no_grad().

    python scripts/bench_closed_loop_formation.py [--batch 1024 16384] [--ticks 20] [--passes 2] [--warmup 1] [--repeats 5]

Timing as scripts/bench_closed_loop_grad.py: a host clock around `passes` passes on a side stream that ends in a stream synchronise, after
`warmup` passes of the same kind; every pass starts from the same iterate; the forms are timed alternately `repeats` times; median and
spread.  Values are compared bit for bit; the two gradients by their largest difference over the largest entry."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIXED = dict(pos_sigma=0.05, vel_sigma=0.1, quat_sigma=0.05)
DZ = 0.7       # the triples' vertical spacing (tests/closed_loop_formation_ref.py)


def inputs(B, K, N, seed, dt):
    """Windows of min(B, 1023) // 3 triples of the mixed workload, each triple on ONE path DZ apart, tiled over the batch."""
    from ndp_nmpc_qd_amd import synth
    b0 = min(B, 1023) // 3
    b = [synth.make_batch(b0, N=N, seed=seed, t0=k * dt, **MIXED) for k in range(K)]
    stack = lambda v: np.repeat(v, 3, axis=0)                                   # noqa: E731
    x0, xr, ur = stack(b[0]["x0"]), np.stack([stack(v["xr"]) for v in b]), np.stack([stack(v["ur"]) for v in b])
    lift = (np.arange(3 * b0) % 3) * DZ
    x0[:, 2] += lift
    xr[:, :, :, 2] += lift[None, :, None]
    reps = -(-B // (3 * b0))
    tile = lambda v, axis: np.ascontiguousarray(np.concatenate([v] * reps, axis=axis).take(range(B), axis=axis))  # noqa: E731
    v = np.arange(B)
    t, m = v // 3 * 3, v % 3
    index = np.stack([t + (m + 1) % 3, t + (m + 2) % 3], axis=1).astype(np.int32)
    index[index >= B] = -1
    index[B - B % 3:] = -1                                                      # an incomplete last triple hears nobody
    rng = np.random.default_rng(seed + 1)
    return dict(x0=tile(x0, 0), xr=tile(xr, 1), ur=tile(ur, 1), f=rng.normal(0.0, 0.1, (K, B, N + 1, 3)).astype(np.float32), index=index)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--ticks", type=int, nargs="+", default=[20])
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import _lib
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
            x0 = t(v["x0"]).requires_grad_(True)
            xr, ur, f, idx = t(v["xr"]), t(v["ur"]), t(v["f"]), t(v["index"])
            w = t(_lib.load_weights()).requires_grad_(True)
            g = torch.Generator(device=dev).manual_seed(B + K)
            G, H, A, Fu = (torch.randn(s, generator=g, dtype=torch.float64, device=dev)
                           for s in ((K, B, 10), (K, B, 4), (K, B, N + 1, 10), (K, B, 3)))
            eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
            xr0, ur0, f0, u0 = xr[0], ur[0], f[0], torch.empty(B, 4, dtype=torch.float64, device=dev)

            def prepare():
                eng.reset_device(xr0, ur0, stream=stream)
                eng.update_device(x0.detach(), xr0, ur0, u0, f=f0, stream=stream)

            def chain(grad=True):
                prepare()
                x, L = x0, 0.0
                for k in range(K):
                    fp = TL.plant_force(eng, x, idx, weights=w)
                    uk, X, _ = TL.control_step_trajectory(eng, x, xr[k], ur[k], f=f[k])
                    x = TL.plant_step(eng, x, uk, fp, dt=dt)
                    if grad:
                        L = L + (G[k] * x).sum() + (H[k] * uk).sum() + (A[k] * X).sum() + (Fu[k] * fp).sum()
                return (x.detach(),) + (tuple(torch.autograd.grad(L, (x0, w))) if grad else ())

            def one_call(grad=True):
                prepare()
                xs, us, Xs, fps = TL.closed_loop_formation(eng, x0, xr, ur, idx, f=f, weights=w, dt=dt)
                if not grad:
                    return (xs[-1].detach(),)
                return (xs[-1].detach(),) + tuple(torch.autograd.grad((G * xs).sum() + (H * us).sum() + (A * Xs).sum() + (Fu * fps).sum(), (x0, w)))

            def no_grad(call):
                def run_():
                    with torch.no_grad():
                        return call(False)
                return run_
            forms = {"chain": chain, "one_call": one_call, "chain_fwd": no_grad(chain), "one_call_fwd": no_grad(one_call)}

            def run(call, passes):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.cuda.stream(stream):
                    for _ in range(passes):
                        res = call()
                    stream.synchronize()
                return (time.perf_counter() - t0) / passes * 1e6, res

            res = {k: run(call, a.warmup)[1] for k, call in forms.items()}
            ok = torch.isfinite(res["chain"][1]).all(dim=1) & torch.isfinite(res["one_call"][1]).all(dim=1)
            rel = lambda p, q: float((p - q).abs().max() / q.abs().max().clamp_min(1e-300))      # noqa: E731
            cmp_ = dict(x_last_bit_equal=bool(torch.equal(res["chain"][0], res["one_call"][0])),
                        gx0_rel=rel(res["chain"][1][ok], res["one_call"][1][ok]), gw_rel=rel(res["chain"][2].double(), res["one_call"][2].double()),
                        vehicles_compared=int(ok.sum()))
            times = {k: [] for k in forms}
            for _ in range(a.repeats):                          # alternating: what else runs on the host moves all alike
                for k, call in forms.items():
                    times[k].append(run(call, a.passes)[0])
            st = eng.status()[0]
            eng.close()
            med = {k + "_us": float(np.median(x)) for k, x in times.items()}
            out[f"B{B}_ticks{K}"] = {"median": med, "min_max": {k + "_us": [float(min(x)), float(max(x))] for k, x in times.items()},
                                 "chain_over_one_call": med["chain_us"] / med["one_call_us"],
                                 "chain_fwd_over_one_call_fwd": med["chain_fwd_us"] / med["one_call_fwd_us"], **cmp_,
                                 "status_nonzero_last_tick": int((st != 0).sum())}
            del x0, xr, ur, f, G, H, A, Fu, res
            torch.cuda.empty_cache()
    print(json.dumps({"experiment": "gradient of a formation's closed-loop loss: the layer's chain against one call per direction", "N": N,
                      "device": torch.cuda.get_device_name(0), "passes": a.passes, "warmup": a.warmup, "repeats": a.repeats, "shapes": out}))


if __name__ == "__main__":
    main()
