#!/usr/bin/env python3
"""Forward mode of a closed-loop flight, one call against the layer's chain, as one JSON line.  B vehicles of the mixed workload, K ticks,
N = 20, a float32 force the controller sees and a force on the plant, T directions of x_0, xr, ur, f and fp:

  chain_us      torch_layer.control_step_jvp -> plant_rollout_jvp(ticks = 1), tick by tick (per tick: a tape of three clones, the step,
                the step's forward mode on a copy of the tape, the plant's tangent with its primal) -- the route there was before,
                unchanged;
  one_call_us   torch_layer.closed_loop_jvp: ndp_closed_loop_device with a tape, then ndp_closed_loop_jvp_device.

    python scripts/bench_closed_loop_jvp.py [--batch 1024 16384] [--ticks 20] [--tangents 1 8] [--passes 2] [--warmup 1] [--repeats 5]

Each figure is a host clock around `passes` passes on a side stream that ends in a stream synchronise, after `warmup` passes of the same
kind; every pass starts from the same iterate (reset_device to tick 0's window, then one warm-up step); the forms are timed alternately
`repeats` times and the median is reported with the spread (scripts/bench_closed_loop_grad.py's pattern).  The windows are those of 1024
vehicles, tiled over the batch.

    python scripts/bench_closed_loop_jvp.py --trace-form one_call --batch 1024 --ticks 4 --tangents 1

runs ONE pass of one form and nothing else: what a kernel trace counts launches on (the difference of two tick counts is the per-tick
figure)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_closed_loop_grad import inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--ticks", type=int, nargs="+", default=[20])
    ap.add_argument("--tangents", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-form", choices=["chain", "one_call"], default=None)
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
            for T in a.tangents:
                v = inputs(B, K, N, 20231516, dt)
                t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
                x0, xr, ur, f, fp = (t(v[n]) for n in ("x0", "xr", "ur", "f", "fp"))
                g = torch.Generator(device=dev).manual_seed(B + K + T)
                tx0, txr, tur, tf, tfp = (torch.randn(s, generator=g, dtype=torch.float64, device=dev) for s in (
                    (B, T, 10), (K, B, T, N + 1, 10), (K, B, T, N, 4), (K, B, T, N + 1, 3), (K, B, T, 3)))
                eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
                u0 = torch.empty(B, 4, dtype=torch.float64, device=dev)

                def prepare():
                    eng.reset_device(xr[0], ur[0], stream=stream)
                    eng.update_device(x0, xr[0], ur[0], u0, f=f[0], stream=stream)

                def chain():
                    prepare()
                    x, tx, dxs = x0, tx0, []
                    for k in range(K):
                        uk, X, U, du0, dX, dU = TL.control_step_jvp(eng, x, xr[k], ur[k], (tx, txr[k], tur[k], tf[k]), f=f[k])
                        xs, dx = TL.plant_rollout_jvp(eng, x, uk[None], (tx, du0[None], tfp[k][None]), f=fp[k][None], dt=dt)
                        x, tx = xs[0], dx[0]
                        dxs.append(tx)
                    return torch.stack(dxs)

                def one_call():
                    prepare()
                    return TL.closed_loop_jvp(eng, x0, xr, ur, (tx0, txr, tur, tf, tfp), f=f, fp=fp, dt=dt)[3]

                forms = {"chain": chain, "one_call": one_call}

                def run(call, passes):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with torch.cuda.stream(stream):
                        for _ in range(passes):
                            res = call()
                        stream.synchronize()
                    return (time.perf_counter() - t0) / passes * 1e6, res

                if a.trace_form:
                    run(forms[a.trace_form], 1)
                    eng.close()
                    continue
                res = {k: run(call, a.warmup)[1] for k, call in forms.items()}
                # the two routes' tangents side by side (the step link is the same kernel on the same data; the plant's tangent may round
                # differently from one kernel to the next)
                ok = torch.isfinite(res["chain"]).all(dim=3).all(dim=2).all(dim=0) & torch.isfinite(res["one_call"]).all(dim=3).all(dim=2).all(dim=0)
                ddx = float((res["chain"][:, ok] - res["one_call"][:, ok]).abs().max())
                times = {k: [] for k in forms}
                for _ in range(a.repeats):                          # alternating: what else runs on the host moves all alike
                    for k, call in forms.items():
                        times[k].append(run(call, a.passes)[0])
                st = eng.status()[0]
                eng.close()
                med = {k + "_us": float(np.median(x)) for k, x in times.items()}
                out[f"B{B}_K{K}_T{T}"] = {"median": med, "min_max": {k + "_us": [float(min(x)), float(max(x))] for k, x in times.items()},
                                          "chain_over_one_call": med["chain_us"] / med["one_call_us"],
                                          "dxs_chain_minus_one_call_max": ddx, "vehicles_compared": int(ok.sum()),
                                          "status_nonzero_last_tick": int((st != 0).sum())}
                del x0, xr, ur, f, fp, tx0, txr, tur, tf, tfp, res
                torch.cuda.empty_cache()
    if a.trace_form:
        return
    print(json.dumps({"experiment": "forward mode of a closed-loop flight: the layer's chain against one call", "N": N,
                      "device": torch.cuda.get_device_name(0), "passes": a.passes, "warmup": a.warmup, "repeats": a.repeats, "shapes": out}))


if __name__ == "__main__":
    main()
