#!/usr/bin/env python3
"""Forward mode of a closed-loop flight with and without a direction of the model, as one JSON line.  B vehicles of the mixed workload, K
ticks, N = 20, a float32 force the controller sees and a force on the plant, T directions of x_0, xr, ur, f and fp in both forms:

  plain_us   torch_layer.closed_loop_jvp: ndp_closed_loop_device with a tape, then ndp_closed_loop_jvp_device (rti_jvp_kernel per tick);
  model_us   the same call with tmodel [B,T,16] beside them: ndp_closed_loop_jvp_model_device (rti_mjvp_kernel per tick).

    python scripts/bench_closed_loop_model_jvp.py [--batch 1024] [--ticks 20] [--tangents 1 8] [--passes 2] [--warmup 1] [--repeats 5]

Timed the way scripts/bench_closed_loop_jvp.py times: a host clock around `passes` passes on a side stream that ends in a stream
synchronise, after `warmup` passes of the same kind; every pass starts from the same iterate; the forms are timed alternately `repeats`
times and the median is reported with the spread."""
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
    ap.add_argument("--batch", type=int, nargs="+", default=[1024])
    ap.add_argument("--ticks", type=int, nargs="+", default=[20])
    ap.add_argument("--tangents", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import isa_inspect, _lib
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
                tan = tuple(torch.randn(s, generator=g, dtype=torch.float64, device=dev) for s in (
                    (B, T, 10), (K, B, T, N + 1, 10), (K, B, T, N, 4), (K, B, T, N + 1, 3), (K, B, T, 3)))
                tm = torch.randn((B, T, 16), generator=g, dtype=torch.float64, device=dev)
                eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
                u0 = torch.empty(B, 4, dtype=torch.float64, device=dev)

                def prepare():
                    eng.reset_device(xr[0], ur[0], stream=stream)
                    eng.update_device(x0, xr[0], ur[0], u0, f=f[0], stream=stream)

                def plain():
                    prepare()
                    return TL.closed_loop_jvp(eng, x0, xr, ur, tan, f=f, fp=fp, dt=dt)[3]

                def model():
                    prepare()
                    return TL.closed_loop_jvp(eng, x0, xr, ur, tan, f=f, fp=fp, dt=dt, tmodel=tm)[3]

                forms = {"plain": plain, "model": model}

                def run(call, passes):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with torch.cuda.stream(stream):
                        for _ in range(passes):
                            res = call()
                        stream.synchronize()
                    return (time.perf_counter() - t0) / passes * 1e6, res

                res = {k: run(call, a.warmup)[1] for k, call in forms.items()}
                ok = torch.isfinite(res["plain"]).all(dim=3).all(dim=2).all(dim=0) & torch.isfinite(res["model"]).all(dim=3).all(dim=2).all(dim=0)
                times = {k: [] for k in forms}
                for _ in range(a.repeats):                          # alternating: what else runs on the host moves all alike
                    for k, call in forms.items():
                        times[k].append(run(call, a.passes)[0])
                eng.close()
                med = {k + "_us": float(np.median(x)) for k, x in times.items()}
                out[f"B{B}_K{K}_T{T}"] = {"median": med, "min_max": {k + "_us": [float(min(x)), float(max(x))] for k, x in times.items()},
                                          "model_over_plain": med["model_us"] / med["plain_us"], "vehicles_finite_in_both": int(ok.sum())}
                del x0, xr, ur, f, fp, tan, tm, res
                torch.cuda.empty_cache()
    regs = {n: {k: m[k] for k in ("vgpr", "agpr", "scratch")} for n, m in isa_inspect.CodeObject(_lib.LIB_PATH).kernels().items()
            if "rti_mjvp_kernel" in n or "rti_jvp_kernel" in n}
    print(json.dumps({"experiment": "forward mode of a closed-loop flight: with a model direction against without", "N": N,
                      "device": torch.cuda.get_device_name(0), "passes": a.passes, "warmup": a.warmup, "repeats": a.repeats, "shapes": out,
                      "registers": regs}))


if __name__ == "__main__":
    main()
