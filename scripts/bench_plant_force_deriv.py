#!/usr/bin/env python3
"""Time of the derivatives of the downwash force on the plant on one device, as one JSON line: B vehicles, K neighbour slots each, N = 20.

  vjp_us / jvp1_us / jvp4_us   ndp_plant_force_multi_vjp_device (gz and gw), ndp_plant_force_multi_jvp_device with T = 1 / 4 directions of
                               the states and the weights;
  win_vjp_us / win_jvp1_us / win_jvp4_us   the only route there was before: the vehicles packed into the engine's prediction windows
                               (other[o][n] = x[o], ego_ref[v][n] = x[v], ego_xy = x[v][0:2], upstream and directions at node 0) through
                               ndp_downwash_multi_vjp_device / ndp_downwash_multi_jvp_device, which compute N + 1 rows per vehicle to use
                               one.  The packing itself is done once, outside the timed region.

    python scripts/bench_plant_force_deriv.py [--batch 1024 16384] [--slots 1 2] [--passes 20] [--warmup 3] [--repeats 5]

Each figure is a host clock around `passes` calls on a side stream that ends in a stream synchronise, after `warmup` calls of the same
kind; the forms are timed alternately `repeats` times and the median is reported with the spread (scripts/bench_plant_rollout.py's
pattern).  There is no speed bar on these numbers; they go into DESIGN section 9 as measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import _lib
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    N, NP = 20, _lib.MLP_NPARAM
    out = {}
    for B in a.batch:
        eng = ndp.BatchedNMPC(B, N=N, disturbance=True)
        for K in a.slots:
            rng = np.random.default_rng(B + K)
            t = lambda v, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(v)).to(dev, dt)      # noqa: E731
            xn = np.concatenate([rng.uniform(-0.75, 0.75, (B, 3)), rng.uniform(-1.5, 1.5, (B, 3)), rng.normal(size=(B, 4))], axis=1)
            idxn = ((np.arange(B)[:, None] + 1 + rng.integers(0, B - 1, (B, K))) % B).astype(np.int32)
            idxn[rng.random((B, K)) < 0.15] = -1
            x, idx, gf = t(xn), t(idxn, torch.int32), t(rng.normal(size=(B, 3)))
            d2 = ((xn[np.clip(idxn, 0, None)][..., :2] - xn[:, None, :2]) ** 2).sum(axis=2)
            open_share = float(((idxn >= 0) & (d2 < eng.cfg.r_horiz ** 2)).mean())
            gz, gw = torch.empty(B, K, 6, dtype=torch.float64, device=dev), torch.empty(NP, dtype=torch.float32, device=dev)
            tx = {T: t(rng.normal(size=(B, T, 10))) for T in (1, 4)}
            tw = {T: t(0.01 * rng.normal(size=(T, NP)), torch.float32) for T in (1, 4)}
            df = {T: torch.empty(B, T, 3, dtype=torch.float64, device=dev) for T in (1, 4)}
            # the windows-packing route
            win = x[:, None, :].expand(B, N + 1, 10).contiguous()
            exy = x[:, :2].contiguous()
            up = torch.zeros(B, N + 1, 3, dtype=torch.float64, device=dev)
            up[:, 0] = gf
            wgz = torch.empty(B, K, N + 1, 6, dtype=torch.float64, device=dev)
            o = idx.clamp(min=0).long()
            tz, wdf = {}, {}
            for T in (1, 4):
                tz[T] = torch.zeros(B, T, K, N + 1, 6, dtype=torch.float64, device=dev)
                tz[T][:, :, :, 0] = (tx[T][o][..., :6] - tx[T][:, None, :, :6]).transpose(1, 2)
                wdf[T] = torch.empty(B, T, N + 1, 3, dtype=torch.float64, device=dev)
            forms = {
                "vjp": lambda: eng.plant_force_multi_vjp_device(x, idx, gf, gz=gz, gw=gw, stream=stream),
                "win_vjp": lambda: eng.downwash_multi_vjp_device(win, idx, win, up, ego_xy=exy, gz=wgz, gw=gw, stream=stream),
            }
            for T in (1, 4):
                forms[f"jvp{T}"] = lambda T=T: eng.plant_force_multi_jvp_device(x, idx, tx=tx[T], tw=tw[T], n_tan=T, df=df[T], stream=stream)
                forms[f"win_jvp{T}"] = lambda T=T: eng.downwash_multi_jvp_device(win, idx, win, tz=tz[T], tw=tw[T], ego_xy=exy, n_tan=T,
                                                                                 df=wdf[T], stream=stream)

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
            same = bool(torch.equal(gz, wgz[:, :, 0])) and all(bool(torch.equal(df[T], wdf[T][:, :, 0])) for T in (1, 4))
            times = {k: [] for k in forms}
            for _ in range(a.repeats):                          # alternating: what else runs on the host moves all alike
                for k, call in forms.items():
                    times[k].append(run(call, a.passes))
            med = {k + "_us": float(np.median(v)) for k, v in times.items()}
            out[f"{B}x{K}"] = {"median": med, "min_max": {k + "_us": [float(min(v)), float(max(v))] for k, v in times.items()},
                               "win_over_new": {k: med[f"win_{k}_us"] / med[f"{k}_us"] for k in ("vjp", "jvp1", "jvp4")},
                               "open_share_of_slots": open_share, "same_bits_as_the_windows_route": same}
        eng.close()
    print(json.dumps({"experiment": "derivatives of the downwash force on the plant: the new calls against the windows-packing route through the "
                                    "prediction's derivatives",
                      "device": torch.cuda.get_device_name(0), "N": N, "passes": a.passes, "warmup": a.warmup, "repeats": a.repeats,
                      "cases": out}))


if __name__ == "__main__":
    main()
