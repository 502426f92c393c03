#!/usr/bin/env python3
"""Time per training epoch of the downwash network (loss, weight gradient, optimiser step) on one device, two ways, as one JSON line:

  rows_us      the fit on sample rows: torch_layer.downwash_fit_rows (ONE fused call: forward, loss and weight gradient,
               ndp_mlp_fit_rows_device) + DownwashAdamSN -- full batch, and with --batch-size as one mini-batch step on an index list;
  windows_us   the path on prediction windows: the rows packed 21 to an instance of an engine of ceil(n / 21) instances,
               torch_layer.downwash + torch MSE on the masked rows + backward (ndp_downwash_vjp_device) + DownwashAdamSN.

    python scripts/bench_fit_rows.py [--rows 6144 98304] [--epochs 100] [--warmup 10] [--repeats 5] [--batch-size 512]

Both are a host clock around `epochs` epochs on a side stream that end in a stream synchronise, after `warmup` epochs of the same kind;
the forms are timed alternately `repeats` times and the median is reported with the spread (scripts/bench_train_step.py's pattern).  The
data are synthetic rows labelled by the shipped network, the start is the shipped blob perturbed by 2 %.  There is no speed bar on
these numbers; they go into DESIGN section 9 as measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NODES = 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[6144, 98304])
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--sn", type=float, default=4.0)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import _lib
    from ndp_nmpc_qd_amd.torch_layer import DownwashAdamSN, downwash, downwash_fit_rows, downwash_rows
    dev = torch.device("cuda:0")
    blob = _lib.load_weights()
    stream = torch.cuda.Stream(device=dev)
    out = {}
    for n in a.rows:
        rng = np.random.default_rng(n)
        x = np.concatenate([rng.uniform(-1.5, 1.5, (n, 3)), rng.uniform(-3.0, 3.0, (n, 3))], axis=1).astype(np.float32)
        start = (blob.astype(np.float64) * (1.0 + 0.02 * rng.normal(size=blob.size))).astype(np.float32)
        small = ndp.BatchedNMPC(1, N=NODES - 1, disturbance=True)
        z = torch.from_numpy(x).to(dev)
        y = downwash_rows(small, z, weights=torch.from_numpy(blob).to(dev))
        # the same rows on windows
        Bw = (n + NODES - 1) // NODES
        big = ndp.BatchedNMPC(Bw, N=NODES - 1, disturbance=True)
        other = torch.zeros(Bw * NODES, 10, dtype=torch.float64, device=dev)
        other[:n, :6] = z.double()
        other = other.reshape(Bw, NODES, 10)
        ego = torch.zeros_like(other)
        target = torch.zeros(Bw * NODES, 3, dtype=torch.float32, device=dev)
        target[:n] = y
        target = target.reshape(Bw, NODES, 3)
        mask = torch.zeros(Bw * NODES, 1, dtype=torch.float32, device=dev)
        mask[:n] = 1.0
        mask = mask.reshape(Bw, NODES, 1)
        scale = 1.0 / (3.0 * n)
        M = min(a.batch_size, n)

        def run(form, epochs):
            eng = big if form == "windows" else small
            w = torch.nn.Parameter(torch.from_numpy(start).to(dev))
            opt = DownwashAdamSN(w, eng, sn=a.sn)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for _ in range(epochs):
                    opt.zero_grad()
                    if form == "windows":
                        d = (downwash(eng, other, ego, weights=w) - target) * mask
                        loss = (d * d).sum() * scale
                    elif form == "rows":
                        loss = downwash_fit_rows(eng, z, y, w)
                    else:                   # one mini-batch step: a fresh permutation's head as the index list, nothing to the host
                        idx = torch.randperm(n, device=dev)[:M].to(torch.int32)
                        loss = downwash_fit_rows(eng, z, y, w, index=idx)
                    loss.backward()
                    opt.step()
                stream.synchronize()
            dt = time.perf_counter() - t0
            assert int(opt.state[w]["step"].item()) == epochs
            return dt / epochs * 1e6, float(loss.detach())

        forms = ("rows", "windows", "rows_minibatch")
        times, last = {k: [] for k in forms}, {}
        for k in forms:
            run(k, a.warmup)
        for _ in range(a.repeats):                  # alternating: what else runs on the host moves all alike
            for k in forms:
                us, last[k] = run(k, a.epochs)
                times[k].append(us)
        small.close()
        big.close()
        med = {k: float(np.median(v)) for k, v in times.items()}
        out[str(n)] = {"us_per_epoch_median": med, "us_per_epoch_min_max": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
                       "windows_over_rows": med["windows"] / med["rows"], "minibatch_rows": M, "windows_instances": Bw,
                       "loss_after": last}
    print(json.dumps({"experiment": "one training epoch of the downwash network: loss, weight gradient, Adam + spectral-norm cap",
                      "device": torch.cuda.get_device_name(0), "epochs": a.epochs, "warmup": a.warmup, "repeats": a.repeats, "sn": a.sn,
                      "rows": out}))


if __name__ == "__main__":
    main()
