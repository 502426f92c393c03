#!/usr/bin/env python3
"""Time per optimiser step of the downwash network on one device, two ways, as one JSON line:

  device_step_us   ndp_mlp_adam_sn_device (Adam + the four norms + the cap in ONE launch, the step counter on the device), with and
                   without installing the new weights behind it, sn at the shipped norms (every layer scaled in most steps) and off;
  torch_step_us    the reference's lines in torch (nn_train.py:147-157): torch.optim.Adam.step() on the eight parameter tensors, then per
                   weight matrix torch.linalg.matrix_norm(W, 2) and the host branch `if s > SN: W.data = W / s * SN` -- four
                   device-to-host synchronisations per step.

    python scripts/bench_train_step.py [--steps 300] [--warmup 30] [--repeats 5]

Both are a host clock around `steps` steps that end in a device synchronise, after `warmup` steps of the same kind; the two are timed
alternately `repeats` times and the median is reported with the spread.  The gradient is a fixed random tensor (the backward pass that
makes it is the same for both and is not timed).  There is no speed bar on this number; it goes into DESIGN section 9 as measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sn", type=float, default=4.0)
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import _lib, mlp_frag
    dev = torch.device("cuda:0")
    blob = _lib.load_weights()
    rng = np.random.default_rng(5)
    grad = torch.from_numpy((1e-3 * rng.normal(size=blob.size)).astype(np.float32)).to(dev)
    eng = ndp.BatchedNMPC(4, N=20, disturbance=True)
    stream = torch.cuda.Stream(device=dev)

    def device_run(steps, sn, install):
        w = torch.from_numpy(blob).to(dev)
        m, v = torch.zeros_like(w), torch.zeros_like(w)
        st = torch.zeros(1, dtype=torch.int64, device=dev)
        sig, info = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.mlp_adam_sn_device(w, grad, m, v, st, sn=sn, sigma=sig, info=info, install=install, stream=stream)
        stream.synchronize()
        dt = time.perf_counter() - t0
        assert int(st.item()) == steps
        return dt / steps * 1e6, sig.cpu().numpy()

    def torch_run(steps, sn):
        params = [torch.nn.Parameter(torch.from_numpy(np.array(p)).to(dev)) for p in mlp_frag.split(blob).values()]
        grads = [torch.from_numpy(np.array(g)).to(dev) for g in mlp_frag.split(grad.cpu().numpy()).values()]
        opt = torch.optim.Adam(params, lr=1e-4)
        for p, g in zip(params, grads):
            p.grad = g
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.step()
            if sn > 0:
                for p in params:
                    W = p.detach()
                    if W.ndim > 1:
                        s = torch.linalg.matrix_norm(W, 2)
                        if s > sn:
                            p.data = p / s * sn
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt / steps * 1e6, np.array([float(torch.linalg.matrix_norm(p.detach().double(), 2)) for p in params if p.ndim > 1])

    forms = {"device_sn_install": lambda n: device_run(n, a.sn, True), "device_sn": lambda n: device_run(n, a.sn, False),
             "device_nocap": lambda n: device_run(n, 0.0, False), "torch_sn": lambda n: torch_run(n, a.sn),
             "torch_nocap": lambda n: torch_run(n, 0.0)}
    times, sigma = {k: [] for k in forms}, {}
    for f in forms.values():
        f(a.warmup)
    for _ in range(a.repeats):                      # alternating: what else runs on the host moves both alike
        for k, f in forms.items():
            us, sigma[k] = f(a.steps)
            times[k].append(us)
    eng.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"experiment": "one optimiser step of the downwash network (17 859 parameters): Adam + spectral-norm cap",
                      "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "sn": a.sn,
                      "us_per_step_median": med, "us_per_step_min_max": {k: [float(min(v)), float(max(v))] for k, v in times.items()},
                      "torch_over_device_sn": med["torch_sn"] / med["device_sn"],
                      "sigma_after": {k: [float(x) for x in s] for k, s in sigma.items()}}))


if __name__ == "__main__":
    main()
