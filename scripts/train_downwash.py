#!/usr/bin/env python3
"""The reference's training loop (nn_train.py:129-157) on this library: full batch, MSE, Adam, the spectral-norm cap after every step.

    python scripts/train_downwash.py [--input downwash_input.csv --output downwash_output.csv] [--sn 4] [--epochs 10000] [--out FILE.bin]

Every epoch is three enqueues on one stream -- the network's forward (torch_layer.downwash), its backward (the weight gradient,
ndp_downwash_vjp_device) and ONE launch for Adam and the cap (torch_layer.DownwashAdamSN, ndp_mlp_adam_sn_device) -- and no value comes
back to the host except the losses printed every 1000 epochs.  The result is written as a blob file (17 859 float32, the order of
ndp_set_mlp_weights), with the four spectral norms printed beside it.

Data.  --input / --output: CSV files with the reference's column names (x, y, z, vx, vy, vz and fx, fy, fz), read with numpy; split 75 / 25
by a seeded permutation (the reference uses sklearn's split with random_state 42: the same proportions, not the same rows).  Without them:
--samples rows drawn uniformly in the training envelope (|dx|, |dy|, |dz| <= 1.5 m, |dv| <= 3 m/s) and labelled by the SHIPPED network.
That is a plumbing demonstration: the data are made by a network of the very architecture that is fitted, so it shows that the loop runs,
that the loss goes down and that the cap holds -- it says nothing about real downwash, and a fit to it is not a replacement for
downwash_sn4.bin.

The samples are packed 21 to an instance (the nodes of a prediction window, gates open); the rows that pad the last instance get a zero
upstream gradient and do not count in the mean.

Not the reference's: its --SN 0 path trains with dropout, this loop has none (with --sn 0 it is plain Adam); the start is nn.Linear's
default initialisation drawn with numpy's generator, not torch's."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NODES = 21


def read_csv(path, cols):
    a = np.genfromtxt(path, delimiter=",", names=True, dtype=np.float64)
    missing = [c for c in cols if c not in (a.dtype.names or ())]
    if missing:
        raise SystemExit(f"{path}: no column(s) {missing} (found {a.dtype.names})")
    return np.stack([np.atleast_1d(a[c]) for c in cols], axis=1)


def linear_init(rng):
    """nn.Linear's default: weights and biases U(-1/sqrt(fan_in), 1/sqrt(fan_in)), in blob order."""
    from ndp_nmpc_qd_amd import mlp_frag
    parts, fan = [], None
    for name, shp in mlp_frag.SHAPES:
        fan = shp[1] if len(shp) == 2 else fan
        parts.append(rng.uniform(-1.0, 1.0, size=shp).reshape(-1) / np.sqrt(fan))
    return np.concatenate(parts).astype(np.float32)


class Packed:
    """Rows x [n,6], y [n,3] on the nodes of ceil(n / 21) instances of an engine of their own."""

    def __init__(self, ndp, torch, dev, x, y):
        n = x.shape[0]
        self.B = (n + NODES - 1) // NODES
        pad = self.B * NODES - n
        z = np.zeros((self.B * NODES, 10))
        z[:n, :6] = x
        self.other = torch.from_numpy(z.reshape(self.B, NODES, 10)).to(dev)
        self.ego = torch.zeros_like(self.other)
        t = np.zeros((self.B * NODES, 3), dtype=np.float32)
        t[:n] = y
        self.target = torch.from_numpy(t.reshape(self.B, NODES, 3)).to(dev)
        m = np.r_[np.ones(n, dtype=np.float32), np.zeros(pad, dtype=np.float32)]
        self.mask = torch.from_numpy(m.reshape(self.B, NODES, 1)).to(dev)
        self.scale = 1.0 / (3.0 * n)
        self.engine = ndp.BatchedNMPC(self.B, N=NODES - 1, disturbance=True)

    def loss(self, downwash, w):
        """MSE over the real rows (nn.MSELoss: the mean over rows and components); the padding rows' upstream gradient is exactly 0."""
        d = (downwash(self.engine, self.other, self.ego, weights=w) - self.target) * self.mask
        return (d * d).sum() * self.scale


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input", help="CSV with columns x, y, z, vx, vy, vz")
    ap.add_argument("--output", help="CSV with columns fx, fy, fz")
    ap.add_argument("--sn", type=float, default=0.0, help="max spectral norm of a single layer (0: no cap)")
    ap.add_argument("--epochs", type=int, default=10000)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--samples", type=int, default=8192, help="synthetic rows when no CSV is given")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default="downwash_trained.bin")
    a = ap.parse_args()
    if (a.input is None) != (a.output is None):
        raise SystemExit("--input and --output go together")
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import _lib
    from ndp_nmpc_qd_amd.torch_layer import DownwashAdamSN, downwash
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    if a.input:
        x, y = read_csv(a.input, ("x", "y", "z", "vx", "vy", "vz")), read_csv(a.output, ("fx", "fy", "fz"))
        if x.shape[0] != y.shape[0]:
            raise SystemExit(f"{a.input} has {x.shape[0]} rows, {a.output} {y.shape[0]}")
        what = f"{x.shape[0]} rows of {a.input}"
    else:
        x = np.concatenate([rng.uniform(-1.5, 1.5, (a.samples, 3)), rng.uniform(-3.0, 3.0, (a.samples, 3))], axis=1)
        lab = Packed(ndp, torch, dev, x, np.zeros((a.samples, 3)))
        with torch.no_grad():
            f = downwash(lab.engine, lab.other, lab.ego, weights=torch.from_numpy(_lib.load_weights()).to(dev))
        torch.cuda.synchronize()
        y = f.cpu().numpy().reshape(-1, 3)[:a.samples]
        lab.engine.close()
        what = f"{a.samples} synthetic rows labelled by the shipped network (a plumbing demonstration, not downwash data)"
    perm = rng.permutation(x.shape[0])
    n_train = int(0.75 * x.shape[0])
    train = Packed(ndp, torch, dev, x[perm[:n_train]], y[perm[:n_train]])
    test = Packed(ndp, torch, dev, x[perm[n_train:]], y[perm[n_train:]])
    print(f"data: {what}; {n_train} train / {x.shape[0] - n_train} test rows on {train.B} / {test.B} instances; sn = {a.sn}, lr = {a.lr}")
    w = torch.nn.Parameter(torch.from_numpy(linear_init(rng)).to(dev))
    opt = DownwashAdamSN(w, train.engine, lr=a.lr, sn=a.sn)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for epoch in range(a.epochs):
            opt.zero_grad()
            loss = train.loss(downwash, w)
            loss.backward()
            opt.step()
            if (epoch + 1) % 1000 == 0 or epoch + 1 == a.epochs:
                with torch.no_grad():
                    test_loss = test.loss(downwash, w)
                st = opt.state[w]
                print("epoch:", epoch + 1, " loss:", float(loss.detach()), "test_loss: ", float(test_loss),
                      " sigma:", [round(s, 6) for s in st["sigma"].tolist()], " skipped:", int(st["info"][0]))
        stream.synchronize()
    blob = w.detach().cpu().numpy().astype("<f4")
    blob.tofile(a.out)
    print(f"wrote {a.out}: {blob.size} float32; spectral norms {train.engine.mlp_spectral_norms(blob).tolist()}")
    train.engine.close()
    test.engine.close()


if __name__ == "__main__":
    main()
