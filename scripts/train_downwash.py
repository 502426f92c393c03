#!/usr/bin/env python3
"""The reference's training loop (nn_train.py:129-157) on this library: MSE on flat sample rows, Adam, the spectral-norm cap after every
step -- full batch as the reference, or mini-batches.

    python scripts/train_downwash.py [--input downwash_input.csv --output downwash_output.csv] [--sn 4] [--epochs 10000]
                                     [--batch-size 0] [--out FILE.bin]

The data set lives on the device as the reference holds it (nn_train.py:99-108): x [n,6] and y [n,3] in float32.  Every step is two
enqueues on one stream -- ONE fused call for the forward, the loss and the weight gradient (torch_layer.downwash_fit_rows,
ndp_mlp_fit_rows_device) and ONE launch for Adam and the cap (torch_layer.DownwashAdamSN, ndp_mlp_adam_sn_device) -- and no value comes
back to the host except the losses printed after the first epoch, every 1000 epochs and at the end.  One small engine serves training and evaluation: its batch shape plays no
part.  The result is written as a blob file (17 859 float32, the order of ndp_set_mlp_weights), with the four spectral norms printed beside
it.

--batch-size M (0: full batch, the reference's): every epoch draws a torch.randperm on the device and walks it in index lists of M rows;
the last list is padded with -1 (empty slots) and every step uses scale = 1 / (3 M_real), so each step's loss is nn.MSELoss over its own
rows.  Nothing is pulled to the host between steps.

Data.  --input / --output: CSV files with the reference's column names (x, y, z, vx, vy, vz and fx, fy, fz), read with numpy; split 75 / 25
by a seeded permutation (the reference uses sklearn's split with random_state 42: the same proportions, not the same rows).  Without them:
--samples rows drawn uniformly in the training envelope (|dx|, |dy|, |dz| <= 1.5 m, |dv| <= 3 m/s) and labelled by the SHIPPED network.
That is a plumbing demonstration: the data are made by a network of the very architecture that is fitted, so it shows that the loop runs,
that the loss goes down and that the cap holds -- it says nothing about real downwash, and a fit to it is not a replacement for
downwash_sn4.bin.

Not the reference's: the start is nn.Linear's default initialisation drawn with numpy's generator, not torch's.  (The reference's network
has no dropout in either path: the Dropout layers of nn_net.py:10,13,16 are commented out, so its net.train() changes nothing; with --sn 0
this loop is plain Adam, as the reference's --SN 0 path is.)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input", help="CSV with columns x, y, z, vx, vy, vz")
    ap.add_argument("--output", help="CSV with columns fx, fy, fz")
    ap.add_argument("--sn", type=float, default=0.0, help="max spectral norm of a single layer (0: no cap)")
    ap.add_argument("--epochs", type=int, default=10000)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--batch-size", type=int, default=0, help="rows per optimiser step (0: the full training set, the reference's)")
    ap.add_argument("--samples", type=int, default=8192, help="synthetic rows when no CSV is given")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default="downwash_trained.bin")
    a = ap.parse_args()
    if (a.input is None) != (a.output is None):
        raise SystemExit("--input and --output go together")
    if a.batch_size < 0:
        raise SystemExit("--batch-size must be 0 (full batch) or positive")
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import _lib
    from ndp_nmpc_qd_amd.torch_layer import DownwashAdamSN, downwash_fit_rows, downwash_rows
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    torch.manual_seed(a.seed)
    engine = ndp.BatchedNMPC(1, N=20, disturbance=True)          # any shape serves: the row calls do not use it
    if a.input:
        x, y = read_csv(a.input, ("x", "y", "z", "vx", "vy", "vz")), read_csv(a.output, ("fx", "fy", "fz"))
        if x.shape[0] != y.shape[0]:
            raise SystemExit(f"{a.input} has {x.shape[0]} rows, {a.output} {y.shape[0]}")
        what = f"{x.shape[0]} rows of {a.input}"
    else:
        x = np.concatenate([rng.uniform(-1.5, 1.5, (a.samples, 3)), rng.uniform(-3.0, 3.0, (a.samples, 3))], axis=1)
        f = downwash_rows(engine, torch.from_numpy(x.astype(np.float32)).to(dev), weights=torch.from_numpy(_lib.load_weights()).to(dev))
        y = f.cpu().numpy()
        what = f"{a.samples} synthetic rows labelled by the shipped network (a plumbing demonstration, not downwash data)"
    perm = rng.permutation(x.shape[0])
    n_train = int(0.75 * x.shape[0])
    to_dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)  # noqa: E731    (nn_train.py:106-108)
    x_train, y_train = to_dev(x[perm[:n_train]]), to_dev(y[perm[:n_train]])
    x_test, y_test = to_dev(x[perm[n_train:]]), to_dev(y[perm[n_train:]])
    M = a.batch_size if 0 < a.batch_size < n_train else 0
    steps = (n_train + M - 1) // M if M else 1
    print(f"data: {what}; {n_train} train / {x.shape[0] - n_train} test rows; sn = {a.sn}, lr = {a.lr}, "
          + (f"mini-batches of {M} ({steps} steps per epoch)" if M else "full batch"))
    w = torch.nn.Parameter(torch.from_numpy(linear_init(rng)).to(dev))
    opt = DownwashAdamSN(w, engine, lr=a.lr, sn=a.sn)
    pad = torch.full((steps * M - n_train,), -1, dtype=torch.int32, device=dev) if M else None
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for epoch in range(a.epochs):
            if M:
                lists = torch.cat([torch.randperm(n_train, device=dev).to(torch.int32), pad]).reshape(steps, M)
            for k in range(steps):
                opt.zero_grad()
                if M:
                    real = M if k + 1 < steps else n_train - (steps - 1) * M
                    loss = downwash_fit_rows(engine, x_train, y_train, w, index=lists[k], scale=1.0 / (3.0 * real))
                else:
                    loss = downwash_fit_rows(engine, x_train, y_train, w)
                loss.backward()
                opt.step()
            if epoch == 0 or (epoch + 1) % 1000 == 0 or epoch + 1 == a.epochs:
                with torch.no_grad():
                    train_loss = downwash_fit_rows(engine, x_train, y_train, w.detach())
                    test_loss = downwash_fit_rows(engine, x_test, y_test, w.detach())
                st = opt.state[w]
                print("epoch:", epoch + 1, " loss:", float(train_loss), "test_loss: ", float(test_loss),
                      " sigma:", [round(s, 6) for s in st["sigma"].tolist()], " skipped:", int(st["info"][0]))
        stream.synchronize()
    blob = w.detach().cpu().numpy().astype("<f4")
    blob.tofile(a.out)
    print(f"wrote {a.out}: {blob.size} float32; spectral norms {engine.mlp_spectral_norms(blob).tolist()}")
    engine.close()


if __name__ == "__main__":
    main()
