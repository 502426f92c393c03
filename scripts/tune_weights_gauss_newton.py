#!/usr/bin/env python3
"""Tunes the controller's cost weights on the CLOSED-LOOP tracking residuals of scripts/tune_weights_closed_loop.py's problem by
Levenberg-Marquardt, with the Jacobian of the whole flight in the weights from TWO forward-mode calls
(torch_layer.closed_loop_jvp with tmodel: ndp_closed_loop_jvp_model_device, at most 8 directions per call; 13 weights are tuned, Qd[6]
weighs a constant).

    python scripts/tune_weights_gauss_newton.py [--batch 256] [--ticks 20] [--iters 6] [--horizon 20] [--force 1.0]

The flight, the force on the plant and the residuals are that script's: r = (x_{k+1} - the reference at that time)[0:6] per tick and
vehicle, loss = mean |r|^2.  The weights are tuned as Qd0 exp(s), Rd0 exp(r) (positive whatever the step does; a weight that is 0 stays
0), so a column of the Jacobian in s_j is the forward-mode tangent along the direction Qd_j e_j.  Per iteration: two forward calls give
J [residuals, 13]; the step solves (J'J + lambda diag(J'J)) d = -J'r; lambda is halved after an accepted step and multiplied by 4 after
a refused one (at most 10 refusals per iteration).  Every evaluation restarts the engine from tick 0's window, so they differ in the
weights alone; a vehicle whose step fails in any evaluation of an iteration is left out of that iteration's residuals."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIXED = dict(pos_sigma=0.5, vel_sigma=1.0, quat_sigma=0.15)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--force", type=float, default=1.0, help="sigma of the force on the plant, N")
    a = ap.parse_args()
    import torch
    import ndp_nmpc_qd_amd as ndp
    from ndp_nmpc_qd_amd import synth
    from ndp_nmpc_qd_amd import torch_layer as TL
    from ndp_nmpc_qd_amd.params import nmpc_params as CP
    dev = torch.device("cuda:0")
    B, K, N, dt = a.batch, a.ticks, a.horizon, CP.ts_nmpc
    b = [synth.make_batch(B, N=N, seed=synth.SEED0 + 40, t0=k * dt, **MIXED) for k in range(K + 1)]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)      # noqa: E731
    x0, xr, ur = t(b[0]["x0"]), t(np.stack([v["xr"] for v in b[:K]])), t(np.stack([v["ur"] for v in b[:K]]))
    target = np.stack([v["xr"][:, 0, :6] for v in b[1:]])                   # [K,B,6]: the reference at the time x_{k+1} is reached
    fp = t(np.random.default_rng(7).normal(0.0, a.force, (K, B, 3)))
    eng = ndp.BatchedNMPC(B, N=N)
    w0 = np.array(list(eng.cfg.Qd) + list(eng.cfg.Rd))
    cols = [j for j in range(14) if j != 6 and w0[j] > 0]                   # the tuned entries of (Qd | Rd)
    groups = [cols[:8], cols[8:]]

    def flight(w, jac):
        """(xs [K,B,10] numpy, J [K,B,10,len(cols)] numpy or None) at the weights w [14]."""
        eng.set_model(Qd=w[:10], Rd=w[10:])
        if not jac:
            eng.reset(b[0]["xr"], b[0]["ur"])
            with torch.no_grad():
                xs = TL.closed_loop(eng, x0, xr, ur, fp=fp, dt=dt)[0]
            return xs.cpu().numpy(), None
        Js = []
        for grp in groups:
            tm = torch.zeros(len(grp), 16, dtype=torch.float64, device=dev)
            for d, j in enumerate(grp):
                tm[d, j] = w[j]                                             # d w_j / d s_j = w_j
            eng.reset(b[0]["xr"], b[0]["ur"])
            out = TL.closed_loop_jvp(eng, x0, xr, ur, (None,) * 5, fp=fp, dt=dt, tmodel=tm)
            Js.append(out[3])
        return out[0].cpu().numpy(), torch.cat(Js, dim=2).permute(0, 1, 3, 2).cpu().numpy()

    s = np.zeros(14)
    lam = 1e-2
    for it in range(a.iters):
        w = w0 * np.exp(s)
        xs, J = flight(w, True)
        ok = np.isfinite(xs).all(axis=(0, 2)) & np.isfinite(J).all(axis=(0, 2, 3))
        res = (xs[:, :, :6] - target)
        Jf = J[:, ok, :6].reshape(-1, len(cols))
        r = res[:, ok].reshape(-1)
        loss = float(r @ r) / (K * int(ok.sum()))
        JtJ, g = Jf.T @ Jf, Jf.T @ r
        for refusals in range(11):
            d = np.linalg.solve(JtJ + lam * np.diag(np.diag(JtJ)), -g)
            cand = s.copy()
            cand[cols] += d
            xs_c, _ = flight(w0 * np.exp(cand), False)
            if np.isfinite(xs_c[:, ok]).all():
                rc = (xs_c[:, ok, :6] - target[:, ok]).reshape(-1)
                new = float(rc @ rc) / (K * int(ok.sum()))
                if new < loss:
                    s, lam = cand, lam * 0.5
                    break
            lam *= 4.0
        else:
            print(f"iteration {it}: loss {loss:.6e}  no decrease within 10 refusals, stopping", flush=True)
            break
        print(f"iteration {it}: loss {loss:.6e} -> {new:.6e}  |J'r|max {np.abs(g).max():.2e}  lambda {lam:.2e}  refusals {refusals}  "
              f"vehicles {int(ok.sum())} of {B}", flush=True)
    w = w0 * np.exp(s)
    print("Qd", w[:10].tolist())
    print("Rd", w[10:].tolist())
    eng.close()


if __name__ == "__main__":
    main()
