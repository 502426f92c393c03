"""What the tests of the one-call closed-loop backward (ndp_closed_loop_vjp_device) add to tests/closed_loop_chain_ref.py: the MODEL
gradient of the chained loss, composed from the references the suite already trusts, and the oracle's closed loop at another model for
the finite differences that hold the composition.

    gmodel[v] = sum_k fixed_set_ref.model_grad_ref(tick k of v; upstream gu0 = H_k + gu_p of the reverse sweep, gX = A_k)[0:15]
    gmodel[v][15] = -(1/m) sum_k <gfp_k, fp_k>                 the PLANT's mass share: the force enters the plant as fp / m only

with gu_p and gfp_k the plant link's outputs of closed_loop_chain_ref.reverse's sweep (recomputed here: `reverse` does not return them).
The same PARTIAL derivative: every tick's linearisation point and final set are held fixed, so the finite differences restart every tick
from the recorded iterate and kept set."""
import numpy as np

from tests import closed_loop_chain_ref as R
from tests import fixed_set_ref as F


def sweep_upstreams(sys_, rec, G, H, A):
    """The reverse sweep's per-tick quantities the model gradient needs: (gu0 [K,n,4] the step's upstream H_k + gu_p, gfp [K,n,3])."""
    which, K = sys_["which"], sys_["K"]
    n = len(which)
    gu0, gfp = np.zeros((K, n, 4)), np.zeros((K, n, 3))
    gx_next = np.zeros((n, 10))
    for k in reversed(range(K)):
        gx_p, gu_p, gfp[k] = R.plant_link(sys_, k, G[k][which] + gx_next)
        gu0[k] = H[k][which] + gu_p
        gx0 = R.step_link(sys_, k, gu0[k], A[k][which])[0]
        gx_next = gx_p + gx0
    return gu0, gfp


def model_reverse(oracle, sys_, rec, G, H, A, cfg=None):
    """(total [n,16], per_tick [K,n,16]): the model gradient of sum over `which` of L, one row per vehicle in the order of `which`.
    per_tick[k][:, 0:15] is model_grad_ref's of tick k (column 15 of it: that tick's plant share); total sums the ticks."""
    which, K, N = sys_["which"], sys_["K"], sys_["N"]
    cfg = oracle.default_cfg(N=N, use_fd=True) if cfg is None else cfg
    gu0, gfp = sweep_upstreams(sys_, rec, G, H, A)
    per = np.zeros((K, len(which), 16))
    for k in range(K):
        for j, v in enumerate(which):
            g, _ = F.model_grad_ref(oracle, cfg, rec["x"][k][v], rec["xr"][k][v], rec["ur"][k][v], rec["force"][k][v], rec["Xpre"][k][v],
                                    rec["Upre"][k][v], rec["act"][k][v], gu0[k][j], A[k][v], None)
            per[k, j, :15] = g[:15]
            per[k, j, 15] = -(gfp[k][j] @ rec["fp"][k][v]) / cfg.mass
    return per.sum(axis=0), per


def loss_at(oracle, cfg, rec, G, H, A, dt=R.DT, substeps=R.SUBSTEPS):
    """(L [B], stable [B]): the chained loss of the oracle's closed loop at the model of cfg (qp_mode 0, the force on), every tick
    restarted from the record's pre-step iterate and kept set; stable: every tick a set finish on the record's final set."""
    K, B = rec["xr"].shape[0], rec["x"].shape[1]
    x = rec["x"][0].copy()
    L, stable = np.zeros(B), np.ones(B, dtype=bool)
    for k in range(K):
        X, U, act = rec["Xpre"][k].copy(), rec["Upre"][k].copy(), rec["act_pre"][k].copy()
        u0, st, it, _ = oracle.step_batch_as(cfg, x, rec["xr"][k], rec["ur"][k], rec["force"][k], X, U, act)
        x = oracle.plant_step(cfg, x.copy(), u0, np.ascontiguousarray(rec["fp"][k]), dt, substeps)
        stable &= (st == 0) & ((it & 0xffff) == 0) & (act == rec["act"][k]).all(axis=(1, 2))
        L += (G[k] * x).sum(axis=1) + (H[k] * u0).sum(axis=1) + (A[k] * X).sum(axis=(1, 2))
    return L, stable


def model_fd(oracle, rec, G, H, A, col, rel=1e-5, cfg=None, dt=R.DT, substeps=R.SUBSTEPS):
    """(fd [B], stable [B]): the central difference of loss_at in model entry col (0..9 Qd, 10..13 Rd, 14: the mass -- controller AND
    plant, one handle has one mass), step rel x the entry of the model the record was made at (cfg; None: the default's)."""
    N = rec["xr"].shape[2] - 1
    base = R.twin_cfg(oracle, N, cfg)
    val = base.Qd[col] if col < 10 else base.Rd[col - 10] if col < 14 else base.mass
    h = rel * val
    out, stable = [], np.ones(rec["x"].shape[1], dtype=bool)
    for sgn in (1.0, -1.0):
        c = F.copy_cfg(base)
        if col < 10:
            c.Qd[col] = val + sgn * h
        elif col < 14:
            c.Rd[col - 10] = val + sgn * h
        else:
            c.mass = val + sgn * h
        L, ok = loss_at(oracle, c, rec, G, H, A, dt, substeps)
        out.append(L)
        stable &= ok
    return (out[0] - out[1]) / (2 * h), stable
