"""The float64 references of forward mode along directions of the cost weights and the mass (ndp_step_jvp_model_device,
ndp_closed_loop_jvp_model_device), in plain numpy on top of tests/fixed_set_ref.py and tests/closed_loop_chain_ref.py.

A direction theta' [16] = q' [0:10] | r' [10:14] | m' [14] (the controller's mass) | m'_p [15] (the plant's mass; the step does not read it).

Step: on fixed_set_ref.jvp_system's K and solution the model columns are made exactly as fixed_set_ref.model_grad_ref makes them --
fd_column on two _perturbed configurations; the system is linear in Qd and Rd and affine in 1 / m, so the central difference is exact to
rounding; the mass column is the one in 1 / m times -1 / m^2.  The tangent is K^-1 sum_j theta'_j col_j, pinned input rows exactly 0; it
adds to jvp_apply's tangent along the data (the QP's solution map is differentiated, so the tangent is linear in the whole direction).

Closed loop: closed_loop_chain_ref.forward's recursion with that source term added at every tick (the direction is constant over the
ticks) and t_fp - theta'_15 / m fp_k in the plant link: the plant sees the mass only as fp / m.

tests/test_step_model_jvp.py holds both on the CPU: against central differences of the oracle's step in the model and, by duality, against
model_grad_ref and closed_loop_vjp_ref.model_reverse."""
import numpy as np

from tests import closed_loop_chain_ref as R
from tests import fixed_set_ref as F
from tests import plant_deriv_ref as P

NX, NU = F.NX, F.NU


def model_system(oracle, cfg, x0, xr, ur, f, X, U, act=None, h=0.125, pin_v=None, c=None):
    """fixed_set_ref.jvp_system's dict (c: one made already for these arguments) with the model columns beside the data's: "mcols" [16]
    (entry j: fd_column of model entry j, the mass chained through 1 / m; entry 15: zeros) and "mcol_m2", the mass column from half the
    step in 1 / m (the check that the mass enters through 1 / m alone)."""
    c = F.jvp_system(oracle, cfg, x0, xr, ur, f, X, U, act, h, pin_v) if c is None else c
    A = c["act"]
    ff = None if (f is None or not cfg.use_fd) else np.asarray(f, dtype=np.float64)
    extra = list(pin_v or [])

    def sysf(cc):
        qp = oracle.linearize(cc, x0, xr, ur, ff, X, U)
        return F.system(qp, F.fixed_of(qp, A) + extra)

    def col(j, step):
        return F.fd_column(sysf(F._perturbed(cfg, j, step)), sysf(F._perturbed(cfg, j, -step)), c["sol"], step)

    cols = []
    for j in range(14):
        w = cfg.Qd[j] if j < 10 else cfg.Rd[j - 10]
        cols.append(col(j, h * w if w > 0 else h))      # (a step relative to the weight: Rd stays positive)
    u = 1.0 / cfg.mass
    cols.append(col(14, h * u) * (-u * u))
    cols.append(np.zeros_like(cols[0]))
    c["mcols"] = cols
    c["mcol_m2"] = col(14, 0.5 * h * u) * (-u * u)
    return c


def model_jvp_apply(c, tmodel, tx0=None, txr=None, tur=None, tf=None):
    """(du0 [4], dX [N+1,10], dU [N,4]) along one direction: theta' = tmodel [16] of the model plus the data's (None = 0)."""
    N, K, nz = c["N"], c["K"], c["nz"]
    nzx = (N + 1) * NX
    th = np.asarray(tmodel, dtype=np.float64)
    dz = np.linalg.solve(K, np.stack(c["mcols"][:15], axis=1) @ th[:15])[:nz]
    for v, _ in c["fixed"]:                             # exactly 0, as the device writes them
        if v >= nzx:
            dz[v] = 0.0
    dX, dU = dz[:nzx].reshape(N + 1, NX).copy(), dz[nzx:].reshape(N, NU).copy()
    if not (tx0 is None and txr is None and tur is None and tf is None):
        _, aX, aU, _ = F.jvp_apply(c, tx0, txr, tur, tf)
        dX, dU = dX + aX, dU + aU
    return dU[0].copy(), dX, dU


def model_jvp_ref(oracle, cfg, x0, xr, ur, f, X, U, act, tmodel, tx0=None, txr=None, tur=None, tf=None, h=0.125, pin_v=None):
    """model_jvp_apply at the iterate (X, U) with the pinned inputs of act held at their bounds."""
    return model_jvp_apply(model_system(oracle, cfg, x0, xr, ur, f, X, U, act, h, pin_v), tmodel, tx0, txr, tur, tf)


def loop_model_systems(oracle, sys_, rec, cfg):
    """closed_loop_chain_ref.systems' dict with every (tick, vehicle) system's model columns added (model_system on the dict it holds)."""
    for k in range(sys_["K"]):
        for j, v in enumerate(sys_["which"]):
            model_system(oracle, cfg, rec["x"][k][v], rec["xr"][k][v], rec["ur"][k][v], rec["force"][k][v], rec["Xpre"][k][v],
                         rec["Upre"][k][v], rec["act"][k][v], c=sys_["S"][k][j])
    sys_["mass"] = cfg.mass
    return sys_


def loop_forward(sys_, rec, t_model, t_x0=None, t_xr=None, t_ur=None, t_fp=None, t_f=None):
    """closed_loop_chain_ref.forward's sweep (ext form) with the model direction t_model [B,T,16], constant over the ticks, beside the
    leaves' (full-batch arrays as `forward` takes them; None = 0).  sys_: loop_model_systems'.  Returns (dx [K,n,T,10] of x_{k+1},
    du0 [K,n,T,4], dX [K,n,T,N+1,10]); rows in the order of `which`."""
    which, K, N = sys_["which"], sys_["K"], sys_["N"]
    n, T = len(which), t_model.shape[1]
    tx = np.zeros((n, T, 10)) if t_x0 is None else np.array(t_x0[which], dtype=np.float64)
    dx, du0, dX = np.zeros((K, n, T, 10)), np.zeros((K, n, T, 4)), np.zeros((K, n, T, N + 1, 10))
    for k in range(K):
        for j, c in enumerate(sys_["S"][k]):
            v = which[j]
            for t in range(T):
                du0[k, j, t], dX[k, j, t], _ = model_jvp_apply(c, t_model[v, t], tx[j, t], None if t_xr is None else t_xr[k][v, t],
                                                               None if t_ur is None else t_ur[k][v, t], None if t_f is None else t_f[k][v, t])
        tfp = np.zeros((n, T, 3)) if t_fp is None else np.array(t_fp[k][which], dtype=np.float64)
        tfp = tfp - t_model[which][:, :, 15:16] / sys_["mass"] * rec["fp"][k][which][:, None, :]
        dx[k] = P.jvp(sys_["J"][k], tx0=tx, tu=du0[k][None], tf=tfp[None])[0]
        tx = dx[k]
    return dx, du0, dX
