"""The exact directional derivative of one RTI iteration's QP with a fixed active set, in plain numpy, on tests/fixed_set_ref.py: with the
set fixed the QP's solution solves K [z; nu] = [-g; e], and along a direction (tx0, txr, tur, tf) of its data
    [z'; nu'] = K^-1 (sum_theta fd_column(theta) theta' + the dx_0 rows <- tx0),
fd_column = d[-g; e]/dtheta - dK/dtheta [z; nu] (_param_columns).  The columns are exact where the data are affine in the parameter (x0, the
position / velocity rows of xr, ur, f); in the attitude reference qr the Hessian is quadratic, where central differences are exact as well --
checked, not assumed: jvp_ref forms the qr part at two step sizes and returns both."""
import numpy as np

from tests.fixed_set_ref import NU, NX, _param_columns, fd_column, fixed_of, system


def jvp_system(oracle, cfg, x0, xr, ur, f, X, U, act=None, h=0.125, pin_v=None):
    """The system and its data columns at one linearisation (the expensive part, once per instance): what jvp_apply takes."""
    extra = list(pin_v or [])
    K, nz, sol, fixed, cols, xr64, ur64, f64 = _param_columns(oracle, cfg, x0, xr, ur, f, X, U, act, extra, h)
    A = None if act is None else np.asarray(act).reshape(cfg.N, NU)

    def sysf(a):
        qp = oracle.linearize(cfg, x0, a, ur64, f64 if cfg.use_fd else None, X, U)
        return system(qp, fixed_of(qp, A) + extra)

    return dict(N=cfg.N, K=K, nz=nz, sol=sol, fixed=fixed, cols=cols, xr=xr64, sysf=sysf, h=h)


def jvp_apply(c, tx0=None, txr=None, tur=None, tf=None):
    """Returns (du0 [4], dX [N+1,10], dU [N,4], dz2) along one direction: the tangent of the QP's solution, pinned rows of dU exactly 0;
    dz2 = the same tangent (flat, z order) with the attitude-reference columns the direction uses taken at half the step."""
    N, K, nz, cols, h = c["N"], c["K"], c["nz"], c["cols"], c["h"]
    nzx = (N + 1) * NX
    tans = [np.zeros(n) if t is None else np.asarray(t, dtype=np.float64).ravel() for t, n in zip((txr, tur, tf), (nzx, N * NU, (N + 1) * 3))]

    def solve(cs):
        rhs = sum(np.stack(col, axis=1) @ t for col, t in zip(cs, tans))
        if tx0 is not None:
            rhs[nz:nz + NX] += np.asarray(tx0, dtype=np.float64)        # e[0:10] = dx_0 = x0 - X_0
        dz = np.linalg.solve(K, rhs)[:nz]
        for v, _ in c["fixed"]:                                         # exactly 0, as the device writes them
            if v >= nzx:
                dz[v] = 0.0
        return dz

    dz = solve(cols)
    dz2 = dz.copy()
    if txr is not None:
        c2 = list(cols[0])
        for j in (j for j in range(nzx) if j % NX >= 6 and tans[0][j] != 0.0):
            d = np.zeros(nzx)
            d[j] = 0.5 * h
            d = d.reshape(c["xr"].shape)
            c2[j] = fd_column(c["sysf"](c["xr"] + d), c["sysf"](c["xr"] - d), c["sol"], 0.5 * h)
        dz2 = solve([c2, cols[1], cols[2]])
    dX, dU = dz[:nzx].reshape(N + 1, NX), dz[nzx:].reshape(N, NU)
    return dU[0].copy(), dX, dU, dz2


def jvp_ref(oracle, cfg, x0, xr, ur, f, X, U, act=None, tx0=None, txr=None, tur=None, tf=None, h=0.125, pin_v=None):
    """jvp_apply at the iterate (X, U) with the pinned inputs of act (int8 [N,4] or None; pin_v: further (variable index, value) pins) held
    at their bounds."""
    return jvp_apply(jvp_system(oracle, cfg, x0, xr, ur, f, X, U, act, h, pin_v), tx0, txr, tur, tf)
