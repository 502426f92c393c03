"""The exact adjoint (vector-Jacobian product) of one RTI iteration's QP with a fixed active set, in plain numpy.

The QP is psens_ref's: the one oracle.linearize builds at (x0, xr, ur, f, X, U) -- the iterate the step started from -- with the step's
final set of pinned inputs held at their bounds, so that its solution solves K [z; nu] = [-g; e].  For a loss L with gradient gz on the
step variables z = (dx_0..dx_N, du_0..du_{N-1}) -- the new iterate is the old one plus z -- the adjoint [v; mu] solves K' [v; mu] = [gz; 0] and
    dL/dtheta = [v; mu]' (de'/dtheta - dK/dtheta [z; nu]),   e' = [-g; e],
with the data derivatives by central differences of oracle.linearize (exact to rounding: see psens_ref).  dL/dx0 is the multiplier of the
initial-state rows (e[0:10] = x0 - X_0).
"""
import numpy as np

from tests.psens_ref import NU, NX, _system, _with_fd, fixed_of


def upstream(N, gu0=None, gX=None, gU=None):
    """gz on (dx_0..dx_N, du_0..du_{N-1}); gu0 adds to du_0."""
    gz = np.zeros((N + 1) * NX + N * NU)
    if gX is not None:
        gz[:(N + 1) * NX] = np.asarray(gX, dtype=np.float64).ravel()
    if gU is not None:
        gz[(N + 1) * NX:] = np.asarray(gU, dtype=np.float64).ravel()
    if gu0 is not None:
        gz[(N + 1) * NX:(N + 1) * NX + NU] += np.asarray(gu0, dtype=np.float64)
    return gz


def vjp_ref(oracle, cfg, x0, xr, ur, f, X, U, act=None, gu0=None, gX=None, gU=None, h=0.125):
    """Returns (gx0 [10], gxr [N+1,10], gur [N,4], gf [N+1,3]) of L = gz' z* for the QP at the iterate (X, U) with the pinned inputs of act
    (int8 [N,4] or None) held at their bounds.  The force is differenced with the disturbance on, as psens_ref does."""
    N = cfg.N
    xr, ur = np.asarray(xr, dtype=np.float64), np.asarray(ur, dtype=np.float64)
    f = np.zeros((N + 1, 3)) if f is None else np.asarray(f, dtype=np.float64)
    A = None if act is None else np.asarray(act).reshape(N, NU)
    cfd = _with_fd(cfg)
    lin = lambda c, a, b_, ff: oracle.linearize(c, x0, a, b_, ff if c.use_fd else None, X, U)  # noqa: E731
    qp = lin(cfg, xr, ur, f)
    K, rhs0, nz = _system(qp, fixed_of(qp, A))
    sol = np.linalg.solve(K, rhs0)
    adj = np.linalg.solve(K.T, np.concatenate([upstream(N, gu0, gX, gU), np.zeros(K.shape[0] - nz)]))
    out = []
    for which, base, shape in (("xr", xr, (N + 1, NX)), ("ur", ur, (N, NU)), ("f", f, (N + 1, 3))):
        g = np.zeros(base.size)
        for j in range(base.size):
            d = np.zeros(base.size)
            d[j] = h
            sy = []
            for sg in (1.0, -1.0):
                pa = base + sg * d.reshape(shape)
                q2 = lin(cfg, pa, ur, f) if which == "xr" else lin(cfg, xr, pa, f) if which == "ur" else lin(cfd, xr, ur, pa)
                sy.append(_system(q2, fixed_of(q2, A))[:2])
            (Ka, ra), (Kb, rb) = sy
            g[j] = adj @ (((ra - rb) - (Ka - Kb) @ sol) / (2 * h))
        out.append(g.reshape(shape))
    gxr, gur, gf = out
    if A is not None:                                   # exactly 0, as the device writes them
        gur[A != 0] = 0.0
    return adj[nz:nz + NX].copy(), gxr, gur, gf
