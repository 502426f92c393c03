"""The exact parameter sensitivity of one RTI iteration's QP with a fixed active set, in plain numpy.

The QP is the one oracle.linearize builds at (x0, xr, ur, f, X, U) -- the iterate the step started from -- with the step's final set of
pinned inputs held at their bounds.  With the set fixed the QP's solution solves K [z; nu] = [-g; e] (the system of
tests/ref_numpy.kkt_solve), so
    d[z; nu]/dtheta = K^-1 (de'/dtheta - dK/dtheta [z; nu]),   e' = [-g; e],
which is [-(dg/dtheta + dH/dtheta z*) ; db/dtheta] in the rows that move.  The data derivatives are central differences of oracle.linearize:
the data are at most quadratic in every parameter (the attitude weight E(qr)' W E(qr)), so the differences are exact to rounding.  The force is differenced with the
disturbance on (use_fd): it enters the defects additively, so the derivative is the same at any force, and at f = 0 without it.
"""
import ctypes as C

import numpy as np

NX, NU = 10, 4


def _with_fd(cfg):
    c = type(cfg)()
    C.memmove(C.addressof(c), C.addressof(cfg), C.sizeof(cfg))
    c.use_fd = 1
    return c


def fixed_of(qp, act):
    """kkt_solve's pins for a set act (int8 [N,4]: +1 upper, -1 lower, 0 free): the step bounds of linearize."""
    if act is None:
        return []
    N = qp["A"].shape[0]
    return [((N + 1) * NX + NU * k + i, float(qp["uu"][k, i] if act[k, i] > 0 else qp["lu"][k, i]))
            for k, i in zip(*np.nonzero(np.asarray(act).reshape(N, NU)))]


def _system(qp, fixed):
    """kkt_solve's dense system K [z; nu] = [-g; e] (variables dx_0..dx_N, du_0..du_{N-1}; rows x0, dynamics, pins)."""
    A, B, b, Q, q, Rd, r, dx0 = (np.asarray(qp[k], dtype=np.float64) for k in ("A", "B", "b", "Q", "q", "Rd", "r", "dx0"))
    N = A.shape[0]
    nz = (N + 1) * NX + N * NU
    uo = (N + 1) * NX
    H = np.zeros((nz, nz))
    for k in range(N + 1):
        H[k * NX:(k + 1) * NX, k * NX:(k + 1) * NX] = Q[k]
    for k in range(N):
        H[uo + k * NU:uo + (k + 1) * NU, uo + k * NU:uo + (k + 1) * NU] = np.diag(Rd[k])
    ne = (N + 1) * NX + len(fixed)
    E = np.zeros((ne, nz))
    e = np.zeros(ne)
    E[0:NX, 0:NX] = np.eye(NX)
    e[0:NX] = dx0
    for k in range(N):
        rows = slice((k + 1) * NX, (k + 2) * NX)
        E[rows, (k + 1) * NX:(k + 2) * NX] = np.eye(NX)
        E[rows, k * NX:(k + 1) * NX] = -A[k]
        E[rows, uo + k * NU:uo + (k + 1) * NU] = -B[k]
        e[rows] = b[k]
    for i, (v, val) in enumerate(fixed):
        E[(N + 1) * NX + i, v] = 1.0
        e[(N + 1) * NX + i] = val
    K = np.block([[H, E.T], [E, np.zeros((ne, ne))]])
    return K, np.concatenate([-np.concatenate([q.ravel(), r.ravel()]), e]), nz


def psens_ref(oracle, cfg, x0, xr, ur, f, X, U, act=None, h=0.125):
    """Returns (dxr [4,N+1,10], dur [4,N,4], df [4,N+1,3]): row i = d u0[i] / d(parameter) of the QP oracle.linearize builds at the
    iterate (X, U), the pinned inputs of act (int8 [N,4] or None) held at their bounds.  K sol = rhs differentiated: K dsol = drhs - dK sol,
    dK and drhs by central differences (every term of dK is dH: the dynamics do not see the parameters -- included all the same)."""
    N = cfg.N
    xr, ur = np.asarray(xr, dtype=np.float64), np.asarray(ur, dtype=np.float64)
    f = np.zeros((N + 1, 3)) if f is None else np.asarray(f, dtype=np.float64)
    cfd = _with_fd(cfg)
    lin = lambda c, a, b_, ff: oracle.linearize(c, x0, a, b_, ff if c.use_fd else None, X, U)  # noqa: E731
    qp = lin(cfg, xr, ur, f)
    fixed = fixed_of(qp, None if act is None else np.asarray(act).reshape(N, NU))
    K, rhs0, nz = _system(qp, fixed)
    sol = np.linalg.solve(K, rhs0)
    cols = []
    for which, base, shape in (("xr", xr, (N + 1, NX)), ("ur", ur, (N, NU)), ("f", f, (N + 1, 3))):
        for j in range(base.size):
            d = np.zeros(base.size)
            d[j] = h
            sy = []
            for sg in (1.0, -1.0):
                pa = base + sg * d.reshape(shape)
                q2 = lin(cfg, pa, ur, f) if which == "xr" else lin(cfg, xr, pa, f) if which == "ur" else lin(cfd, xr, ur, pa)
                sy.append(_system(q2, fixed_of(q2, None if act is None else np.asarray(act).reshape(N, NU)))[:2])
            (Ka, ra), (Kb, rb) = sy
            cols.append(((ra - rb) - (Ka - Kb) @ sol) / (2 * h))
    dz = np.linalg.solve(K, np.stack(cols, axis=1))[:nz]
    du0 = dz[(N + 1) * NX:(N + 1) * NX + NU]            # [4, n_params]
    n1, n2 = (N + 1) * NX, N * NU
    for v, _ in fixed:                                  # exactly 0, as the device writes them
        if v < (N + 1) * NX + NU:
            du0[v - (N + 1) * NX] = 0.0
    return (du0[:, :n1].reshape(NU, N + 1, NX).copy(), du0[:, n1:n1 + n2].reshape(NU, N, NU).copy(),
            du0[:, n1 + n2:].reshape(NU, N + 1, 3).copy())


def scale(J):
    """The bar's scale: max(1, |J|max)."""
    return max(1.0, float(np.max(np.abs(J))))
