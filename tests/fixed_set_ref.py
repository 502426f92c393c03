"""The exact derivatives of one RTI iteration's QP with a fixed active set, in plain numpy: sens_ref (du/dx0), psens_ref (du0/d(xr, ur, f)),
vjp_ref (the adjoint over (u0, X, U)), model_grad_ref (the gradient in Qd, Rd and the mass) and jvp_ref (the directional derivative).

The QP is the one oracle.linearize builds at (x0, xr, ur, f, X, U) -- the iterate the step started from (pinned to tests/ref_numpy.py) --
with the step's final set of pinned inputs held at their bounds.  With the set fixed its solution solves K [z; nu] = [-g; e] (`system`, the
system of tests/ref_numpy.kkt_solve; z = (dx_0..dx_N, du_0..du_{N-1}), the new iterate is the old one plus z), so
    d[z; nu]/dtheta = K^-1 (de'/dtheta - dK/dtheta [z; nu]),   e' = [-g; e],
and for a loss L with gradient gz on z the adjoint [v; mu] solves K' [v; mu] = [gz; 0] and
    dL/dtheta = [v; mu]' (de'/dtheta - dK/dtheta [z; nu]).
The bracket is a central difference of oracle.linearize, exact to rounding at any step where the data are at most quadratic in the
parameter: `fd_column` on two dense systems for the sixteen model entries (model_grad_ref), and for the many entries of xr, ur and f
(vjp_ref, psens_ref, jvp_ref: _param_columns) `fd_times`, the same difference on two block products K [z; nu] that never form K
(`system_times`; tests/test_deriv_edges.py holds it to the dense product).  jvp_apply keeps the half-step attitude columns it forms in
the dict jvp_system returned, so the directions of one system share them.  Exactness holds for xr, ur and f (the attitude weight E(qr)' W E(qr) is quadratic; every term of dK is dH: the dynamics do not
see them -- included all the same) and for Qd and Rd (linear).  The force is differenced with the disturbance on (use_fd): it enters the
defects additively, so the derivative is the same at any force, and at f = 0 without it.  In the mass the system is not polynomial (the
force enters as f / m), but it is affine in u = 1 / m: the mass is differenced in u (cfg.mass = 1 / (u +- du)), exact to rounding as well
if the mass enters through 1 / m alone, and chained with du/dm = -1 / m^2.  That "if" is checked, not assumed: model_grad_ref returns the
mass entry for two step sizes, and the tests assert that they agree to 1e-9.
In x0 the solution is affine, and the derivative is the solution of the HOMOGENEOUS problem (b = q = r = 0, the pinned inputs held at 0)
with dx_0 = e_j: the same K, factored once for all ten right-hand sides.  dL/dx0 is the multiplier of the initial-state rows
(e[0:10] = x0 - X_0).
Forward mode: along a direction (tx0, txr, tur, tf) of the data
    [z'; nu'] = K^-1 (sum_theta fd_column(theta) theta' + the dx_0 rows <- tx0)
over the same columns (_param_columns).  They are exact where the data are affine in the parameter (x0, the position / velocity rows of xr,
ur, f); in the attitude reference qr the Hessian is quadratic, where central differences are exact as well -- checked, not assumed: jvp_ref
forms the qr part at two step sizes and returns both.
"""
import ctypes as C

import numpy as np

NX, NU = 10, 4


def copy_cfg(cfg):
    c = type(cfg)()
    C.memmove(C.addressof(c), C.addressof(cfg), C.sizeof(cfg))
    return c


def fixed_of(qp, act):
    """kkt_solve's pins for a set act (int8 [N,4]: +1 upper, -1 lower, 0 free): the step bounds of linearize."""
    if act is None:
        return []
    N = qp["A"].shape[0]
    return [((N + 1) * NX + NU * k + i, float(qp["uu"][k, i] if act[k, i] > 0 else qp["lu"][k, i]))
            for k, i in zip(*np.nonzero(np.asarray(act).reshape(N, NU)))]


def system(qp, fixed):
    """kkt_solve's dense system K [z; nu] = [-g; e] (variables dx_0..dx_N, du_0..du_{N-1}; rows x0, dynamics, pins).  Returns (K, rhs, nz)."""
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


def scale(J):
    """The bar's scale: max(1, |J|max)."""
    return max(1.0, float(np.max(np.abs(J))))


def fd_column(sa, sb, sol, step):
    """d rhs - dK sol by central differences: sa, sb = system() of the data at theta + step and theta - step."""
    (Ka, ra), (Kb, rb) = sa[:2], sb[:2]
    return ((ra - rb) - (Ka - Kb) @ sol) / (2 * step)


def system_times(qp, fixed, sol):
    """(K sol, rhs) of system(qp, fixed) without forming K: the stage blocks applied one by one.  What the data columns difference (two
    of these per parameter entry; tests/test_deriv_edges.py holds it to system()'s dense product)."""
    A, B, b, Q, q, Rd, r, dx0 = (np.asarray(qp[k], dtype=np.float64) for k in ("A", "B", "b", "Q", "q", "Rd", "r", "dx0"))
    N = A.shape[0]
    nzx = (N + 1) * NX
    nz = nzx + N * NU
    dx, du, nu, npin = sol[:nzx].reshape(N + 1, NX), sol[nzx:nz].reshape(N, NU), sol[nz:nz + nzx].reshape(N + 1, NX), sol[nz + nzx:]
    tx = np.einsum("kij,kj->ki", Q, dx) + nu                         # H z + E' nu, state rows
    tx[:N] -= np.einsum("kji,kj->ki", A, nu[1:])
    top = np.concatenate([tx.ravel(), (Rd * du - np.einsum("kji,kj->ki", B, nu[1:])).ravel()])
    bx = dx.copy()                                                   # E z
    bx[1:] -= np.einsum("kij,kj->ki", A, dx[:-1]) + np.einsum("kij,kj->ki", B, du)
    z = sol[:nz]
    for i, (v, _) in enumerate(fixed):
        top[v] += npin[i]
    out = np.concatenate([top, bx.ravel(), np.array([z[v] for v, _ in fixed])])
    rhs = np.concatenate([-q.ravel(), -r.ravel(), dx0, b.ravel(), np.array([val for _, val in fixed])])
    return out, rhs


def fd_times(pa, pb, step):
    """fd_column from two system_times results."""
    return ((pa[1] - pb[1]) - (pa[0] - pb[0])) / (2 * step)


def _adjoint(K, nz, N, gu0, gX, gU):
    return np.linalg.solve(K.T, np.concatenate([upstream(N, gu0, gX, gU), np.zeros(K.shape[0] - nz)]))


def _param_columns(oracle, cfg, x0, xr, ur, f, X, U, act, extra, h):
    """The system at (xr, ur, f) with the pins of act (and `extra`, a list of (variable index, value)), its solution, and fd_column for every
    entry of xr, ur and f: (K, nz, sol, fixed, [cols_xr, cols_ur, cols_f], xr, ur, f as float64 arrays)."""
    N = cfg.N
    xr, ur = np.asarray(xr, dtype=np.float64), np.asarray(ur, dtype=np.float64)
    f = np.zeros((N + 1, 3)) if f is None else np.asarray(f, dtype=np.float64)
    A = None if act is None else np.asarray(act).reshape(N, NU)
    cfd = copy_cfg(cfg)
    cfd.use_fd = 1

    def sysf(c, a, b_, ff):
        qp = oracle.linearize(c, x0, a, b_, ff if c.use_fd else None, X, U)
        fixed = fixed_of(qp, A) + extra
        return system(qp, fixed) + (fixed,)

    K, rhs0, nz, fixed = sysf(cfg, xr, ur, f)
    sol = np.linalg.solve(K, rhs0)

    def times(c, a, b_, ff):
        qp = oracle.linearize(c, x0, a, b_, ff if c.use_fd else None, X, U)
        return system_times(qp, fixed_of(qp, A) + extra, sol)

    cols = []
    for which, base in (("xr", xr), ("ur", ur), ("f", f)):
        cols.append([])
        for j in range(base.size):
            d = np.zeros(base.size)
            d[j] = h
            sa, sb = (times(cfg, pa, ur, f) if which == "xr" else times(cfg, xr, pa, f) if which == "ur" else times(cfd, xr, ur, pa)
                      for pa in (base + d.reshape(base.shape), base - d.reshape(base.shape)))
            cols[-1].append(fd_times(sa, sb, h))
    return K, nz, sol, fixed, cols, xr, ur, f


def sens_ref(qp, act=None):
    """qp: dict of oracle.linearize; act: int8 [N,4] (nonzero = the input is pinned on a bound), or None.
    Returns (du0 [4,10], dU [N,4,10], dX [N+1,10,10]): column j is the derivative with respect to x0[j]."""
    N = qp["A"].shape[0]
    uo = (N + 1) * NX
    pins = [] if act is None else [uo + k * NU + i for k, i in zip(*np.nonzero(np.asarray(act).reshape(N, NU)))]
    hom = dict(qp, **{k: np.zeros_like(np.asarray(qp[k], dtype=np.float64)) for k in ("b", "q", "r", "dx0")})
    K, _, nz = system(hom, [(v, 0.0) for v in pins])
    rhs = np.zeros((K.shape[0], NX))
    rhs[nz:nz + NX, :] = np.eye(NX)
    Z = np.linalg.solve(K, rhs)[:nz]
    dX = Z[:uo].reshape(N + 1, NX, NX)
    dU = Z[uo:].reshape(N, NU, NX)
    dX[0] = np.eye(NX)                  # (the initial-state rows, exact)
    for v in pins:                      # exactly 0, as the device writes them
        k, i = divmod(v - uo, NU)
        dU[k, i, :] = 0.0
    return dU[0].copy(), dU, dX


def psens_apply(c):
    """psens_ref from jvp_system's dict (one set of data columns serves every derivative of one linearisation)."""
    N, K, nz, cols, fixed = c["N"], c["K"], c["nz"], c["cols"], c["fixed"]
    dz = np.linalg.solve(K, np.stack(cols[0] + cols[1] + cols[2], axis=1))[:nz]
    du0 = dz[(N + 1) * NX:(N + 1) * NX + NU]            # [4, n_params]
    n1, n2 = (N + 1) * NX, N * NU
    for v, _ in fixed:                                  # exactly 0, as the device writes them
        if (N + 1) * NX <= v < (N + 1) * NX + NU:
            du0[v - (N + 1) * NX] = 0.0
    return (du0[:, :n1].reshape(NU, N + 1, NX).copy(), du0[:, n1:n1 + n2].reshape(NU, N, NU).copy(),
            du0[:, n1 + n2:].reshape(NU, N + 1, 3).copy())


def psens_ref(oracle, cfg, x0, xr, ur, f, X, U, act=None, h=0.125):
    """Returns (dxr [4,N+1,10], dur [4,N,4], df [4,N+1,3]): row i = d u0[i] / d(parameter) of the QP oracle.linearize builds at the
    iterate (X, U), the pinned inputs of act (int8 [N,4] or None) held at their bounds."""
    return psens_apply(jvp_system(oracle, cfg, x0, xr, ur, f, X, U, act, h))


def vjp_apply(c, gu0=None, gX=None, gU=None):
    """vjp_ref from jvp_system's dict."""
    N, K, nz, cols = c["N"], c["K"], c["nz"], c["cols"]
    adj = _adjoint(K, nz, N, gu0, gX, gU)
    gxr, gur, gf = (np.array([adj @ col for col in cs]).reshape(base.shape) for cs, base in zip(cols, (c["xr"], c["ur"], c["f"])))
    if c["act"] is not None:                            # exactly 0, as the device writes them
        gur[c["act"] != 0] = 0.0
    return adj[nz:nz + NX].copy(), gxr, gur, gf


def vjp_ref(oracle, cfg, x0, xr, ur, f, X, U, act=None, gu0=None, gX=None, gU=None, h=0.125, pin_v=None):
    """Returns (gx0 [10], gxr [N+1,10], gur [N,4], gf [N+1,3]) of L = gz' z* for the QP at the iterate (X, U) with the pinned inputs of act
    (int8 [N,4] or None) held at their bounds.  pin_v: optional list of (variable index, value) pins added to act's (the interior-point
    comparison pins the active velocity bounds too)."""
    return vjp_apply(jvp_system(oracle, cfg, x0, xr, ur, f, X, U, act, h, pin_v), gu0, gX, gU)


def _perturbed(cfg, j, d):
    """cfg with model entry j (0..9 Qd, 10..13 Rd, 14: 1 / mass) moved by d."""
    c = copy_cfg(cfg)
    if j < 10:
        c.Qd[j] += d
    elif j < 14:
        c.Rd[j - 10] += d
    else:
        c.mass = 1.0 / (1.0 / cfg.mass + d)
    return c


def model_grad_ref(oracle, cfg, x0, xr, ur, f, X, U, act=None, gu0=None, gX=None, gU=None, h=0.125, pin_v=None):
    """Returns (g [16], gm2): g[0:10] = dL/dQd, g[10:14] = dL/dRd, g[14] = dL/dmass, g[15] = 0 of L = gz' z* for the QP at the iterate
    (X, U) with the pinned inputs of act (int8 [N,4] or None) held at their bounds; gm2 = dL/dmass from half the step in 1 / m.
    pin_v: as vjp_ref's."""
    N = cfg.N
    A = None if act is None else np.asarray(act).reshape(N, NU)
    ff = None if (f is None or not cfg.use_fd) else np.asarray(f, dtype=np.float64)
    extra = list(pin_v or [])

    def sysf(c):
        qp = oracle.linearize(c, x0, xr, ur, ff, X, U)
        return system(qp, fixed_of(qp, A) + extra)

    K, rhs0, nz = sysf(cfg)
    sol = np.linalg.solve(K, rhs0)
    adj = _adjoint(K, nz, N, gu0, gX, gU)

    def d(j, step):
        return adj @ fd_column(sysf(_perturbed(cfg, j, step)), sysf(_perturbed(cfg, j, -step)), sol, step)

    g = np.zeros(16)
    for j in range(14):
        w = cfg.Qd[j] if j < 10 else cfg.Rd[j - 10]
        g[j] = d(j, h * w if w > 0 else h)              # (a step relative to the weight: Rd stays positive)
    u = 1.0 / cfg.mass
    dm = -u * u
    g[14] = d(14, h * u) * dm                           # (without a force: 0 -- gravity and the thrust do not see the mass)
    return g, d(14, 0.5 * h * u) * dm


def jvp_system(oracle, cfg, x0, xr, ur, f, X, U, act=None, h=0.125, pin_v=None):
    """The system and its data columns at one linearisation (the expensive part, once per instance): what jvp_apply takes."""
    extra = list(pin_v or [])
    K, nz, sol, fixed, cols, xr64, ur64, f64 = _param_columns(oracle, cfg, x0, xr, ur, f, X, U, act, extra, h)
    A = None if act is None else np.asarray(act).reshape(cfg.N, NU)

    def sysf(a):
        qp = oracle.linearize(cfg, x0, a, ur64, f64 if cfg.use_fd else None, X, U)
        return system_times(qp, fixed_of(qp, A) + extra, sol)

    return dict(N=cfg.N, K=K, nz=nz, sol=sol, fixed=fixed, cols=cols, xr=xr64, ur=ur64, f=f64, act=A, sysf=sysf, h=h)


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
            if j not in c.setdefault("half", {}):                       # (kept: the directions of one system share them)
                d = np.zeros(nzx)
                d[j] = 0.5 * h
                d = d.reshape(c["xr"].shape)
                c["half"][j] = fd_times(c["sysf"](c["xr"] + d), c["sysf"](c["xr"] - d), 0.5 * h)
            c2[j] = c["half"][j]
        dz2 = solve([c2, cols[1], cols[2]])
    dX, dU = dz[:nzx].reshape(N + 1, NX), dz[nzx:].reshape(N, NU)
    return dU[0].copy(), dX, dU, dz2


def jvp_ref(oracle, cfg, x0, xr, ur, f, X, U, act=None, tx0=None, txr=None, tur=None, tf=None, h=0.125, pin_v=None):
    """jvp_apply at the iterate (X, U) with the pinned inputs of act (int8 [N,4] or None; pin_v: further (variable index, value) pins) held
    at their bounds."""
    return jvp_apply(jvp_system(oracle, cfg, x0, xr, ur, f, X, U, act, h, pin_v), tx0, txr, tur, tf)
