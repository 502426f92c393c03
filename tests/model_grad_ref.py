"""The exact gradient of one RTI iteration's QP in the cost weights Qd [10], Rd [4] and the mass, with a fixed active set, in plain numpy.

vjp_ref's system and adjoint: K [z; nu] = [-g; e] at the iterate (X, U) with the pinned inputs held at their bounds, K' [v; mu] = [gz; 0],
    dL/dtheta = [v; mu]' (de'/dtheta - dK/dtheta [z; nu]),   e' = [-g; e],
with the data derivatives by central differences of oracle.linearize in cfg.Qd[j], cfg.Rd[i] and cfg.mass.  The system is LINEAR in Qd and
Rd, so those differences are exact to rounding at any step.  In the mass it is not (the force enters as f / m), but it is affine in
u = 1 / m: the mass is differenced in u (cfg.mass = 1 / (u +- du)), exact to rounding as well if the mass enters through 1 / m alone, and
chained with du/dm = -1 / m^2.  That "if" is checked, not assumed: model_grad_ref returns the mass entry for two step sizes, and the tests
assert that they agree to 1e-9.
"""
import ctypes as C

import numpy as np

from tests.psens_ref import NU, NX, _system, fixed_of
from tests.vjp_ref import upstream


def _copy(cfg):
    c = type(cfg)()
    C.memmove(C.addressof(c), C.addressof(cfg), C.sizeof(cfg))
    return c


def _perturbed(cfg, j, d):
    """cfg with model entry j (0..9 Qd, 10..13 Rd, 14: 1 / mass) moved by d."""
    c = _copy(cfg)
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
    pin_v: optional list of (variable index, value) pins added to act's (the interior-point comparison pins the active velocity bounds)."""
    N = cfg.N
    A = None if act is None else np.asarray(act).reshape(N, NU)
    ff = None if (f is None or not cfg.use_fd) else np.asarray(f, dtype=np.float64)
    extra = list(pin_v or [])

    def system(c):
        qp = oracle.linearize(c, x0, xr, ur, ff, X, U)
        return _system(qp, fixed_of(qp, A) + extra)

    K, rhs0, nz = system(cfg)
    sol = np.linalg.solve(K, rhs0)
    adj = np.linalg.solve(K.T, np.concatenate([upstream(N, gu0, gX, gU), np.zeros(K.shape[0] - nz)]))

    def d(j, step):
        (Ka, ra, _), (Kb, rb, _) = system(_perturbed(cfg, j, step)), system(_perturbed(cfg, j, -step))
        return adj @ (((ra - rb) - (Ka - Kb) @ sol) / (2 * step))

    g = np.zeros(16)
    for j in range(14):
        w = cfg.Qd[j] if j < 10 else cfg.Rd[j - 10]
        g[j] = d(j, h * w if w > 0 else h)              # (a step relative to the weight: Rd stays positive)
    u = 1.0 / cfg.mass
    dm = -u * u
    g[14] = d(14, h * u) * dm                           # (without a force: 0 -- gravity and the thrust do not see the mass)
    return g, d(14, 0.5 * h * u) * dm
