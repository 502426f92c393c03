"""The exact initial-state sensitivity of one RTI iteration's QP with a fixed active set, in plain numpy.

The QP is the one oracle.linearize builds at the iterate the step started from (pinned to tests/ref_numpy.py).  With the set held
fixed its solution is affine in dx_0, and the derivative is the solution of the HOMOGENEOUS problem (b = q = r = 0, the pinned inputs
held at 0) with dx_0 = e_j -- the same dense KKT system as ref_numpy.kkt_solve, factored once for all ten right-hand sides.
"""
import numpy as np

NX, NU = 10, 4


def sens_ref(qp, act=None):
    """qp: dict of oracle.linearize; act: int8 [N,4] (nonzero = the input is pinned on a bound), or None.
    Returns (du0 [4,10], dU [N,4,10], dX [N+1,10,10]): column j is the derivative with respect to x0[j]."""
    A, B, Q, Rd = (np.asarray(qp[k], dtype=np.float64) for k in ("A", "B", "Q", "Rd"))
    N = A.shape[0]
    nz = (N + 1) * NX + N * NU
    uo = (N + 1) * NX
    pins = [] if act is None else [uo + k * NU + i for k, i in zip(*np.nonzero(np.asarray(act).reshape(N, NU)))]
    H = np.zeros((nz, nz))
    for k in range(N + 1):
        H[k * NX:(k + 1) * NX, k * NX:(k + 1) * NX] = Q[k]
    for k in range(N):
        H[uo + k * NU:uo + (k + 1) * NU, uo + k * NU:uo + (k + 1) * NU] = np.diag(Rd[k])
    ne = (N + 1) * NX + len(pins)
    E = np.zeros((ne, nz))
    E[0:NX, 0:NX] = np.eye(NX)
    for k in range(N):
        r = slice((k + 1) * NX, (k + 2) * NX)
        E[r, (k + 1) * NX:(k + 2) * NX] = np.eye(NX)
        E[r, k * NX:(k + 1) * NX] = -A[k]
        E[r, uo + k * NU:uo + (k + 1) * NU] = -B[k]
    for i, v in enumerate(pins):
        E[(N + 1) * NX + i, v] = 1.0
    KKT = np.block([[H, E.T], [E, np.zeros((ne, ne))]])
    rhs = np.zeros((nz + ne, NX))
    rhs[nz:nz + NX, :] = np.eye(NX)
    Z = np.linalg.solve(KKT, rhs)[:nz]
    dX = Z[:uo].reshape(N + 1, NX, NX)
    dU = Z[uo:].reshape(N, NU, NX)
    dX[0] = np.eye(NX)                  # (the initial-state rows, exact)
    for v in pins:                      # exactly 0, as the device writes them
        k, i = divmod(v - uo, NU)
        dU[k, i, :] = 0.0
    return dU[0].copy(), dU, dX


def scale(K):
    """The bar's scale: max(1, |K|max)."""
    return max(1.0, float(np.max(np.abs(K))))
