"""An optimality certificate for one RTI iteration's QP, in plain numpy: does a returned step satisfy the QP's KKT conditions?

The QP is the one oracle.linearize builds (pinned to tests/ref_numpy.py by test_oracle_pins.py):

    min  sum_k 1/2 dx_k' Q_k dx_k + q_k' dx_k + 1/2 du_k' diag(Rd_k) du_k + r_k' du_k   (+ stage N's state terms)
    s.t. dx_0 = dx0,  dx_{k+1} = A_k dx_k + B_k du_k + b_k,  lu_k <= du_k <= uu_k,  lv_k <= dv_k <= uv_k (k = 1..N-1)

No QP solver is called.  The costates follow from the step by one backward pass, and the input box's KKT conditions are then one
number: the natural residual |du - P(du - g)| (P = projection onto the box, g = the reduced input gradient), which is zero exactly
when every free input has g = 0 and every input on a bound has a multiplier of the right sign.  It means the same for an active-set
answer (inputs exactly on their bounds) and an interior-point one (inputs within the barrier's reach of them).

The velocity bounds' multipliers are not covered: an instance with a velocity within `vel_flag` of its bound is FLAGGED, and its
stationarity residual says nothing (the caller holds such instances to another solver instead).
"""
import numpy as np

NX, NU = 10, 4


def _scale(*terms):
    return max(max(float(np.max(np.abs(t))) if np.size(t) else 0.0 for t in terms), 1e-300)


def certificate(qp, dx, du, vel_flag=1e-6, on_bound=1e-9):
    """qp: dict of oracle.linearize; dx [N+1,10], du [N,4]: the step.  Returns a dict of
      eq     equality residual (initial state and dynamics), over the largest term of those rows
      stat   natural residual of the input box with g scaled by the largest term of g (|Rd du|, |r|, |B' lam|)
      vbox   violation of the velocity bounds (stages 1..N-1), absolute
      flag   True when a velocity lies within vel_flag of a bound (stat does not cover that instance then)
      act    int8 [N,4] implied active set, +1 on the upper / -1 on the lower input bound (active_set()'s encoding)
      g      the reduced input gradient [N,4] (unscaled), lam the costates [N+1,10]
    """
    A, B, b, Q, q, Rd, r = (qp[k] for k in ("A", "B", "b", "Q", "q", "Rd", "r"))
    lu, uu, lv, uv = qp["lu"], qp["uu"], qp["lv"], qp["uv"]
    N = A.shape[0]
    dx, du = np.asarray(dx, dtype=np.float64), np.asarray(du, dtype=np.float64)
    assert dx.shape == (N + 1, NX) and du.shape == (N, NU)

    Adx = np.einsum("kij,kj->ki", A, dx[:N])
    Bdu = np.einsum("kij,kj->ki", B, du)
    e_dyn = dx[1:] - Adx - Bdu - b
    e_0 = dx[0] - qp["dx0"]
    eq = max(float(np.abs(e_dyn).max()), float(np.abs(e_0).max())) / _scale(dx, Adx, Bdu, b, qp["dx0"])

    lam = np.zeros((N + 1, NX))
    lam[N] = Q[N] @ dx[N] + q[N]
    for k in range(N - 1, -1, -1):
        lam[k] = Q[k] @ dx[k] + q[k] + A[k].T @ lam[k + 1]
    Blam = np.einsum("kji,kj->ki", B, lam[1:])
    g = Rd * du + r + Blam
    gs = g / _scale(Rd * du, r, Blam)
    stat = float(np.abs(du - np.clip(du - gs, lu, uu)).max())

    dv, lo, hi = dx[1:N, 3:6], lv[1:N], uv[1:N]
    vbox = float(max(0.0, (lo - dv).max(initial=0.0), (dv - hi).max(initial=0.0)))
    flag = bool(np.minimum(np.abs(dv - lo), np.abs(hi - dv)).min(initial=np.inf) < vel_flag)

    tol_u = on_bound * np.maximum(1.0, np.maximum(np.abs(lu), np.abs(uu)))
    act = np.where(du >= uu - tol_u, 1, np.where(du <= lu + tol_u, -1, 0)).astype(np.int8)
    return dict(eq=eq, stat=stat, vbox=vbox, flag=flag, act=act, g=g, lam=lam)


def worst(c):
    """One number for a pass / fail bar: the largest of the three residuals (meaningless for a flagged instance)."""
    return max(c["eq"], c["stat"], c["vbox"])


def certify_batch(oracle, cfg, x0, xr, ur, f, X_old, U_old, X_new, U_new, **kw):
    """The certificate of every instance of a batch step: X_old / U_old the iterate the step started from, X_new / U_new the one it
    returned (cfg: an oracle cfg with the handle's N, use_fd).  Returns a list of certificate dicts."""
    out = []
    for i in range(x0.shape[0]):
        qp = oracle.linearize(cfg, x0[i], xr[i], ur[i], None if f is None else f[i], X_old[i], U_old[i])
        out.append(certificate(qp, X_new[i] - X_old[i], U_new[i] - U_old[i], **kw))
    return out
