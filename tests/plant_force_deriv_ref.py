"""The reference derivatives of the downwash force ON THE PLANT in float64, composed of tests/mlp_vjp_ref.vjp64, tests/mlp_jvp_ref.jvp64 and
the gather / scatter between the vehicles' states and the network's input rows:

    f[v] = scale * sum over the open slots k of net64((x[o_k] - x[v])[0:6]),   o_k = other_index[v][k]

a slot open iff 0 <= o_k < B and (no gate or |x[o_k].xy - x[v].xy|^2 < r_horiz^2, the forward's strict expression).  And the inputs of the
reference comparisons: vehicles SHARE states -- one vehicle is ego in its own slots and neighbour in others' -- so a slot cannot be redrawn
on its own.  A slot fails when its smallest float64 |pre-activation| is below mlp_vjp_ref.MARGIN (a ReLU that rounding may decide) or its
gate distance lies within 10 % of r_horiz^2; every failing slot's EGO vehicle gets a new state, and all slots are judged again, until none
fails (nothing is dropped from a comparison).  The loop is capped (MAX_ROUNDS) and the cap asserted: at K = 8 it does not terminate (each
vehicle sits in ~14 slots, and the chance that all pass falls below the chance that a redraw breaks another), so reference comparisons
use K <= 3.  Also the two-tick chain plant_force -> plant_step against tests/plant_deriv_ref.py.  Used by tests/test_plant_force_deriv.py
and tests/test_plant_force_deriv_gpu.py."""
import numpy as np
import torch

from ndp_nmpc_qd_amd import mlp_frag
from ndp_nmpc_qd_amd.params import nmpc_params as CP
from tests import mlp_jvp_ref as J
from tests import mlp_vjp_ref as R
from tests import plant_deriv_ref as P

MAX_ROUNDS = 40      # of the redraw loop (measured: 2 .. 8 rounds at K <= 3, see tests/test_plant_force_deriv.py)
R_HORIZ = 1.0        # ndp_cfg's default, the engines of the tests


def gather(x, idx, gate, r2=R_HORIZ * R_HORIZ):
    """x [B,10], idx int [B,K] -> (z [B,K,6] = (x[o] - x[v])[0:6] (0 on empty slots), open [B,K], d2 [B,K] the gate distances)."""
    B = x.shape[0]
    has = (idx >= 0) & (idx < B)
    o = np.where(has, idx, np.arange(B)[:, None])
    z = x[o][..., :6] - x[:, None, :6]
    d2 = z[..., 0] * z[..., 0] + z[..., 1] * z[..., 1]
    return z, has & ((d2 < r2) if gate else True), d2


def force64(blob, x, idx, gate=True, scale=1.0, r2=R_HORIZ * R_HORIZ):
    """f [B,3] float64.  r2: the gate's squared radius, here and in everything below (the default: ndp_cfg's default radius)."""
    z, op, _ = gather(x, idx, gate, r2)
    B, K = idx.shape
    f = R.vjp64(blob, z.reshape(-1, 6), np.zeros((B * K, 3)))[3].reshape(B, K, 3)
    return scale * (f * op[:, :, None]).sum(axis=1)


def scatter(gz, idx, B):
    """g_x [B,10] from g_z [B,K,6]: + on x[o][0:6], - on x[v][0:6]."""
    gx = np.zeros((B, 10))
    has = (idx >= 0) & (idx < B)
    np.add.at(gx[:, :6], idx[has], gz[has])
    gx[:, :6] -= (gz * has[:, :, None]).sum(axis=1)
    return gx


def vjp64(blob, x, idx, gf, gate=True, scale=1.0, r2=R_HORIZ * R_HORIZ):
    """The adjoint of force64: gf [B,3].  -> (g_z [B,K,6] per slot, 0 on closed and empty slots; g_x [B,10], its scatter; g_w [17859];
    margin [B,K] of every slot, open or not)."""
    B, K = idx.shape
    z, op, _ = gather(x, idx, gate, r2)
    up = scale * np.broadcast_to(gf[:, None], (B, K, 3)) * op[:, :, None]
    gz, gw, margin, _ = R.vjp64(blob, z.reshape(-1, 6), up.reshape(-1, 3))
    gz = gz.reshape(B, K, 6)
    return gz, scatter(gz, idx, B), gw, margin.reshape(B, K)


def jvp64(blob, x, idx, tx=None, tw=None, gate=True, scale=1.0, r2=R_HORIZ * R_HORIZ):
    """The tangent of force64 along tx [B,10] (None = 0) and tw [17859] (None = 0): df [B,3]."""
    B, K = idx.shape
    z, op, _ = gather(x, idx, gate, r2)
    tz = None
    if tx is not None:
        has = (idx >= 0) & (idx < B)
        o = np.where(has, idx, np.arange(B)[:, None])
        tz = (tx[o][..., :6] - tx[:, None, :6]).reshape(-1, 6)
    d = J.jvp64(blob, z.reshape(-1, 6), tz, tw)[0].reshape(B, K, 3)
    return scale * (d * op[:, :, None]).sum(axis=1)


def draw_states(rng, n):
    """n vehicle states: positions U(+-0.75), velocities U(+-1.5), a unit quaternion."""
    x = np.empty((n, 10))
    x[:, :3] = rng.uniform(-0.75, 0.75, (n, 3))
    x[:, 3:6] = rng.uniform(-1.5, 1.5, (n, 3))
    q = rng.normal(size=(n, 4))
    x[:, 6:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return x


def failing(blob, x, idx, p=None, r2=R_HORIZ * R_HORIZ):
    """[B,K] bool: the slots with a neighbour whose margin is below mlp_vjp_ref.MARGIN or whose gate distance is within 10 % of r_horiz^2
    (judged whether the gate is used or not: one case serves gate on and off)."""
    B, K = idx.shape
    z, has, d2 = gather(x, idx, False)
    with torch.no_grad():
        margin = R.forward64(R.params64(blob) if p is None else p, torch.tensor(z.reshape(-1, 6)))[1].numpy().reshape(B, K)
    return has & ((margin < R.MARGIN) | ((d2 > 0.9 * r2) & (d2 < 1.1 * r2)))


def shared_case(seed, blob, B, K, empty=0.15, r2=R_HORIZ * R_HORIZ):
    """States x [B,10] and random indices int32 [B,K] (never the vehicle itself; `empty` of the slots -1), redrawn until no slot fails
    at the gate radius of r2.  -> dict(x, index, rounds, redrawn)."""
    rng = np.random.default_rng(seed)
    x = draw_states(rng, B)
    idx = ((np.arange(B)[:, None] + 1 + rng.integers(0, max(B - 1, 1), (B, K))) % B).astype(np.int32)
    idx[rng.random((B, K)) < empty] = -1
    if B == 1:
        idx[:] = -1
    p = R.params64(blob)
    rounds, redrawn = 0, 0
    while True:
        bad = failing(blob, x, idx, p, r2).any(axis=1)
        if not bad.any():
            break
        rounds += 1
        assert rounds <= MAX_ROUNDS, f"the redraw loop does not terminate (B = {B}, K = {K})"
        x[bad] = draw_states(rng, int(bad.sum()))
        redrawn += int(bad.sum())
    return dict(x=x, index=idx, rounds=rounds + 1, redrawn=redrawn)


# ---------------------------------------------------------------- the chain: ticks of plant_force -> plant_step
def chain_forward(blob, x0, u, idx, gate=True, scale=1.0, dt=CP.ts_nmpc, substeps=4):
    """x0 [B,10], u [ticks,B,4] -> (xs [ticks+1,B,10] with xs[0] = x0, fs [ticks,B,3])."""
    xs, fs = [x0], []
    for k in range(u.shape[0]):
        fs.append(force64(blob, xs[-1], idx, gate, scale))
        xs.append(P.rollout(xs[-1], u[k:k + 1], fs[-1][None], dt=dt, substeps=substeps)[0])
    return np.array(xs), np.array(fs)


def chain_ok(blob, xs, idx):
    """No slot fails at any state the chain evaluates the force at."""
    return not any(failing(blob, x, idx).any() for x in xs[:-1])


def chain_vjp(blob, x0, u, idx, gxT, gate=True, scale=1.0, dt=CP.ts_nmpc, substeps=4):
    """The gradient of <gxT, x after the last tick>: (g_x0 [B,10], g_u [ticks,B,4], g_w [17859])."""
    xs, fs = chain_forward(blob, x0, u, idx, gate, scale, dt, substeps)
    B = x0.shape[0]
    gx, gu, gw = gxT, np.zeros_like(u), np.zeros(mlp_frag.NPARAM)
    for k in reversed(range(u.shape[0])):
        Jk = P.jacobian(xs[k], u[k:k + 1], fs[k][None], dt=dt, substeps=substeps)
        gx_p, gu_k, gf_k = P.vjp(Jk, gx[None])
        _, gx_f, gw_k, _ = vjp64(blob, xs[k], idx, gf_k[0], gate, scale)
        gx, gu[k], gw = gx_p + gx_f, gu_k[0], gw + gw_k
    assert gx.shape == (B, 10)
    return gx, gu, gw


def chain_jvp(blob, x0, u, idx, tx0, tu, tw, gate=True, scale=1.0, dt=CP.ts_nmpc, substeps=4):
    """The tangent of the state after the last tick along tx0 [B,10], tu [ticks,B,4], tw [17859]: [B,10]."""
    xs, fs = chain_forward(blob, x0, u, idx, gate, scale, dt, substeps)
    dx = tx0
    for k in range(u.shape[0]):
        df = jvp64(blob, xs[k], idx, dx, tw, gate, scale)
        Jk = P.jacobian(xs[k], u[k:k + 1], fs[k][None], dt=dt, substeps=substeps)
        dx = P.jvp(Jk, dx[:, None], tu[k][None, :, None], df[None, :, None])[0, :, 0]
    return dx


def chain_case(seed, blob, B, K, ticks):
    """A shared-state case (no empty slot) with inputs u [ticks,B,4] from the plant's envelope in which no slot fails at any state the
    chain evaluates the force at; seeds are tried in order from `seed` (a later state cannot be redrawn).  -> dict(x, index, u, seed)."""
    for s in range(seed, seed + 50):
        c = shared_case(s, blob, B, K, empty=0.0)
        u = P.inputs(B, ticks, s)[1]
        xs, fs = chain_forward(blob, c["x"], u, c["index"])
        _, op, _ = gather(xs[-2], c["index"], True)
        if chain_ok(blob, xs, c["index"]) and op.any():
            return dict(x=c["x"], index=c["index"], u=u, seed=s)
    raise AssertionError("no seed gives a chain without a failing slot")
